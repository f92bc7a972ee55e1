#!/usr/bin/env python
"""What a training batch costs to make: the device pass of segmif_amd.data (csrc/augment.hip) against the same transform on the
host, next to the segmentation step that consumes the batch.

    python tools/augment_bench.py [--batch 8] [--frames 64] [--backbone mit_b3] [--out profiles/augment_bench.txt]

  device   hipEvent time of one AugmentedBatches step (upload + pick + apply), warm, 480 x 640 -> 512, and of the two kernels
           alone on prepared records; the host time of drawing the parameters and building the tables is listed apart
  host     the same transform per batch through PIL / numpy (three bilinear resizes, one nearest, flip, brightness / contrast,
           float32 pad, up to ten np.unique passes, crop, / 255, transpose) in one process and on a pool of at most 16 threads
  step     seg_train_step on the batch, same run
"""
import argparse
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def host_sample(ir, vis, mask, label, p, crop):
    """the loader's per-sample work with PIL and numpy, from drawn parameters p"""
    from PIL import Image
    size = (p["nw"], p["nh"])
    rs = lambda a, how: np.asarray(Image.fromarray(a).resize(size, resample=how))
    ir3 = rs(np.repeat(ir[:, :, None], 3, 2), Image.BILINEAR).astype(np.float32)
    vis3 = rs(vis, Image.BILINEAR).astype(np.float32)
    mask3 = rs(np.repeat(mask[:, :, None], 3, 2), Image.BILINEAR).astype(np.float32)
    lab = rs(label, Image.NEAREST)
    if p["flip"]:
        ir3, vis3, mask3, lab = np.fliplr(ir3), np.fliplr(vis3), np.fliplr(mask3), np.fliplr(lab)
    if p["bright_on"]:
        vis3 = np.clip(vis3.astype(np.float32) + np.float32(p["beta"]), 0, 255).astype(np.uint8)
    if p["contrast_on"]:
        vis3 = np.clip(vis3.astype(np.float32) * np.float32(p["alpha"]), 0, 255).astype(np.uint8)
    H, W = p["H"], p["W"]
    pads = []
    for img in (ir3, vis3, mask3):
        c = np.zeros((H, W, 3), dtype=np.float32)
        c[:] = (123.675, 116.28, 103.53)
        c[p["pad_h"]:p["pad_h"] + p["nh"], p["pad_w"]:p["pad_w"] + p["nw"]] = img
        pads.append(c)
    pl = np.ones((H, W), dtype=np.float32) * 255
    pl[p["pad_h"]:p["pad_h"] + p["nh"], p["pad_w"]:p["pad_w"] + p["nw"]] = lab
    for hs, ws in p["cand"]:
        index, cnt = np.unique(pl[hs:hs + crop, ws:ws + crop], return_counts=True)
        cnt = cnt[index != 255]
        if len(cnt) and np.max(cnt) / np.sum(cnt) < 0.75:
            break
    return [np.transpose(c[hs:hs + crop, ws:ws + crop] / 255.0, (2, 0, 1)) for c in pads] + [pl[hs:hs + crop, ws:ws + crop]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--backbone", default="mit_b3")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    a = ap.parse_args()
    import detweights as dw
    from segmif_amd import data, ops, train
    from segmif_amd.core import Network3
    H, W, crop, B = 480, 640, 512, a.batch
    src = data.synthetic_pairs(a.frames, H, W, seed=0)
    ds = data.DeviceDataset.from_arrays(**src)
    it = data.AugmentedBatches(ds, batch=B, crop_size=crop, seed=0)
    lines = [f"# tools/augment_bench.py: {B} samples per batch, {H} x {W} -> {crop}, {a.frames} resident synthetic frames, "
             f"{torch.cuda.get_device_name(0)}", "#"]

    def timed(fn, n):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, 1e3 * (time.perf_counter() - t0) / n

    dev_ms, wall_ms = timed(lambda: next(it), a.iters)
    lines.append(f"device: one AugmentedBatches step (draw, tables, upload, pick, apply)  events {dev_ms:8.3f} ms   wall {wall_ms:8.3f} ms")
    idx = list(range(B))
    params = it.draw(B)
    t0 = time.perf_counter()
    for _ in range(20):
        rec, tab = data.pack_records(idx, it.draw(B), H, W)
    host_prep = 1e3 * (time.perf_counter() - t0) / 20
    lines.append(f"        of that on the host: parameters + Pillow tables (numpy)           wall {host_prep:8.3f} ms   "
                 f"({(rec.nbytes + tab.nbytes) / 1e3:.0f} kB uploaded)")
    rec, tab = data.pack_records(idx, params, H, W)
    dev = torch.from_numpy(np.concatenate([rec.reshape(-1), tab])).cuda()
    rec_d, tab_d = dev[:rec.size].view(B, -1), dev[rec.size:]
    pick_ms, _ = timed(lambda: ops.augment_pick(ds.label, rec_d, tab_d, crop, crop), a.iters)
    apply_ms, _ = timed(lambda: ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, crop, crop), a.iters)
    out_mb = B * crop * crop * (9 * 4 + 8) / 1e6
    lines.append(f"        kernels alone: pick {pick_ms:.3f} ms, apply {apply_ms:.3f} ms (writes {out_mb:.0f} MB: {out_mb / apply_ms:.0f} GB/s)")
    try:
        import PIL  # noqa: F401
        sets = [it.draw(B) for _ in range(4)]
        one = lambda p_i: host_sample(src["ir"][p_i[1]], src["vis"][p_i[1]], src["mask"][p_i[1]], src["label"][p_i[1]], p_i[0], crop)
        t0 = time.perf_counter()
        for ps in sets:
            [one((p, i)) for i, p in enumerate(ps)]
        lines.append(f"host:   the same transform through PIL / numpy, one process, one thread    wall {1e3 * (time.perf_counter() - t0) / len(sets):8.3f} ms per batch")
        threads = min(16, B)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            list(ex.map(one, [(p, i) for i, p in enumerate(sets[0])]))
            t0 = time.perf_counter()
            for ps in sets:
                list(ex.map(one, [(p, i) for i, p in enumerate(ps)]))
            lines.append(f"host:   the same on a pool of {threads} threads                                   wall {1e3 * (time.perf_counter() - t0) / len(sets):8.3f} ms per batch")
    except ImportError:
        lines.append("host:   PIL does not import here: the host side was not timed")
    torch.manual_seed(0)
    random.seed(0)
    seg = Network3(a.backbone, 9, pretrained=None)
    dw.load_det_weights(seg, seed=0)
    seg = seg.cuda().eval()  # (the regime tools/train_bench.py times)
    opt = train.make_seg_optimizer(seg, max_iter=80000)
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    _, _, vis3, _, label = next(it)
    step_ms, step_wall = timed(lambda: train.seg_train_step(seg, opt, vis3, label, crit), 10)
    lines.append(f"step:   seg_train_step {a.backbone} on the batch ({B} x 3 x {crop} x {crop})              events {step_ms:8.3f} ms   wall {step_wall:8.3f} ms")
    lines.append(f"#\n# device pass / step = {100 * dev_ms / step_ms:.2f} % (events), {100 * wall_ms / step_wall:.2f} % (wall)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
