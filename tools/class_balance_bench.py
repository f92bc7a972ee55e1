#!/usr/bin/env python
"""What the class-balance path costs and what it changes: the counting pass of csrc/label_stats.hip, the second pick rule of
csrc/augment.hip, and the class shares of the batches with rare-class sampling and without it.

    python tools/class_balance_bench.py [--frames 1569] [--resident 64] [--batches 200] [--out profiles/class_balance_bench.txt]

  count    hipEvent time of ops.label_stats over FRAMES x 480 x 640 synthetic uint8 labels (one launch), beside torch.bincount
           called per frame on the device
  pick     ops.augment_pick_class beside ops.augment_pick on the same prepared records, batch 4, crop 512
  shares   per-class pixel shares of BATCHES batches of AugmentedBatches over RESIDENT synthetic frames, with a
           RareClassSampler and without one; the batch labels are counted with ops.label_stats (the int64 entry)

The labels are synthetic and made to be imbalanced (background about nine tenths, the higher classes ever rarer): the shares
say what the sampler does to such a set, not what it does to a data set.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, CROP, BATCH, N_CLASS = 480, 640, 512, 4, 9


def imbalanced_labels(n, seed, device):
    """(n, H, W) uint8 on the device: class 0 with up to four rectangles a frame; class c is drawn with probability ~ 2^-c and its
    rectangles shrink with c"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    lab = torch.zeros((n, H, W), dtype=torch.uint8, device=device)
    ys, xs = torch.arange(H, device=device)[None, :, None], torch.arange(W, device=device)[None, None, :]
    p = torch.tensor([2.0 ** -c for c in range(1, N_CLASS)])
    for _ in range(4):
        cls = torch.multinomial(p, n, replacement=True, generator=g) + 1
        on = torch.rand(n, generator=g) < 0.6
        side = (320.0 / cls.float().sqrt()).long()
        rh, rw = (torch.rand(n, generator=g) * side).long() + 8, (torch.rand(n, generator=g) * side).long() + 8
        y0, x0 = (torch.rand(n, generator=g) * (H - rh)).long(), (torch.rand(n, generator=g) * (W - rw)).long()
        for lo in range(0, n, 128):
            s = slice(lo, lo + 128)
            d = lambda t: t[s].to(device)[:, None, None]
            box = (ys >= d(y0)) & (ys < d(y0 + rh)) & (xs >= d(x0)) & (xs < d(x0 + rw)) & d(on)
            lab[s] = torch.where(box, d(cls).to(torch.uint8), lab[s])
    return lab


def timed(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=1569)
    ap.add_argument("--resident", type=int, default=64)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--min-pixels", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_balance_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("class_balance_bench measures on the MI355X: no device, no numbers")
    from segmif_amd import data, ops
    lines = [f"# tools/class_balance_bench.py: {a.frames} x {H} x {W} synthetic uint8 labels, batch {BATCH}, crop {CROP}, "
             f"{torch.cuda.get_device_name(0)}; device events, warm", "#"]

    # ---- count
    labels = imbalanced_labels(a.frames, 0, "cuda")
    mb = labels.numel() / 1e6
    ours = ops.label_stats(labels)
    theirs = torch.stack([torch.bincount(f.reshape(-1), minlength=256) for f in labels])
    if not torch.equal(ours[:, :256], theirs) or ours[:, 256].any():
        raise RuntimeError("label_stats and torch.bincount disagree")
    ms = timed(lambda: ops.label_stats(labels), 200)
    ms_bc = timed(lambda: [torch.bincount(f.reshape(-1), minlength=256) for f in labels], 2, warm=1)
    lines.append(f"count:  ops.label_stats, one launch over the set ({mb:.0f} MB)        {ms:9.3f} ms   {mb / ms:7.1f} GB/s")
    lines.append(f"        torch.bincount per frame on the device ({a.frames} calls)       {ms_bc:9.3f} ms   {mb / ms_bc:7.1f} GB/s   (equal tables)")
    share = ours[:, :N_CLASS].sum(0).double()
    lines.append("        class shares of the set: " + " ".join(f"{c}:{v:.4f}" for c, v in enumerate((share / share.sum()).tolist())))
    del theirs

    # ---- pick
    src = data.synthetic_pairs(a.resident, H, W, seed=0)
    src["label"] = labels[:a.resident].cpu().numpy()
    ds = data.DeviceDataset.from_arrays(**src)
    stats = ds.label_stats()
    plain = data.AugmentedBatches(ds, batch=BATCH, crop_size=CROP, seed=0)
    params = plain.draw(BATCH)
    rec, tab = data.pack_records(list(range(BATCH)), params, H, W)
    rec_d, tab_d = torch.from_numpy(rec).cuda(), torch.from_numpy(tab).cuda()
    rare = int(np.argmin(np.where(stats.pixels > 0, stats.pixels, np.iinfo(np.int64).max)))
    want = torch.tensor([[rare, 1500]] * BATCH, dtype=torch.int32, device="cuda")
    tally = torch.zeros((N_CLASS, 2), dtype=torch.int64, device="cuda")
    ms_pick = timed(lambda: ops.augment_pick(ds.label, rec_d, tab_d, CROP, CROP), 200)
    ms_class = timed(lambda: ops.augment_pick_class(ds.label, rec_d, tab_d, CROP, CROP, want, tally), 200)
    ms_apply = timed(lambda: ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, CROP, CROP), 200)
    lines.append(f"pick:   ops.augment_pick {ms_pick:.4f} ms, ops.augment_pick_class {ms_class:.4f} ms (the call allocates its `got`), "
                 f"beside ops.augment_apply {ms_apply:.4f} ms")

    # ---- shares
    def shares(sampler):
        it = data.AugmentedBatches(ds, batch=BATCH, crop_size=CROP, seed=1, sampler=sampler)
        total = torch.zeros(257, dtype=torch.int64, device="cuda")
        for _ in range(a.batches):
            total += ops.label_stats(next(it)[4]).sum(0)
        t = total.cpu().numpy()
        return t[:N_CLASS] / t[:N_CLASS].sum(), t[255] / t.sum(), (it.rcs_tally() if sampler is not None else None)

    sampler = data.RareClassSampler(stats, range(len(ds)), min_pixels=a.min_pixels, seed=1)
    with_, ign_w, tally_w = shares(sampler)
    without, ign_o, _ = shares(None)
    lines.append(f"shares: labelled-pixel shares of {a.batches} batches over {a.resident} resident frames (set: "
                 + " ".join(f"{c}:{v:.4f}" for c, v in enumerate(stats.freq)) + ")")
    lines.append("        sequential loader:    " + " ".join(f"{c}:{v:.4f}" for c, v in enumerate(without)) + f"   padding {ign_o:.3f}")
    lines.append("        rare-class sampling:  " + " ".join(f"{c}:{v:.4f}" for c, v in enumerate(with_)) + f"   padding {ign_w:.3f}")
    lines.append("        sampling probability: " + " ".join(f"{c}:{v:.4f}" for c, v in enumerate(sampler.prob))
                 + (f"   dropped: {sampler.dropped}" if sampler.dropped else ""))
    lines.append("        drawn/hit per class:  " + " ".join(f"{c}:{int(d)}/{int(h)}" for c, (d, h) in enumerate(tally_w)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
