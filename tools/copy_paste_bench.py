#!/usr/bin/env python
"""What instance copy-paste costs on the device: the bank build stage by stage, ops.copy_paste beside ops.class_mix, the same paste
from torch operators and ops.augment_apply, and one loader step with paste=None of this tree next to the parent commit's.

    python tools/copy_paste_bench.py [--frames 1569] [--max-bytes N] [--iters 200] [--rounds 5] [--parent-tree DIR] [--out profiles/copy_paste_bench.txt]

  1. the bank of N synthetic frames of 480 x 640 (data.synthetic_pairs): device-event time of the labeller (connected_components),
     of the boxes calls, of the pack calls and of ObjectBank.build as a whole (which also holds the readback, the sort and the
     uploads), median [min .. max] over the rounds; objects and bytes; and the same boxes from scipy.ndimage (label + find_objects per
     class, on the host, copies included) after the records were compared for equality.
  2. ops.copy_paste at batch 4 and 8, crop 512, three objects in every sample, against ops.class_mix on the same batch (the cost of the
     plain copy it contains), the same paste composed from torch operators on the device (results compared for equal bits first)
     and ops.augment_apply; alternating inside each round.
  3. with --parent-tree DIR (a built checkout of the parent commit): one AugmentedBatches step with default arguments (paste=None)
     of this tree against the parent's, in fresh child processes, alternating.

The frames are synthetic: the numbers say what the passes cost, nothing about what pasting does to a data set.
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CROP, N_CLASS = 480, 640, 512, 9
CACHE = 256e6  # the Infinity Cache, bytes


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:10.4f} ms  [{ts[0]:10.4f} .. {ts[-1]:10.4f}]"


def alternating(cand, iters, rounds):
    for fn in cand.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in cand}
    for _ in range(rounds):
        for k, fn in cand.items():
            res[k].append(timed(fn, iters))
    return res


def host_boxes(label, min_area, max_box):
    """the records of the bank from scipy.ndimage on the host: label + find_objects per class, the root as the minimum index"""
    from scipy import ndimage as ndi
    lab_h = label.cpu().numpy()
    out = []
    structure = np.ones((3, 3), dtype=int)
    for f in range(len(lab_h)):
        for c in range(1, N_CLASS):
            lab, n = ndi.label(lab_h[f] == c, structure=structure)
            if not n:
                continue
            area = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
            first = ndi.minimum(np.arange(H * W).reshape(H, W), lab, index=np.arange(1, n + 1)).astype(np.int64)
            for i, (sy, sx) in enumerate(ndi.find_objects(lab)):
                bw, bh = sx.stop - sx.start, sy.stop - sy.start
                if area[i] >= min_area and bw * bh <= max_box:
                    out.append((f, int(first[i]), c, int(area[i]), sx.start, sy.start, bw, bh))
    return np.asarray(sorted(out), dtype=np.int32).reshape(-1, 8)


def bank_build(a, lines):
    from segmif_amd import data, ops
    from segmif_amd.utils.objects import connected_components
    ds = data.DeviceDataset.from_arrays(**data.synthetic_pairs(a.frames, H, W, seed=0))
    bank = data.ObjectBank.build(ds, max_bytes=a.max_bytes)
    chunk = 32
    spans = [(f, min(chunk, a.frames - f)) for f in range(0, a.frames, chunk)]
    lab32 = [ds.label[f:f + n].to(torch.int32) for f, n in spans]
    roots = [connected_components(m, N_CLASS)[0] for m in lab32]
    records, counter = torch.empty((len(bank) + 16, 8), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    work = [None]

    def boxes():
        counter.zero_()
        for (f, n), root in zip(spans, roots):
            work[0] = ops.object_boxes(root, ds.label[f:f + n], N_CLASS, 0x1fe, 64, H * W // 4, records, counter, frame0=f, workspace=work[0])

    def pack():
        for (f, n), root in zip(spans, roots):
            m0, m1 = (int(v) for v in np.searchsorted(bank.records_host[:, 0], [f, f + n]))
            if m1 > m0:
                ops.object_pack(bank.records[m0:m1], bank.offsets[m0:m1 + 1], bank.patches, root, ds.ir[f:f + n], ds.vis[f:f + n], ds.mask[f:f + n], frame0=f)

    res = alternating({"labeller (connected_components) ": lambda: [connected_components(m, N_CLASS) for m in lab32],
                       "boxes (3 launches a chunk)       ": boxes, "pack (1 launch a chunk)          ": pack,
                       "ObjectBank.build, all of it      ": lambda: data.ObjectBank.build(ds, max_bytes=a.max_bytes)}, max(1, a.iters // 100), a.rounds)
    boxes()
    if int(counter.item()) != len(bank):
        raise RuntimeError("the boxes calls and the bank disagree on the number of objects")
    t0 = time.perf_counter()
    host = host_boxes(ds.label, 64, H * W // 4)
    host_ms = (time.perf_counter() - t0) * 1e3
    if not np.array_equal(host, bank.records_host):
        raise RuntimeError("the bank's records and scipy.ndimage's disagree")
    lines.append(f"bank of {a.frames} synthetic frames of {H} x {W}: {len(bank)} objects, {bank.patches.numel()} bytes of patches "
                 f"({bank.nbytes} with records and offsets; max_bytes {a.max_bytes}, every other argument of ObjectBank.build at its default); "
                 f"chunks of {chunk} frames; records equal scipy.ndimage's")
    for row in bank.table():
        lines.append("  " + row)
    for k, ts in res.items():
        lines.append(f"  {k} {spread(ts)}")
    lines.append(f"  scipy.ndimage on the host (label + find_objects per class, the copy included)   {host_ms:10.1f} ms, once")
    resident = ds.label.numel() * 6 / 1e6
    lines.append(f"  note: the resident set is {resident:.0f} MB and the root maps {ds.label.numel() * 4 / 1e6:.0f} MB: neither fits the 256 MB Infinity Cache; "
                 f"the patch store ({bank.patches.numel() / 1e6:.1f} MB) " + ("does" if bank.patches.numel() < CACHE else "does not"))
    lines.append("#")
    return ds, bank


def torch_paste(ir3, vis3, mask3, label, bank, table):
    """the rule from torch operators: slots first to last, a gather of the patch pixels per slot and torch.where per tensor"""
    out = [ir3.clone(), vis3.clone(), mask3.clone(), label.clone()]
    B, h, w = label.shape
    ys, xs = torch.arange(h, device=label.device)[:, None], torch.arange(w, device=label.device)[None, :]
    rec, off = bank.records_host, bank.offsets_host
    unit = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(label.device)  # byte / 255, rounded to nearest
    for b in range(B):
        for obj, dx, dy, ow, oh, sx, sy, flip in table[b].tolist():
            if obj < 0:
                continue
            cls, bw, bh = int(rec[obj, 2]), int(rec[obj, 6]), int(rec[obj, 7])
            u, v = xs - dx, ys - dy
            inside = (u >= 0) & (u < ow) & (v >= 0) & (v < oh)
            su = torch.clamp((u.clamp(0, ow - 1) * sx + (sx >> 1)) >> 16, max=bw - 1)
            if flip & 1:
                su = bw - 1 - su
            sv = torch.clamp((v.clamp(0, oh - 1) * sy + (sy >> 1)) >> 16, max=bh - 1)
            px = bank.patches[int(off[obj]) + sv * bw + su]  # (h, w, 8)
            on = inside & (px[..., 5] == 1)
            val = unit[px.long()]
            for c in range(3):
                out[0][b, c] = torch.where(on, val[..., 0], out[0][b, c])
                out[1][b, c] = torch.where(on, val[..., 1 + c], out[1][b, c])
                out[2][b, c] = torch.where(on, val[..., 4], out[2][b, c])
            out[3][b] = torch.where(on, torch.full_like(out[3][b], cls), out[3][b])
    return out


def paste(a, lines, ds, bank):
    from segmif_amd import data, ops
    for B in (4, 8):
        it = data.AugmentedBatches(ds, batch=B, crop_size=CROP, seed=1)
        params = it.draw(B)
        rec, tab = data.pack_records(list(range(B)), params, H, W)
        rec_d, tab_d = torch.from_numpy(rec).cuda(), torch.from_numpy(tab).cuda()
        ops.augment_pick(ds.label, rec_d, tab_d, CROP, CROP)
        batch = ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, CROP, CROP)
        policy = data.CopyPaste(bank, prob=1.0, max_objects=3, seed=B)
        table_h = policy.draw(B, CROP, CROP)
        while (table_h[:, :, 0] < 0).any():  # three objects in every sample
            table_h = np.where((table_h[:, :, :1] < 0), policy.draw(B, CROP, CROP), table_h)
        table = torch.from_numpy(np.ascontiguousarray(table_h)).cuda()
        mix_table = torch.from_numpy(data.ClassMix(prob=1.0, n_class=N_CLASS, seed=B).draw(B)).cuda()
        got = ops.copy_paste(*batch, bank, table, N_CLASS)
        want = torch_paste(*batch, bank, table_h)
        for x, y in zip(got[:4], want):
            same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.is_floating_point() else torch.equal(x, y)
            if not same:
                raise RuntimeError("ops.copy_paste and the torch composition disagree")
        res = alternating({"ops.copy_paste (memset + 1 launch, 5 allocations)": lambda: ops.copy_paste(*batch, bank, table, N_CLASS),
                           "ops.class_mix (3 launches, 6 allocations)        ": lambda: ops.class_mix(*batch, mix_table, N_CLASS),
                           "ops.augment_apply for the same records           ": lambda: ops.augment_apply(ds.ir, ds.vis, ds.mask, ds.label, rec_d, tab_d, CROP, CROP)},
                          a.iters, a.rounds)
        res["the same paste from torch operators (equal bits) "] = [timed(lambda: torch_paste(*batch, bank, table_h), max(2, a.iters // 50)) for _ in range(a.rounds)]
        px = B * CROP * CROP
        used = np.unique(table_h[:, :, 0])
        touched = int((bank.records_host[used, 6].astype(np.int64) * bank.records_host[used, 7]).sum()) * 8
        moved, store = 2 * px * 44 + touched, bank.patches.numel()
        lines.append(f"B = {B}, crop {CROP}, 3 objects a sample: {int(got[4].sum())} of {px} pixels pasted ({float(got[4].sum()) / px:.4f}); a batch and "
                     f"its copy are {2 * px * 44 / 1e6:.0f} MB, the patches of the table's {len(used)} objects {touched / 1e6:.2f} MB: together they "
                     + ("fit" if moved < CACHE else "do NOT fit") + " the Infinity Cache and every timed call reuses them, so the figures are cache-warm; "
                     f"the whole store ({store / 1e6:.0f} MB) " + ("fits too" if store + 2 * px * 44 < CACHE else "does NOT fit: a training step's paste, with "
                     "other objects every step, reads its patches from HBM"))
        for k, ts in res.items():
            lines.append(f"  {k} {spread(ts)}")
    lines.append("#")


def registers():
    from segmif_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "copy_paste.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return ["# registers: NOT recorded (the compile failed)"]
    out = ["# hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:"]
    for name in ("boxes_init_kernel", "boxes_gather_kernel", "boxes_emit_kernel", "pack_kernel", "paste_kernel"):
        block = r.stderr.split(name, 1)[-1]
        field = lambda f: (re.search(f + r": (\d+)", block) or [None, "?"])[1]
        scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
        out.append(f"#   {name}: {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, occupancy {occ} waves/SIMD, "
                   f"LDS {lds} bytes a workgroup")
    return out


def child_step(iters):
    """this process's tree: median device-event ms of one AugmentedBatches step with default arguments, printed as the last line"""
    from segmif_amd import data
    ds = data.DeviceDataset.from_arrays(**data.synthetic_pairs(32, H, W, seed=0))
    it = data.AugmentedBatches(ds, batch=8, crop_size=CROP, seed=1)
    for _ in range(5):
        out = next(it)
    torch.cuda.synchronize()
    ts = sorted(timed(lambda: next(it), iters) for _ in range(5))
    out = next(it)
    print(f"STEP {ts[2]:.4f} {ts[0]:.4f} {ts[-1]:.4f} {len(out)} {int(out[4].sum())}")


def against_parent(a, lines):
    if not a.parent_tree:
        lines.append("# one AugmentedBatches step of this tree against the parent commit: not measured (no --parent-tree)")
        return
    n = max(20, a.iters)
    res = {"this tree": [], "parent   ": []}
    for _ in range(2):
        for k, tree in (("this tree", ROOT), ("parent   ", os.path.abspath(a.parent_tree))):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child-step", tree, "--iters", str(n)],
                               cwd=tree, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"the child on {tree} ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            res[k].append(r.stdout.strip().splitlines()[-1].split()[1:])
    lines.append(f"# one AugmentedBatches step (batch 8, crop {CROP}, 32 resident frames, default arguments: paste=None; the host's draws and the pinned "
                 f"upload included) in fresh child processes, alternating, {n} steps per window, 5 windows each: median [min .. max] ms, the tuple's "
                 "length, the sum of the labels of the step after")
    for k, rows in res.items():
        for med, lo, hi, length, labels in rows:
            lines.append(f"{k} {float(med):9.4f} ms  [{float(lo):9.4f} .. {float(hi):9.4f}]  tuple of {length}  labels sum {labels}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=1569, help="synthetic frames in the bank's set (MFNet's training split holds 1 569)")
    ap.add_argument("--max-bytes", type=int, default=4 << 30, help="ObjectBank.build's limit for this set (its default, 1 GiB, is below what "
                    "1 569 synthetic frames bank: their rectangles are larger than a data set's objects)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--child-step", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_paste_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.child_step if a.child_step else ROOT)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/copy_paste_bench.py times kernels: it needs the MI355X")
    if a.child_step:
        return child_step(a.iters)
    lines = [f"# tools/copy_paste_bench.py: synthetic frames, {N_CLASS} classes, device events, {a.rounds} alternating rounds, {a.iters} calls per window "
             f"(a hundredth for the bank's stages), {torch.cuda.get_device_name(0)}", "#"]
    ds, bank = bank_build(a, lines)
    paste(a, lines, ds, bank)
    lines += registers()
    lines.append("#")
    against_parent(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
