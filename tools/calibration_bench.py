#!/usr/bin/env python
"""What the calibration statistics cost: the kernel of csrc/calibration_stats.hip next to the same tables composed from torch
operators on the device and next to ops.pseudo_label on the same logits, the evaluate loop with and without calibration=, and
the pair forward of this tree next to the parent commit's.

    python tools/calibration_bench.py [--iters 20] [--rounds 5] [--parent-tree DIR] [--out profiles/calibration_bench.txt]

  1. (8, 128, 128, 9) -> 512 x 512 and (64, 120, 160, 9) -> 480 x 640 float32 NHWC logits = randn * 3, labels that agree with the
     argmax on 70 % of the pixels and are 255 on 5 %; 15 bins, threshold 0.968, NT = 1 and NT = 16 (DEFAULT_TEMPERATURES).
     utils/calibration.calibration_stats against ops.bilinear + softmax + max + bucketize + bincount per temperature, float32 on the
     device - the integer tables are compared first (they may differ on the pixels whose confidence falls on the other side of an
     edge in the other arithmetic: the share is printed), then device-event times of warm calls, alternating the candidates inside
     each round; median [min .. max] over the rounds.  The logits are 4.7 MB and 44 MB: every call reads them warm from the 256 MiB
     Infinity Cache.  The torch composition writes the resized logits (75 MB and 708 MB).
  2. Evaluator.update on batches of 8 frames of 480 x 640 (mit_b1, seeded weights), with labels, with and without calibration=
     (16 temperatures): device-event ms per batch, alternating.
  3. with --parent-tree DIR (a built checkout of the parent commit): PairForward of this tree against the parent's, each in fresh
     child processes of this one session, alternating - "off costs nothing".  Without it the section says so.
Nothing in the package is rerouted by this tool.  Nothing here measures the calibration of a trained model: the weights are seeded.
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return f"{ts[len(ts) // 2]:9.4f} ms  [{ts[0]:9.4f} .. {ts[-1]:9.4f}]"


def torch_tables(x, label, temperatures, edges, thresholds):
    """the same tables from torch operators: counts (NT, M, 3) with the confidence sum as float64, above (NT, NK, 2), sums (NT, 2)"""
    from segmif_amd import ops
    B, OH, OW = label.shape
    C = x.shape[3]
    v = ops.bilinear(x, OH, OW).reshape(-1, C)
    y = label.reshape(-1)
    valid = (y >= 0) & (y < C)
    v, y = v[valid], y[valid]
    correct = v.argmax(dim=1) == y
    M = edges.numel() + 1
    counts, above, sums = [], [], []
    for T in temperatures:
        logp = torch.log_softmax(v * float(np.float32(1) / np.float32(T)), dim=1)
        p = logp.exp()
        conf = p.max(dim=1).values
        b = torch.bucketize(conf, edges, right=True)
        counts.append(torch.stack([torch.bincount(b, minlength=M).double(), torch.bincount(b, weights=correct.double(), minlength=M),
                                   torch.bincount(b, weights=conf.double(), minlength=M)], dim=1))
        above.append(torch.stack([torch.stack([(conf > t).sum(), ((conf > t) & correct).sum()]) for t in thresholds]))
        sums.append(torch.stack([-logp.gather(1, y[:, None]).double().sum(),
                                 ((p - torch.nn.functional.one_hot(y, C)) ** 2).sum(dim=1).double().sum()]))
    return torch.stack(counts), torch.stack(above), torch.stack(sums)


def make_inputs(shape, size, seed=0):
    from segmif_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 3).cuda()
    pred = ops.bilinear_argmax(x, *size).long()
    u = torch.rand(pred.shape, generator=g).cuda()
    label = torch.where(u < 0.7, pred, torch.randint(0, shape[3], pred.shape, generator=g).cuda())
    label[u > 0.95] = 255
    return x, label.contiguous()


def kernels(a, lines):
    from segmif_amd import _lib, ops
    from segmif_amd.utils import calibration as cal
    edges = cal.uniform_edges(15)
    edges_t = torch.from_numpy(edges).cuda()
    thr = (0.968,)
    for shape, size in (((8, 128, 128, 9), (512, 512)), ((64, 120, 160, 9), (480, 640))):
        x, label = make_inputs(shape, size)
        pixels = label.numel()
        lines.append(f"# {shape} -> {size[0]} x {size[1]}: logits {x.numel() * 4 / 1e6:.1f} MB (cache-warm), labels {pixels * 8 / 1e6:.1f} MB, "
                     f"{pixels / 1e6:.2f} M pixels")
        for temps in ((1.0,), cal.DEFAULT_TEMPERATURES):
            NT = len(temps)
            table = cal.calibration_stats(x, label, temps, edges, thr)
            tc, ta, ts = torch_tables(x, label, temps, edges_t, thr)
            moved = float((table.counts[:, :, 0].double() - tc[:, :, 0]).abs().sum()) / 2 / (NT * float(table.totals[0]))
            rel = (table.sums - ts).abs() / ts.abs()
            conf_rel = float(((table.counts[:, :, 2].double() / 2.0 ** 32).sum(dim=1) - tc[:, :, 2].sum(dim=1)).abs().max() / tc[:, :, 2].sum(dim=1).max())
            lines.append(f"#   NT {NT}: against the torch composition: share of pixels in another bin {moved:.2e}, correct counts equal "
                         f"{bool((table.counts[:, :, 1].sum(dim=1).double() == tc[:, :, 1].sum(dim=1)).all())}, confidence sums differ by {conf_rel:.2e}, "
                         f"NLL sums by {float(rel[:, 0].max()):.2e}, Brier sums by {float(rel[:, 1].max()):.2e}; workspace "
                         f"{_lib.load().segmif_calibration_workspace_bytes(shape[0], size[0], size[1], NT) / 1e6:.2f} MB")
            cand = {"torch operators ": lambda: torch_tables(x, label, temps, edges_t, thr),
                    "calibration_stats": lambda: cal.calibration_stats(x, label, temps, edges, thr),
                    "pseudo_label     ": lambda: ops.pseudo_label(x, size[0], size[1])}
            for fn in cand.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            res = {k: [] for k in cand}
            iters = max(2, a.iters // (4 if shape[0] == 64 else 1))
            for _ in range(a.rounds):
                for k, fn in cand.items():
                    res[k].append(timed(fn, iters))
            for k in cand:
                med = sorted(res[k])[len(res[k]) // 2]
                extra = f"  {pixels * NT * shape[3] / med / 1e6:8.1f} G exponentials/s, {(x.numel() * 4 + pixels * 8) / med / 1e6:7.1f} GB/s of inputs" \
                    if k.startswith("calibration") else ""
                lines.append(f"NT {NT:2d} {k} {spread(res[k])}{extra}")
        del x, label
    lines.append("#")


def make_frames(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    ir = torch.randint(0, 256, (n, 480, 640), generator=g, dtype=torch.uint8).cuda()
    vis = torch.randint(0, 256, (n, 480, 640, 3), generator=g, dtype=torch.uint8).cuda()
    mask = torch.randint(0, 256, (n, 480, 640), generator=g, dtype=torch.uint8).cuda()
    label = torch.randint(0, 9, (n, 480, 640), generator=g).cuda()
    return ir, vis, mask, label


def make_nets():
    from segmif_amd.core import Fusion_Network3_ac, Network3
    torch.manual_seed(0)
    return Network3("mit_b1", 9, pretrained=None).cuda().eval(), Fusion_Network3_ac().cuda().eval()


def evaluate_loop(a, lines):
    from segmif_amd.evaluate import Evaluator
    seg, fus = make_nets()
    frames = make_frames(8)
    cand = {"Evaluator                 ": Evaluator(seg, fus), "Evaluator(calibration={}) ": Evaluator(seg, fus, calibration={})}
    for ev in cand.values():
        for _ in range(2):
            ev.update(*frames)
    torch.cuda.synchronize()
    res = {k: [] for k in cand}
    n = max(2, a.iters // 5)
    for _ in range(a.rounds):
        for k, ev in cand.items():
            res[k].append(timed(lambda: ev.update(*frames), n))
    lines.append(f"# Evaluator.update, mit_b1 on seeded weights, 8 frames of 480 x 640 with labels, eager, {n} batches per window; 16 temperatures, "
                 "15 bins; device-event ms per batch")
    for k in cand:
        lines.append(f"{k} {spread(res[k])}")
    lines.append("#")


def child_pair(iters):
    """this process's tree: median device-event ms of PairForward.eager, printed as the last line"""
    from segmif_amd.pipeline import PairForward
    seg, fus = make_nets()
    g = torch.Generator().manual_seed(2)
    ir, vis = torch.rand(8, 1, 480, 640, generator=g).cuda(), torch.rand(8, 3, 480, 640, generator=g).cuda()
    mask3 = torch.rand(8, 1, 480, 640, generator=g).cuda().repeat(1, 3, 1, 1)
    pair = PairForward(seg, fus)
    with torch.no_grad():
        for _ in range(3):
            out = pair.eager(ir, vis, mask3)
        torch.cuda.synchronize()
        ts = sorted(timed(lambda: pair.eager(ir, vis, mask3), iters) for _ in range(5))
    print(f"PAIR {ts[2]:.4f} {ts[0]:.4f} {ts[-1]:.4f} {len(out)} {int(out[1].sum())}")


def against_parent(a, lines):
    if not a.parent_tree:
        lines.append("# PairForward of this tree against the parent commit: not measured (no --parent-tree)")
        return
    n = max(3, a.iters // 4)
    res = {"this tree": [], "parent   ": []}
    for _ in range(2):
        for k, tree in (("this tree", ROOT), ("parent   ", os.path.abspath(a.parent_tree))):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child-pair", tree, "--iters", str(n)],
                               cwd=tree, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"the child on {tree} ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            res[k].append(r.stdout.strip().splitlines()[-1].split()[1:])
    lines.append(f"# PairForward.eager (mit_b1, 8 pairs of 480 x 640, default arguments) in fresh child processes, alternating, {n} calls per window, "
                 "5 windows each: median [min .. max] ms, the tuple's length, the sum of the labels")
    for k, rows in res.items():
        for med, lo, hi, length, labels in rows:
            lines.append(f"{k} {float(med):9.4f} ms  [{float(lo):9.4f} .. {float(hi):9.4f}]  tuple of {length}  labels sum {labels}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--child-pair", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.child_pair if a.child_pair else ROOT)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/calibration_bench.py times kernels: it needs the MI355X")
    if a.child_pair:
        return child_pair(a.iters)
    lines = [f"# tools/calibration_bench.py: {a.iters} calls per window, {a.rounds} alternating rounds, {torch.cuda.get_device_name(0)}", "#"]
    kernels(a, lines)
    evaluate_loop(a, lines)
    against_parent(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
