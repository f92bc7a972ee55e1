#!/usr/bin/env python
"""What the object-level statistics cost on the device: utils/objects.object_stats (csrc/objects.hip) beside
utils/metrics.confusion_matrix and utils/metrics.boundary_stats on the same inputs, beside what a user does today on the host, at the
two extremes of the component count, and the pair forward of this tree next to the parent commit's.

    python tools/object_bench.py [--iters 50] [--rounds 5] [--parent-tree DIR] [--out profiles/object_bench.txt]

  1. the synthetic blocky label maps of tools/boundary_bench.py, 9 classes, 64 frames of 480 x 640 and 8 of 512 x 512, connectivity 8,
     the default size edges.  First the tables are compared for EQUALITY with the host's: both maps copied to the host,
     scipy.ndimage.label per class, numpy tables (timed once by the wall clock, copies included; skipped when scipy is missing).
     Then device-event times of warm calls, alternating the candidates inside each round; median [min .. max] over the rounds.  The
     component counts of the inputs are printed.  The inputs of the timed calls stay the same; where maps and workspace fit the
     256 MiB Infinity Cache (the 8 x 512 x 512 case: 25 MB of maps, 55 MB of workspace) the rate is a cache-warm one; the 64 frames
     (236 MB of maps, two chunks of up to 256 MiB of workspace under the default max_workspace_bytes) do not fit.
  2. the two extremes, 64 frames of 480 x 640 each: a constant frame (one component a frame) and a 1-pixel checkerboard under
     4-connectivity (every pixel its own component).
  3. with --parent-tree DIR (a built checkout of the parent commit): PairForward of this tree against the parent's with default
     arguments, each in fresh child processes of this one session, alternating - "off costs nothing".  Without it the section
     says so.
Nothing in the package is rerouted by this tool.
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
K = 9
SHAPES = [(64, 480, 640), (8, 512, 512)]


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


def host_tables(pred, label, conn, edges):
    """what a user does today: both maps to the host, scipy.ndimage.label per class, numpy tables -> obj, mass as object_stats'"""
    from scipy import ndimage as ndi
    p, l = pred.cpu().numpy().astype(np.int64), label.cpu().numpy()
    g = np.where((l >= 0) & (l < K), l, -1)
    p = np.where((g >= 0) & (p >= 0) & (p < K), p, -1)
    structure = np.ones((3, 3), dtype=int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    B, S = len(g), len(edges) + 1
    obj, mass = np.zeros((B, 2, K, S, 11), dtype=np.int64), np.zeros((B, 2, K, S, 2), dtype=np.int64)
    for b in range(B):
        for side, (m, other) in enumerate(((g[b], p[b]), (p[b], g[b]))):
            for c in range(K):
                lab, n = ndi.label(m == c, structure=structure)
                if not n:
                    continue
                area = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
                hit = np.bincount(lab[other == c], minlength=n + 1)[1:]
                s = np.searchsorted(np.asarray(edges, dtype=np.int64), area, side="right")
                np.add.at(obj[b, side, c], (s, (10 * hit) // area), 1)
                np.add.at(mass[b, side, c, :, 0], s, area)
                np.add.at(mass[b, side, c, :, 1], s, hit)
    return obj, mass


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


def kernels(a, lines):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from boundary_bench import blocky
    from segmif_amd import _lib
    from segmif_amd.utils import metrics, objects
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    for (B, H, W) in SHAPES:
        d, theta = metrics.boundary_widths(H, W)
        pred, label = (t.cuda() for t in blocky(B, H, W, d, seed=B))
        table = objects.object_stats(pred, label, K)
        n = table.obj.sum(dim=(0, 2, 3, 4)).tolist()
        small = table.obj[:, :, :, 0].sum(dim=(0, 2, 3)).tolist()
        ws = int(_lib.load().segmif_object_workspace_bytes(1, H, W))
        frames_per_chunk = max(1, min(B, (256 << 20) // ws))
        lines.append(f"# ({B}, {H}, {W}), blocks of side {3 * d}: maps {B * H * W * 12 / 1e6:.1f} MB, workspace {ws / 1e6:.1f} MB a frame, "
                     f"{frames_per_chunk} frames a chunk, {-(-B // frames_per_chunk) * 4} launches; {n[0]} components of the ground truth "
                     f"({small[0]} below 1024 pixels), {n[1]} of the prediction ({small[1]} below 1024 pixels); status {table.status.tolist()}")
        fits = B * H * W * 12 + frames_per_chunk * ws <= 256 << 20
        lines.append("# maps and workspace " + ("fit the 256 MiB Infinity Cache and the timed calls repeat on the same inputs: a cache-warm rate" if fits
                                                else "do not fit the 256 MiB Infinity Cache"))
        if have_scipy:
            t0 = time.perf_counter()
            obj_h, mass_h = host_tables(pred, label, 8, objects.DEFAULT_SIZE_EDGES)
            host_s = time.perf_counter() - t0
            if not (np.array_equal(table.obj.cpu().numpy(), obj_h) and np.array_equal(table.mass.cpu().numpy(), mass_h)):
                raise RuntimeError("object_stats and the host's scipy tables disagree")
            lines.append(f"host: copy + scipy.ndimage.label per class + numpy tables (equal tables)  {host_s * 1e3:11.1f} ms by the wall clock, once")
        else:
            lines.append("host: scipy is not installed: the tables were not compared and the host path was not timed")
        cand = {"object_stats    ": lambda: objects.object_stats(pred, label, K),
                "boundary_stats  ": lambda: metrics.boundary_stats(pred, label, K, d, theta),
                "confusion_matrix": lambda: metrics.confusion_matrix(pred, label, K)}
        res = alternating(cand, max(2, a.iters // (4 if B == 64 else 1)), a.rounds)
        med = sorted(res["object_stats    "])[a.rounds // 2]
        for k in cand:
            extra = f"  {B * H * W / med / 1e6:7.2f} G pixels/s, {B * H * W * 12 / med / 1e6:7.1f} GB/s of the maps" if k.startswith("object") else ""
            lines.append(f"{k} {spread(res[k])}{extra}")
        if have_scipy:
            lines.append(f"# the host path takes {host_s * 1e3 / med:.0f} x object_stats")
        del pred, label
    lines.append("#")
    B, H, W = 64, 480, 640
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for name, m, conn in (("constant frame, connectivity 8", torch.full((B, H, W), 3), 8),
                          ("1-pixel checkerboard, connectivity 4", ((yy + xx) % 2)[None].repeat(B, 1, 1), 4)):
        label = m.to(torch.int64).cuda().contiguous()
        pred = label.to(torch.int32)
        table = objects.object_stats(pred, label, K, conn)
        n = table.obj.sum(dim=(0, 2, 3, 4)).tolist()
        res = alternating({"object_stats": lambda: objects.object_stats(pred, label, K, conn)}, max(2, a.iters // 4), a.rounds)
        lines.append(f"# ({B}, {H}, {W}) {name}: {n[0]} components of the ground truth, {n[1]} of the prediction; status {table.status.tolist()}")
        lines.append(f"object_stats     {spread(res['object_stats'])}")
        del pred, label
    lines.append("#")


def registers():
    from segmif_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "objects.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return ["# registers: NOT recorded (the compile failed)"]
    out = ["# hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:"]
    for name in ("objects_local_kernel", "objects_border_kernel", "objects_count_kernel", "objects_tally_kernel"):
        block = r.stderr.split(name, 1)[-1]
        field = lambda f: (re.search(f + r": (\d+)", block) or [None, "?"])[1]
        scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
        out.append(f"#   {name}: {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, occupancy {occ} waves/SIMD, "
                   f"LDS {lds} bytes a workgroup")
    return out


def make_nets():
    from segmif_amd.core import Fusion_Network3_ac, Network3
    torch.manual_seed(0)
    return Network3("mit_b1", 9, pretrained=None).cuda().eval(), Fusion_Network3_ac().cuda().eval()


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
    n = max(3, a.iters // 10)
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--child-pair", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.child_pair if a.child_pair else ROOT)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/object_bench.py times kernels: it needs the MI355X")
    if a.child_pair:
        return child_pair(a.iters)
    lines = [f"# tools/object_bench.py: synthetic blocky label maps, {K} classes, {a.iters} calls per window (a quarter at 64 frames), "
             f"{a.rounds} alternating rounds, {torch.cuda.get_device_name(0)}", "#"]
    kernels(a, lines)
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
