#!/usr/bin/env python
"""What the contour statistics cost on the device: utils/metrics.boundary_stats (csrc/boundary_stats.hip), the same tables
composed from torch operators, and utils/metrics.confusion_matrix on the same inputs for scale.

    python tools/boundary_bench.py [--iters 200] [--out profiles/boundary_bench.txt]

  kernel     hipEvent time of boundary_stats on synthetic blocky label maps at (64, 480, 640) with d = 16, theta = 6 and at
             (8, 512, 512) with d = 14, theta = 5 (boundary_widths of those frames), K = 9
  bytes      what the kernel's algorithm moves, counted from the shapes: every 64 x 64 tile reads its labels (8 B) and
             predictions (4 B) with a halo of max(d, theta + 1), clipped to the frame, columns rounded out to groups of 4; beside
             it the 12 B a pixel that a pass without halo would read.  The rate is those bytes over the kernel's time; the inputs
             of the timed calls stay the same and fit the Infinity Cache, so it is a cache-warm rate
  torch      the same tables from one-hot planes, max_pool2d for the erosions and dilations and masked sums, after its tables
             were compared with the kernel's for equality
  confusion  confusion_matrix (one pass over the two maps, no window)

Without a device the tool prints the counted bytes and the compiler's resource usage and says that nothing was measured; it
then leaves an existing output file alone.
"""
import argparse
import os
import re
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 9
SHAPES = [(64, 480, 640), (8, 512, 512)]


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


def blocky(B, H, W, d, seed):
    """label maps of blocks of side about 3 d, mostly background, with some ignored pixels; the prediction is the label moved by
    (2, 1) with a quarter of the blocks re-labelled"""
    g = torch.Generator().manual_seed(seed)
    side = 3 * d
    gh, gw = H // side + 2, W // side + 2
    grid = torch.where(torch.rand((B, gh, gw), generator=g) < 0.6, 0, torch.randint(0, K, (B, gh, gw), generator=g))
    regrid = torch.where(torch.rand((B, gh, gw), generator=g) < 0.25, torch.randint(0, K, (B, gh, gw), generator=g), grid)
    yy, xx = torch.arange(H + 2)[:, None] // side, torch.arange(W + 1)[None, :] // side
    label = grid[:, yy, xx][:, 2:, 1:].contiguous()
    pred = regrid[:, yy, xx][:, :H, :W].to(torch.int32).contiguous()
    label[:, : H // 8, : W // 8] = 255
    return pred, label


def torch_tables(pred, label, d, theta):
    """the rule of include/segmif_hip.h from torch operators -> (cls (B, K, 8), trimap (B, K, K)) int64"""
    B, H, W = label.shape
    valid = (label >= 0) & (label < K)
    g = torch.where(valid, label, K)
    p = torch.where(valid & (pred >= 0) & (pred < K), pred.long(), K)
    dtype = torch.float16 if label.is_cuda else torch.float32
    planes = lambda m: F.one_hot(m, K + 1).permute(0, 3, 1, 2)[:, :K].to(dtype)

    def band(M):  # mask - erosion; the frame is padded with "not the class"
        grown = F.max_pool2d(F.pad(1 - M, (d, d, d, d), value=1.0), 2 * d + 1, 1)
        return M * grown

    def contour(M):  # a pixel of the class with a pixel inside the frame that is not of it next to it
        return M * F.max_pool2d(1 - M, 3, 1, 1)

    near = (lambda C: F.max_pool2d(C, 2 * theta + 1, 1, theta)) if theta else (lambda C: C)
    G, P = planes(g), planes(p)
    GB, PB, GC, PC = band(G), band(P), contour(G), contour(P)
    count = lambda x: x.sum(dim=(2, 3), dtype=torch.float32).long()  # (exact below 2^24 pixels a frame)
    cls = torch.stack([count(GB), count(PB), count(GB * PB), count(GC), count(PC), count(GC * near(PC)), count(PC * near(GC)),
                       torch.zeros((B, K), dtype=torch.int64, device=label.device)], dim=2)
    in_band = (GB.sum(dim=1) > 0) & (p < K)
    frame = torch.arange(B, device=label.device)[:, None, None].expand(B, H, W)
    idx = (frame * K + g) * K + p
    tri = torch.bincount(idx[in_band], minlength=B * K * K).view(B, K, K)
    return cls, tri


def counted_bytes(B, H, W, d, theta, tile=64):
    R = max(d, theta + 1)
    total = 0
    for y0 in range(0, H, tile):
        rows = min(H, y0 + tile + R) - max(0, y0 - R)
        for x0 in range(0, W, tile):
            lo, hi = (x0 - R) // 4 * 4, -(-(x0 + tile + R) // 4) * 4  # the groups of 4 columns the tile loads
            cols = sum(1 for gx in range(lo, hi, 4) for e in range(4) if 0 <= gx + e < W and gx + 3 >= 0 and gx < W)
            total += rows * cols * 12
    return B * total, B * H * W * 12


def registers():
    from segmif_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "boundary_stats.hip"),
                                            "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return "registers: NOT recorded (the compile failed)"
    block = r.stderr.split("boundary_stats_kernel", 1)[-1]
    field = lambda name: (re.search(name + r": (\d+)", block) or [None, "?"])[1]
    scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
    return (f"registers: boundary_stats_kernel {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, "
            f"occupancy {occ} waves/SIMD, LDS {lds} bytes a workgroup of 512 threads (hipcc -O3 --offload-arch=gfx950 "
            "-Rpass-analysis=kernel-resource-usage)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.txt"))
    a = ap.parse_args()
    from segmif_amd.utils import metrics
    have = torch.cuda.is_available()
    lines = [f"# tools/boundary_bench.py: synthetic blocky label maps, {K} classes, "
             + (f"{torch.cuda.get_device_name(0)}; device events, {a.iters} calls a figure (torch: {max(3, a.iters // 40)}), warm" if have
                else "NO DEVICE: the times below are NOT measured"), "#"]
    for (B, H, W) in SHAPES:
        d, theta = metrics.boundary_widths(H, W)
        moved, least = counted_bytes(B, H, W, d, theta, metrics.BOUNDARY_TILE)
        lines.append(f"({B}, {H}, {W}), d = {d}, theta = {theta}: the kernel's loads {moved / 1e6:.1f} MB = {moved / least:.2f} x the "
                     f"{least / 1e6:.1f} MB of the two maps (12 B a pixel)")
        if not have:
            lines.append("  kernel, torch, confusion: not measured")
            continue
        pred, label = (t.cuda() for t in blocky(B, H, W, d, seed=B))
        got = metrics.boundary_stats(pred, label, K, d, theta)
        want = torch_tables(pred, label, d, theta)
        if not (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])):
            raise RuntimeError("boundary_stats and the torch composition disagree")
        tot = got[0].sum(dim=0)
        lines.append(f"  tables equal; band {int(tot[:, 0].sum())} of {int(((label >= 0) & (label < K)).sum())} valid pixels, "
                     f"{int(tot[:, 3].sum())} contour pixels")
        ms_k = timed(lambda: metrics.boundary_stats(pred, label, K, d, theta), a.iters)
        ms_t = timed(lambda: torch_tables(pred, label, d, theta), max(3, a.iters // 40), warm=1)
        ms_c = timed(lambda: metrics.confusion_matrix(pred, label, K), a.iters)
        lines.append(f"  kernel:    boundary_stats (two memsets, one launch, two allocations)   {ms_k:9.4f} ms   {moved / 1e6 / ms_k:7.1f} GB/s of its loads, "
                     f"{least / 1e6 / ms_k:7.1f} GB/s of the maps")
        lines.append(f"  torch:     one-hot planes, max_pool2d, masked sums (equal tables)      {ms_t:9.4f} ms   {ms_t / ms_k:6.1f} x the kernel")
        lines.append(f"  confusion: confusion_matrix on the same maps                           {ms_c:9.4f} ms   the kernel is {ms_k / ms_c:5.1f} x it")
    lines.append(registers())
    text = "\n".join(lines) + "\n"
    print(text)
    if have or not os.path.exists(a.out):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
