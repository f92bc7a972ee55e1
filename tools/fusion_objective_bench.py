#!/usr/bin/env python
"""What the table-driven fusion objective costs: the kernel pair of csrc/fusion_objective.hip (forward = the sums launch + the
fixed-order finish; backward = one launch) next to the dedicated Fusionloss3 pair it generalises.

    python tools/fusion_objective_bench.py [--batch 8] [--iters 200] [--out profiles/fusion_objective_bench.txt]

  sobel_l1   segmif_sobel_l1_f32 + segmif_sobel_l1_bwd_f32 (Fusionloss3's own kernels: the yardstick)
  table(2)   the new pair with the Fusionloss3 table: L1(mask, gen) + L1(S mask, S gen)
  table(6)   the new pair with Total_fusion_loss's six terms and a 3-channel mask
Device-event times of the library calls alone (buffers allocated once, coefficients fixed), warm, alternating the three
candidates inside each round; bytes = what each pass must read and write once (float32 planes).  Nothing in the package is
rerouted by this tool: Fusionloss3 keeps its kernels.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_objective_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/fusion_objective_bench.py times kernels: it needs the MI355X")
    from segmif_amd import _lib, autograd as ag, losses
    from segmif_amd.core import loss as core_loss
    lib = _lib.load()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    g = torch.Generator().manual_seed(0)
    r = lambda c: torch.rand(B, c, H, W, generator=g).cuda()
    gen, ir, vis, mask1, mask3 = r(1), r(1), r(1), r(1), (r(3) > 0.5).float()
    grad = torch.empty_like(gen)
    up = torch.ones(1, device="cuda")
    coef = torch.full((8,), 1.0 / n, device="cuda")
    pxy = torch.empty(2, n, device="cuda")
    part2 = torch.empty(2 * lib.segmif_loss_blocks(n), device="cuda", dtype=torch.float64)
    part8 = torch.empty(8 * lib.segmif_fusion_objective_blocks(B, H, W), device="cuda", dtype=torch.float64)
    sums = torch.empty(8, device="cuda", dtype=torch.float64)
    T = losses.ObjTerm
    d2 = ag.objective_descriptor((T("identity", "linear", a_mask=1.0), T("sobel", "linear", a_mask=1.0)), 1)
    d6 = ag.objective_descriptor(core_loss.Total_fusion_loss.TERMS, 3)
    p = lambda t: t.data_ptr()

    def chk(code):
        if code != 0:
            raise RuntimeError(f"library call failed with code {code}")

    cand = {
        "sobel_l1 ": (lambda: chk(lib.segmif_sobel_l1_f32(p(gen), p(mask1), p(pxy), p(part2), p(sums), B, H, W, None)),
                      lambda: chk(lib.segmif_sobel_l1_bwd_f32(p(pxy), p(gen), p(mask1), p(grad), B, H, W, p(up), None)),
                      (2 + 2) * 4 * n, (2 + 2 + 1) * 4 * n),   # forward writes the two sign planes, backward reads them
        "table(2) ": (lambda: chk(lib.segmif_fusion_objective_f32(ctypes.byref(d2), p(gen), None, None, p(mask1), 1, p(part8), p(sums), B, H, W, None)),
                      lambda: chk(lib.segmif_fusion_objective_bwd_f32(ctypes.byref(d2), p(gen), None, None, p(mask1), 1, p(coef), p(grad), B, H, W, None)),
                      2 * 4 * n, (2 + 1) * 4 * n),
        "table(6) ": (lambda: chk(lib.segmif_fusion_objective_f32(ctypes.byref(d6), p(gen), p(ir), p(vis), p(mask3), 3, p(part8), p(sums), B, H, W, None)),
                      lambda: chk(lib.segmif_fusion_objective_bwd_f32(ctypes.byref(d6), p(gen), p(ir), p(vis), p(mask3), 3, p(coef), p(grad), B, H, W, None)),
                      6 * 4 * n, (6 + 1) * 4 * n),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fwd, bwd, _, _ in cand.values():  # warm
        for _ in range(10):
            fwd(), bwd()
    torch.cuda.synchronize()
    res = {k: ([], []) for k in cand}
    for _ in range(a.rounds):
        for k, (fwd, bwd, _, _) in cand.items():
            res[k][0].append(timed(fwd))
            res[k][1].append(timed(bwd))
    lines = [f"# tools/fusion_objective_bench.py: ({B}, 1, {H}, {W}) float32, {a.iters} calls per window, {a.rounds} alternating rounds, "
             f"{torch.cuda.get_device_name(0)}",
             "# device-event ms per call: median [min .. max] over the rounds; GB/s = the bytes a pass must move once / median",
             "#"]
    for k, (_, _, fb, bb) in cand.items():
        for tag, ts, nbytes in (("forward ", sorted(res[k][0]), fb), ("backward", sorted(res[k][1]), bb)):
            med = ts[len(ts) // 2]
            lines.append(f"{k} {tag}  {med:7.4f} ms  [{ts[0]:7.4f} .. {ts[-1]:7.4f}]   {nbytes / 1e6:6.1f} MB  {nbytes / med / 1e6:7.0f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
