#!/usr/bin/env python
"""What the region objectives cost: the kernels of csrc/region_objective.hip next to the same objectives composed from torch
operators on the device.

    python tools/region_objective_bench.py [--batch 8] [--iters 20] [--out profiles/region_objective_bench.txt]

  lovasz torch     Lovasz-Softmax with torch's kernels: softmax, per class |fg - p|, torch.sort over every valid pixel, the cumulative
                   sums of the sorted foreground flags, the dot product (classes present: a host-synchronising test per class)
  lovasz new       losses.RegionObjective("lovasz")
  dice   torch     soft Dice with torch's kernels: softmax, one_hot, three sums per class
  dice   new       losses.RegionObjective("dice")
NHWC logits (batch, 512, 512, 9) = randn * 2, labels uniform with 15 % ignored, as tools/seg_objective_bench.py has them.
Device-event times of warm calls through autograd (forward alone, and forward + backward), alternating the candidates inside each
round; the workspace the new kernels take is printed with them.  Nothing in the package is rerouted by this tool.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_objective_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/region_objective_bench.py times kernels: it needs the MI355X")
    from segmif_amd import _lib, losses
    B, H, W, C = a.batch, 512, 512, 9
    rows = B * H * W
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, H, W, C, generator=g) * 2).cuda().requires_grad_(True)
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.15] = 255
    y = y.cuda()
    new_lovasz, new_dice = losses.RegionObjective("lovasz"), losses.RegionObjective("dice")

    def valid_softmax():
        keep = y.view(-1) != 255
        return torch.softmax(x.view(-1, C)[keep], dim=1), y.view(-1)[keep]

    def torch_lovasz():
        p, yv = valid_softmax()
        terms = []
        for c in range(C):
            fg = (yv == c).float()
            if fg.sum() == 0:  # (classes present: a host synchronisation per class)
                continue
            e, perm = torch.sort((fg - p[:, c]).abs(), descending=True)
            fs = fg[perm]
            G = fs.sum()
            jac = 1.0 - (G - fs.cumsum(0)) / (G + (1.0 - fs).cumsum(0))
            jac[1:] = jac[1:] - jac[:-1]
            terms.append(torch.dot(e, jac))
        return torch.stack(terms).mean()

    def torch_dice():
        p, yv = valid_softmax()
        fg = torch.nn.functional.one_hot(yv, C).float()
        I, S, G = (p * fg).sum(0), p.sum(0), fg.sum(0)
        D = 1.0 - (2.0 * I + 1.0) / (S + G + 1.0)
        return D[G > 0].mean()

    cand = {"lovasz torch": torch_lovasz, "lovasz new  ": lambda: new_lovasz.forward_nhwc(x, y),
            "dice   torch": torch_dice, "dice   new  ": lambda: new_dice.forward_nhwc(x, y)}

    def both(fn):
        torch.autograd.grad(fn(), x)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in cand.values():  # warm
        for _ in range(3):
            both(fn)
    torch.cuda.synchronize()
    res = {k: ([], []) for k in cand}
    for _ in range(a.rounds):
        for k, fn in cand.items():
            res[k][0].append(timed(fn))
            res[k][1].append(timed(lambda: both(fn)))
    size = _lib.load().segmif_region_objective_workspace_bytes
    lines = [f"# tools/region_objective_bench.py: ({B}, {H}, {W}, {C}) float32 NHWC logits, {rows} pixels, {a.iters} calls per window, "
             f"{a.rounds} alternating rounds, {torch.cuda.get_device_name(0)}",
             f"# workspace of the new kernels: lovasz {size(rows, C, 0) / 2 ** 20:.1f} MiB, dice {size(rows, C, 1) / 2 ** 20:.2f} MiB "
             f"(the logits: {rows * C * 4 / 2 ** 20:.1f} MiB)",
             "# values: " + ", ".join(f"{' '.join(k.split())} {float(fn().detach()):.7f}" for k, fn in cand.items()),
             "# device-event ms per call through autograd: median [min .. max] over the rounds", "#"]
    for k in cand:
        for tag, ts in (("forward           ", sorted(res[k][0])), ("forward + backward", sorted(res[k][1]))):
            lines.append(f"{k} {tag}  {ts[len(ts) // 2]:8.4f} ms  [{ts[0]:8.4f} .. {ts[-1]:8.4f}]")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
