#!/usr/bin/env python
"""What the segmentation objectives cost: the kernel pair of csrc/seg_objective.hip next to what a caller had before it.

    python tools/seg_objective_bench.py [--batch 8] [--iters 50] [--out profiles/seg_objective_bench.txt]

  ce    softmax_ce   the node the default criterion runs on: segmif_softmax_ce_f32 (keeps an unnormalised gradient), the fp64
                     partial sum and the aten multiply of its backward
  ce    new pair     losses.SegObjective() - the same objective on the new kernels
  ohem  torch        the reference's OhemCELoss.forward on the device with torch's kernels: CE(reduction='none'), torch.sort over
                     every pixel, the host-synchronising branch
  ohem  new pair     core.OhemCELoss(0.7, rows // 16)
  focal torch        the reference's SoftmaxFocalLoss.forward with torch's kernels
  focal new pair     core.SoftmaxFocalLoss(2.0)
NHWC logits (batch, 512, 512, 9) = randn * 2, labels uniform with 15 % ignored; the torch formulations get the channels-last NCHW
view a caller's criterion receives from seg_criterion_loss.  Device-event times of warm calls through autograd (forward alone,
and forward + backward), alternating the candidates inside each round.  Nothing in the package is rerouted by this tool.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_objective_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/seg_objective_bench.py times kernels: it needs the MI355X")
    from segmif_amd import autograd as ag, losses, ops
    from segmif_amd.core import loss as core_loss
    B, H, W, C = a.batch, 512, 512, 9
    rows = B * H * W
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, H, W, C, generator=g) * 2).cuda().requires_grad_(True)
    y = torch.randint(0, C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.15] = 255
    y = y.cuda()
    n_min = rows // 16
    t = -torch.log(torch.tensor(0.7, dtype=torch.float)).cuda()
    new_ce, new_ohem, new_focal = losses.SegObjective().cuda(), core_loss.OhemCELoss(0.7, n_min).cuda(), core_loss.SoftmaxFocalLoss(2.0).cuda()

    def torch_ohem():
        loss = F.cross_entropy(ops.as_nchw(x), y, ignore_index=255, reduction="none").view(-1)
        loss, _ = torch.sort(loss, descending=True)
        if loss[n_min - 1] > t:  # (the reference's host synchronisation)
            return loss[loss > t].mean()
        return loss[:n_min].mean()

    def torch_focal():
        xn = ops.as_nchw(x)
        return F.nll_loss(torch.pow(1.0 - F.softmax(xn, dim=1), 2.0) * F.log_softmax(xn, dim=1), y, ignore_index=255)

    cand = {"ce    softmax_ce": lambda: ag.softmax_ce(x, y, 255), "ce    new pair  ": lambda: new_ce.forward_nhwc(x, y),
            "ohem  torch     ": torch_ohem, "ohem  new pair  ": lambda: new_ohem.forward_nhwc(x, y),
            "focal torch     ": torch_focal, "focal new pair  ": lambda: new_focal.forward_nhwc(x, y)}

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
    lines = [f"# tools/seg_objective_bench.py: ({B}, {H}, {W}, {C}) float32 NHWC logits, {rows} pixels, OHEM n_min {n_min}, {a.iters} calls per "
             f"window, {a.rounds} alternating rounds, {torch.cuda.get_device_name(0)}",
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
