#!/usr/bin/env python
"""What distillation costs: the kernels of csrc/distill_objective.hip next to the same objectives composed from torch operators on
the device, the distillation step next to the plain segmentation step, and the plain step of this tree next to the parent commit's.

    python tools/distill_bench.py [--iters 20] [--rounds 5] [--parent-tree DIR] [--out profiles/distill_bench.txt]

  1. both modes at (8, 128, 128, 9) and (64, 120, 160, 9) float32 NHWC logits = randn * 3: losses.DistillObjective against softmax,
     log-softmax, multiply and sum in float32 on the device - compared for equality of results first (value and gradient, relative to
     the value and to the gradient's largest element), then device-event times of warm calls through autograd, forward alone and
     forward + backward, alternating the candidates inside each round; median [min .. max] over the rounds.  The logits are 4.7 MB
     and 44 MB per tensor: every one of these calls reads them warm from the 256 MiB Infinity Cache, which a training step's does not.
  2. distill.DistillStep (student mit_b1, teacher mit_b3, channel mode) against train.seg_train_step on the same student: batch 8,
     crop 512, random frames and labels, both eager; device-event ms per step, alternating.
  3. with --parent-tree DIR (a built checkout of the parent commit): seg_train_step of this tree against the parent's, each in fresh
     child processes of this one session, alternating - "off costs nothing".  Without it the section says so.
Nothing in the package is rerouted by this tool.
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_objective(kind, s, t, T):
    """the objective from torch operators, in the inputs' dtype"""
    B, h, w, C = s.shape
    if kind == "pixel":
        zs, zt = s.reshape(-1, C) / T, t.reshape(-1, C) / T
    else:
        zs, zt = (x.reshape(B, h * w, C).transpose(1, 2).reshape(B * C, h * w) / T for x in (s, t))
    k = (torch.softmax(zt, dim=1) * (torch.log_softmax(zt, dim=1) - torch.log_softmax(zs, dim=1))).sum()
    return T * T * k / zs.shape[0]


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


def objectives(a, lines):
    from segmif_amd import _lib, losses
    size = _lib.load().segmif_distill_workspace_bytes
    for shape in ((8, 128, 128, 9), (64, 120, 160, 9)):
        B, h, w, C = shape
        g = torch.Generator().manual_seed(0)
        s = (torch.randn(shape, generator=g) * 3).cuda().requires_grad_(True)
        t = (torch.randn(shape, generator=g) * 3).cuda()
        lines.append(f"# {shape}: {s.numel() * 4 / 1e6:.1f} MB per tensor, cache-warm")
        for kind in ("channel", "pixel"):
            obj = losses.DistillObjective(kind)
            T = obj.temperature
            cand = {"torch": lambda: torch_objective(kind, s, t, T), "new  ": lambda: obj.forward_nhwc(s, t)}
            v = {k: fn() for k, fn in cand.items()}
            gr = {k: torch.autograd.grad(v[k], s)[0] for k in cand}
            ref_v = float(torch_objective(kind, s.detach().double(), t.double(), T))
            sd = s.detach().double().requires_grad_(True)
            ref_g = torch.autograd.grad(torch_objective(kind, sd, t.double(), T), sd)[0]
            gmax = float(ref_g.abs().max())
            lines.append(f"#   {kind} T {T}: float64 value {ref_v:.9f}; " + "; ".join(
                f"{k.strip()} value error {abs(float(v[k].detach()) - ref_v) / abs(ref_v):.2e} gradient error "
                f"{float((gr[k].double() - ref_g).abs().max()) / gmax:.2e}" for k in cand)
                + f"; workspace {size(B * h * w, h * w, C, 1 if kind == 'channel' else 0) / 1024:.1f} KiB")
            for fn in cand.values():
                for _ in range(3):
                    torch.autograd.grad(fn(), s)
            torch.cuda.synchronize()
            res = {k: ([], []) for k in cand}
            for _ in range(a.rounds):
                for k, fn in cand.items():
                    res[k][0].append(timed(fn, a.iters))
                    res[k][1].append(timed(lambda: torch.autograd.grad(fn(), s), a.iters))
            for k in cand:
                lines.append(f"{kind:7s} {k} forward            {spread(res[k][0])}")
                lines.append(f"{kind:7s} {k} forward + backward {spread(res[k][1])}")
        del s, t
    lines.append("#")


def make_step_inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 3, 512, 512, generator=g).cuda()
    y = torch.randint(0, 9, (8, 512, 512), generator=g)
    y[torch.rand(8, 512, 512, generator=g) < 0.1] = 255
    return x, y.cuda()


def steps(a, lines):
    from segmif_amd import losses
    from segmif_amd.core import Network3
    from segmif_amd.distill import DistillStep, FrozenTeacher
    from segmif_amd.train import make_seg_optimizer, seg_train_step
    torch.manual_seed(0)
    student = Network3("mit_b1", 9, pretrained=None).cuda().train()
    teacher = FrozenTeacher(Network3("mit_b3", 9, pretrained=None).cuda())
    x, y = make_step_inputs()
    crit, opt = torch.nn.CrossEntropyLoss(ignore_index=255), make_seg_optimizer(student)
    kd = DistillStep(student, teacher, opt, crit, losses.DistillObjective("channel"))
    cand = {"seg_train_step       ": lambda: seg_train_step(student, opt, x, y, crit), "DistillStep (channel)": lambda: kd.step(x, y),
            "teacher.logits alone ": lambda: teacher.logits(x)}
    for fn in cand.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in cand}
    n = max(3, a.iters // 4)
    for _ in range(a.rounds):
        for k, fn in cand.items():
            res[k].append(timed(fn, n))
    lines.append(f"# student mit_b1, teacher mit_b3, batch 8, crop 512, eager, {n} steps per window; device-event ms per step")
    for k in cand:
        lines.append(f"{k} {spread(res[k])}")
    lines.append("#")


def child_step(iters):
    """this process's tree: median device-event ms of seg_train_step, printed as the last line"""
    from segmif_amd.core import Network3
    from segmif_amd.train import make_seg_optimizer, seg_train_step
    torch.manual_seed(0)
    net = Network3("mit_b1", 9, pretrained=None).cuda().train()
    x, y = make_step_inputs()
    crit, opt = torch.nn.CrossEntropyLoss(ignore_index=255), make_seg_optimizer(net)
    for _ in range(3):
        loss = seg_train_step(net, opt, x, y, crit)
    torch.cuda.synchronize()
    ts = sorted(timed(lambda: seg_train_step(net, opt, x, y, crit), iters) for _ in range(5))
    print(f"STEP {ts[2]:.4f} {ts[0]:.4f} {ts[-1]:.4f} {float(loss):.9f}")


def against_parent(a, lines):
    if not a.parent_tree:
        lines.append("# seg_train_step of this tree against the parent commit: not measured (no --parent-tree)")
        return
    n = max(3, a.iters // 4)
    res = {"this tree": [], "parent   ": []}
    for _ in range(2):
        for k, tree in (("this tree", ROOT), ("parent   ", os.path.abspath(a.parent_tree))):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child-step", tree, "--iters", str(n)],
                               cwd=tree, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"the child on {tree} ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            res[k].append(r.stdout.strip().splitlines()[-1].split()[1:])
    lines.append(f"# seg_train_step (mit_b1, batch 8, crop 512) in fresh child processes, alternating, {n} steps per window, 5 windows each: "
                 "median [min .. max] ms, the third step's loss")
    for k, rows in res.items():
        for med, lo, hi, loss in rows:
            lines.append(f"{k} {float(med):9.4f} ms  [{float(lo):9.4f} .. {float(hi):9.4f}]  loss {loss}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--child-step", metavar="TREE", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.child_step if a.child_step else ROOT)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/distill_bench.py times kernels: it needs the MI355X")
    if a.child_step:
        return child_step(a.iters)
    lines = [f"# tools/distill_bench.py: {a.iters} calls per window, {a.rounds} alternating rounds, {torch.cuda.get_device_name(0)}", "#"]
    objectives(a, lines)
    steps(a, lines)
    against_parent(a, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
