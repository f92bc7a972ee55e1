#!/usr/bin/env python
"""What self-training costs on the device: ops.pseudo_label against the same result from ops.bilinear and torch operators, the
weighted segmentation objective against the unweighted one, and the whole self-training step against seg_train_step.

    python tools/self_training_bench.py [--iters 200] [--step-iters 10] [--parent-tree DIR] [--out profiles/self_training_bench.txt]

  pseudo    device-event time of ops.pseudo_label (labels, count and conf) at (8, 128, 128, 9) -> 512 x 512 and
            (64, 120, 160, 9) -> 480 x 640, and of the composition ops.bilinear + softmax + max + compare + sum that writes and
            re-reads the resized logits, after the two were compared.  The bytes are the algorithm's: the source logits once, 8 B of
            label and 4 B of confidence per output pixel.  The source logits fit the Infinity Cache and every timed call reads the
            same buffers, so the rate is a cache-warm one.
  weighted  ag.seg_objective at (8, 512, 512, 9), forward and forward + backward, without weights, with a pixel weight and with a
            sample weight.  --parent-tree DIR (a checkout of the parent commit with its library built) adds the unweighted figure of
            that tree, taken by a fresh child process in the same session: what the "off" case costs.
  step      SelfTrainingStep (one teacher forward, two student forwards and backwards, one optimizer step, refresh) against
            seg_train_step at batch 8, crop 512, mit_b3, eval-mode regime, synthetic inputs; and the share of the step that is the
            teacher's weight repack after refresh() (a teacher forward right after refresh() against one with warm caches).

The kernel's registers come from the compiler's resource usage (a compile of csrc/pseudo_label.hip; no device needed).  The inputs
are synthetic: the numbers say what the passes cost.  NOTHING here was measured about mIoU.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, n, warm=10):
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


def kernel_registers():
    from segmif_amd import build
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "pseudo_label.hip"),
                                            "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return "registers: NOT recorded (the compile failed)"
    block = r.stderr.split("pseudo_label_kernel", 1)[-1]
    field = lambda name: (re.search(name + r": (\d+)", block) or [None, "?"])[1]
    scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
    return (f"registers: pseudo_label_kernel {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, "
            f"occupancy {occ} waves/SIMD, LDS {lds} bytes (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")


def objective_inputs():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(8, 512, 512, 9, generator=g) * 2).cuda()
    y = torch.randint(0, 9, (8, 512, 512), generator=g)
    y[torch.rand(8, 512, 512, generator=g) < 0.1] = 255
    return x, y.cuda()


def time_objective(ag, x, y, iters, **kw):
    """(forward ms, forward + backward ms) of ag.seg_objective(reduction="mean_all")"""
    xg = x.detach().requires_grad_(True)

    def both():
        xg.grad = None
        ag.seg_objective(xg, y, reduction="mean_all", **kw).backward()

    return timed(lambda: ag.seg_objective(x, y, reduction="mean_all", **kw), iters), timed(both, iters)


def unweighted_only(iters):
    """the child of --parent-tree: prints one JSON line"""
    from segmif_amd import autograd as ag
    x, y = objective_inputs()
    f, fb = time_objective(ag, x, y, iters)
    print(json.dumps({"fwd_ms": f, "fwd_bwd_ms": fb}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: its unweighted objective is timed too")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--unweighted-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--skip-step", action="store_true", help="leave the whole-step section out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_training_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if not torch.cuda.is_available():
        raise RuntimeError("self_training_bench measures on the MI355X: no device, no numbers")
    if a.unweighted_only:
        return unweighted_only(a.iters)
    from segmif_amd import autograd as ag, ops
    lines = [f"# tools/self_training_bench.py: synthetic inputs, {torch.cuda.get_device_name(0)}; device events, {a.iters} calls a figure "
             f"({a.step_iters} for the steps), warm", "#"]
    # ---- pseudo_label ------------------------------------------------------------------------------------------------------------
    for (B, h, w, C), (OH, OW) in (((8, 128, 128, 9), (512, 512)), ((64, 120, 160, 9), (480, 640))):
        x = (torch.randn(B, h, w, C, generator=torch.Generator().manual_seed(1)) * 8).cuda()
        tau = 0.968

        def composed():
            p = torch.softmax(ops.bilinear(x, OH, OW), dim=-1).max(-1)
            return p.indices, (p.values > tau).flatten(1).sum(1), p.values

        lab, cnt, conf = ops.pseudo_label(x, OH, OW, tau=tau, return_conf=True)
        lab_t, cnt_t, conf_t = composed()
        differ = int((lab != lab_t).sum())
        if differ > lab.numel() // 10000 or int((cnt - cnt_t).abs().max()) > lab[0].numel() // 10000 or float((conf - conf_t).abs().max()) > 1e-5:
            raise RuntimeError("ops.pseudo_label and the torch composition disagree")
        ms = timed(lambda: ops.pseudo_label(x, OH, OW, tau=tau, return_conf=True), a.iters)
        ms_nc = timed(lambda: ops.pseudo_label(x, OH, OW, tau=tau), a.iters)
        ms_t = timed(composed, max(10, a.iters // 4))
        px = B * OH * OW
        nbytes, nbytes_nc = 4 * x.numel() + 12 * px, 4 * x.numel() + 8 * px
        lines.append(f"pseudo_label ({B}, {h}, {w}, {C}) -> {OH} x {OW}: confident share {float(cnt.sum()) / px:.3f}; labels differing from the "
                     f"composition {differ} of {px}")
        lines.append(f"  kernel, labels + count + conf: {nbytes / 1e6:7.1f} MB  {ms:8.4f} ms  {nbytes / 1e6 / ms:7.1f} GB/s (cache-warm: the source "
                     f"logits, {4 * x.numel() / 1e6:.1f} MB, fit the Infinity Cache)")
        lines.append(f"  kernel, labels + count:        {nbytes_nc / 1e6:7.1f} MB  {ms_nc:8.4f} ms  {nbytes_nc / 1e6 / ms_nc:7.1f} GB/s")
        lines.append(f"  ops.bilinear + softmax + max + compare + sum (writes and re-reads {4 * px * C / 1e6:.0f} MB of resized logits)  {ms_t:8.4f} ms  "
                     f"= {ms_t / ms:.1f} x the kernel")
        del x, lab, cnt, conf, lab_t, cnt_t, conf_t
    lines.append(kernel_registers())
    # ---- the weighted objective --------------------------------------------------------------------------------------------------
    x, y = objective_inputs()
    u = torch.rand(8, 512, 512, device="cuda") * 2
    q = torch.rand(8, device="cuda")
    lines.append("seg_objective (8, 512, 512, 9), reduction mean_all: forward / forward + backward")
    for name, kw in (("no weights (the path as it was)", {}), ("pixel_weight", dict(pixel_weight=u)), ("sample_weight", dict(sample_weight=q)),
                     ("both", dict(pixel_weight=u, sample_weight=q))):
        f, fb = time_objective(ag, x, y, a.iters, **kw)
        lines.append(f"  {name:34s} {f:8.4f} ms / {fb:8.4f} ms")
    if a.parent_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--unweighted-only", "--tree", a.parent_tree, "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            lines.append("  parent commit, no weights: NOT recorded (the child failed: " + r.stderr.strip().splitlines()[-1][:200] + ")")
        else:
            p = json.loads(r.stdout.strip().splitlines()[-1])
            lines.append(f"  {'parent commit, no weights (child)':34s} {p['fwd_ms']:8.4f} ms / {p['fwd_bwd_ms']:8.4f} ms")
    else:
        lines.append("  parent commit, no weights: NOT recorded (no --parent-tree)")
    del x, y, u, q
    # ---- the whole step ----------------------------------------------------------------------------------------------------------
    if not a.skip_step:
        import segmif_amd.core as core
        from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
        from segmif_amd.train import make_seg_optimizer, seg_train_step
        B, crop = 8, 512
        torch.manual_seed(0)
        net = core.Network3("mit_b3", 9, pretrained=None).cuda().eval()
        opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.999)
        g = torch.Generator().manual_seed(2)
        xL, xU = torch.rand(B, 3, crop, crop, generator=g).cuda(), torch.rand(B, 3, crop, crop, generator=g).cuda()
        yL = torch.randint(0, 9, (B, crop, crop), generator=g).cuda()
        crit = torch.nn.CrossEntropyLoss(ignore_index=255)
        ms_seg = timed(lambda: seg_train_step(net, opt, xL, yL, crit), a.step_iters, warm=3)
        teacher = EmaTeacher(opt, net)
        step = SelfTrainingStep(net, teacher, opt, crit, tau=0.2)
        ms_st = timed(lambda: step.step(xL, yL, xU), a.step_iters, warm=3)
        share = step.confident_share()

        def teacher_cold():
            teacher.refresh()
            teacher.logits(xU)

        ms_cold = timed(teacher_cold, a.step_iters, warm=2)
        ms_warm = timed(lambda: teacher.logits(xU), a.step_iters, warm=2)
        lines.append(f"step, mit_b3, batch {B}, crop {crop}, eval-mode regime (tau 0.2 on random weights: confident share {share:.3f}):")
        lines.append(f"  seg_train_step                         {ms_seg:9.3f} ms")
        lines.append(f"  SelfTrainingStep.step                  {ms_st:9.3f} ms  = {ms_st / ms_seg:.2f} x seg_train_step")
        lines.append(f"  teacher forward after refresh()        {ms_cold:9.3f} ms")
        lines.append(f"  teacher forward, caches warm           {ms_warm:9.3f} ms  -> the repack after refresh() is {ms_cold - ms_warm:.3f} ms, "
                     f"{100 * (ms_cold - ms_warm) / ms_st:.1f} % of the step")
    lines.append("note: synthetic inputs and random weights; nothing here was measured about mIoU")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
