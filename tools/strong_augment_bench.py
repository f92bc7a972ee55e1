#!/usr/bin/env python
"""What the strong augmentation of self-training costs on the device: ops.strong_augment against the same result composed from
torch operators, and the whole self-training step with and without it.

    python tools/strong_augment_bench.py [--iters 200] [--step-iters 10] [--repeats 3] [--parent-tree DIR] [--out profiles/strong_augment_bench.txt]

  kernels   device-event time of ops.strong_augment (both launches, the table already on the device) at (8, 3, 512, 512) and
            (64, 3, 480, 640) for four tables - every sample a copy, jitter only, blur only at radius 5, both - and of the same
            result from torch operators in float32 on the device (clamp, sums, where, floor, two conv2d over a reflect-padded
            batch), after the two were compared.  The bytes are the algorithm's: x twice (the mean pass and the apply pass; once
            where no sample is jittered) plus y.  A batch (25 MB and 236 MB) fits the 256 MiB Infinity Cache beside its output only
            in the small case, and every timed call reads the same buffers: the rates are cache-warm ones, not HBM rates.
  step      SelfTrainingStep at batch 8, crop 512, mit_b3, eval-mode regime, synthetic inputs, with the cross-set mix: without a
            policy, and with StrongAugment(jitter_prob=1, blur_prob=1) so that every sample pays for both operations; --repeats
            alternating runs of each, the spread printed.  --parent-tree DIR (a checkout of the parent commit with its library built) adds
            that tree's step, timed by fresh child processes in the same session, alternating with this tree's: "off costs nothing"
            is judged against it, within the spread.

The kernels' registers come from the compiler's resource usage (a compile of csrc/strong_augment.hip; no device needed).  The
inputs are synthetic: the numbers say what the passes cost.  NOTHING here was measured about mIoU.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
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
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "strong_augment.hip"),
                                            "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return ["registers: NOT recorded (the compile failed)"]
    out = []
    for kernel in ("strong_mean_kernel", "strong_apply_kernel"):
        block = r.stderr.split(kernel, 1)[-1]
        field = lambda name: (re.search(name + r": (\d+)", block) or [None, "?"])[1]
        scratch, occ, lds = field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]"), field(r"LDS Size \[bytes/block\]")
        out.append(f"registers: {kernel} {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, scratch {scratch} bytes/lane, occupancy {occ} "
                   f"waves/SIMD, LDS {lds} bytes")
    return out + ["  (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)"]


def torch_composition(x, t):
    """the rule from torch operators, float32 on the device; t: the host table"""
    dev = x.device
    col = lambda name: torch.from_numpy(np.ascontiguousarray(t[name])).to(dev)[:, None, None, None]
    on = col("jitter_on") != 0
    fb, fc, fs, fh = col("fb"), col("fc"), col("fs"), col("fh")
    luma = lambda v: (0.299 * v[:, 0:1] + 0.587 * v[:, 1:2]) + 0.114 * v[:, 2:3]
    v = (fb * x).clamp(0, 1)
    m = luma(v).double().mean(dim=(1, 2, 3), keepdim=True).float()
    v = (fc * v + (1 - fc) * m).clamp(0, 1)
    v = (fs * v + (1 - fs) * luma(v)).clamp(0, 1)
    r, g, b = v[:, 0], v[:, 1], v[:, 2]
    mx, mn = v.amax(1), v.amin(1)
    eq, cr = mx == mn, mx - mn
    one = torch.ones_like(mx)
    s, d = cr / torch.where(eq, one, mx), torch.where(eq, one, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    h = torch.where(mx == r, bc - gc, torch.where(mx == g, 2 + rc - bc, 4 + gc - rc))
    h = h / 6 + 1
    h = h - h.floor() + fh[:, 0]
    h = h - h.floor()
    h6 = 6 * h
    fl = h6.floor()
    f, i = h6 - fl, fl.long() % 6
    p, q, u = (mx * (1 - s)).clamp(0, 1), (mx * (1 - s * f)).clamp(0, 1), (mx * (1 - s * (1 - f))).clamp(0, 1)
    pick = lambda *c: torch.stack(c, 0).gather(0, i[None])[0]
    v = torch.stack([pick(mx, q, p, p, u, mx), pick(u, mx, mx, q, p, p), pick(p, p, u, mx, mx, q)], 1)
    v = torch.where(on, v, x)
    mean = torch.where(on[:, 0, 0, 0], m[:, 0, 0, 0], torch.zeros_like(m[:, 0, 0, 0]))
    R = int(t["radius"].max())
    if R > 0:  # (every sample through the widest kernel: a sample's own taps past its radius are zero, a copy has the tap 1)
        B, _, hh, ww = x.shape
        taps = torch.from_numpy(np.ascontiguousarray(t["taps"][:, :R + 1])).to(dev)
        full = torch.cat([taps.flip(1)[:, :-1], taps], 1)  # (B, 2R + 1)
        w3 = full.repeat_interleave(3, 0)
        pad = torch.nn.functional.pad(v.reshape(1, 3 * B, hh, ww), (R, R, R, R), mode="reflect")
        rows = torch.nn.functional.conv2d(pad, w3[:, None, None, :], groups=3 * B)
        v = torch.nn.functional.conv2d(rows, w3[:, None, :, None], groups=3 * B).reshape(B, 3, hh, ww)
    return v, mean


def tables(ops, B):
    t = {k: np.zeros(B, dtype=ops.strong_rec_dtype()) for k in ("copy", "jitter only", "blur only, radius 5", "both")}
    rng = np.random.RandomState(0)
    radius, taps = ops.strong_taps(1.15)
    assert radius == 5
    for name, tab in t.items():
        jit, blur = name in ("jitter only", "both"), name in ("blur only, radius 5", "both")
        tab["jitter_on"] = int(jit)
        for f, lo, hi in (("fb", 0.8, 1.2), ("fc", 0.8, 1.2), ("fs", 0.8, 1.2), ("fh", -0.2, 0.2)):
            tab[f] = rng.uniform(lo, hi, B) if jit else (0.0 if f == "fh" else 1.0)
        tab["radius"] = radius if blur else 0
        tab["taps"] = taps if blur else [1.0] + [0.0] * 8
    return t


def step_ms(step_iters, strong, tree_is_parent=False):
    """one timing of SelfTrainingStep.step from a fresh net (ms); strong: time it with the all-on policy"""
    import segmif_amd.core as core
    from segmif_amd.data import ClassMix
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
    from segmif_amd.train import make_seg_optimizer
    B, crop = 8, 512
    torch.manual_seed(0)
    net = core.Network3("mit_b3", 9, pretrained=None).cuda().eval()
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.999)
    g = torch.Generator().manual_seed(2)
    xL, xU = torch.rand(B, 3, crop, crop, generator=g).cuda(), torch.rand(B, 3, crop, crop, generator=g).cuda()
    yL = torch.randint(0, 9, (B, crop, crop), generator=g).cuda()
    kw = {}
    if strong:
        from segmif_amd.data import StrongAugment
        kw["strong"] = StrongAugment(jitter_prob=1.0, blur_prob=1.0, seed=0)
    step = SelfTrainingStep(net, EmaTeacher(opt, net), opt, torch.nn.CrossEntropyLoss(ignore_index=255), tau=0.2, mix=ClassMix(prob=1.0, seed=0), **kw)
    return timed(lambda: step.step(xL, yL, xU), step_iters, warm=3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: its step is timed too")
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--step-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--skip-step", action="store_true", help="leave the whole-step section out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strong_augment_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if not torch.cuda.is_available():
        raise RuntimeError("strong_augment_bench measures on the MI355X: no device, no numbers")
    if a.step_only:  # the child of the step section: one JSON line
        print(json.dumps({"ms": step_ms(a.step_iters, strong=False)}))
        return
    from segmif_amd import ops
    lines = [f"# tools/strong_augment_bench.py: synthetic inputs, {torch.cuda.get_device_name(0)}; device events, {a.iters} calls a figure "
             f"({a.step_iters} for the steps), warm", "#"]
    # ---- the kernels ---------------------------------------------------------------------------------------------------------------
    for B, h, w in ((8, 512, 512), (64, 480, 640)):
        x = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(1)).cuda()
        nbytes = x.numel() * 4
        lines.append(f"strong_augment ({B}, 3, {h}, {w}): x is {nbytes / 1e6:.1f} MB; cache-warm rates (every call reads the same buffers; x and y "
                     f"together {'fit' if 2 * nbytes < 256 * 2 ** 20 else 'do NOT fit'} the 256 MiB Infinity Cache)")
        for name, tab in tables(ops, B).items():
            dev = torch.from_numpy(ops.check_strong_table(tab, B).view(np.int32).reshape(B, ops.STRONG_REC_WORDS)).cuda()
            y, mean = ops.strong_augment(x, dev, return_mean=True)
            yt, mt = torch_composition(x, tab)
            err, merr = float((y - yt).abs().max()), float((mean - mt).abs().max())
            if err > 2e-5 or merr > 1e-5:
                raise RuntimeError(f"ops.strong_augment and the torch composition disagree ({name}: {err:.3e}, mean {merr:.3e})")
            ms = timed(lambda: ops.strong_augment(x, dev), a.iters)
            ms_t = timed(lambda: torch_composition(x, tab), max(5, a.iters // 10), warm=3)
            moved = nbytes * (3 if tab["jitter_on"].any() else 2)
            lines.append(f"  {name:20s} kernels {ms:8.4f} ms  {moved / 1e6:7.1f} MB (x {'twice' if tab['jitter_on'].any() else 'once'} + y)  "
                         f"{moved / 1e6 / ms:7.1f} GB/s | torch operators {ms_t:9.4f} ms = {ms_t / ms:5.1f} x | largest difference {err:.2e}")
            del y, mean, yt, mt
        del x
        torch.cuda.empty_cache()
    lines += kernel_registers()
    # ---- the whole step ------------------------------------------------------------------------------------------------------------
    if not a.skip_step:
        def child(tree):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", "--tree", tree, "--step-iters", str(a.step_iters)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError("the step's child process failed: " + r.stderr.strip()[-400:])
            return json.loads(r.stdout.strip().splitlines()[-1])["ms"]

        off, on, here, parent = [], [], [], []
        for _ in range(a.repeats):  # alternating, so that a drift of the machine lands on every variant
            off.append(step_ms(a.step_iters, strong=False))
            on.append(step_ms(a.step_iters, strong=True))
            if a.parent_tree:
                here.append(child(ROOT))
                parent.append(child(os.path.abspath(a.parent_tree)))
        show = lambda v: f"{np.median(v):9.3f} ms  (runs: {', '.join(f'{t:.3f}' for t in v)})"
        lines.append(f"SelfTrainingStep.step, mit_b3, batch 8, crop 512, cross-set mix, eval-mode regime; {a.repeats} alternating runs, median:")
        lines.append(f"  strong=None                                   {show(off)}")
        lines.append(f"  strong=StrongAugment(jitter 1.0, blur 1.0)    {show(on)}  = {np.median(on) - np.median(off):+.3f} ms")
        if a.parent_tree:
            lines.append(f"  strong=None, fresh child process              {show(here)}")
            lines.append(f"  parent commit, fresh child process            {show(parent)}  -> off against the parent: "
                         f"{np.median(here) - np.median(parent):+.3f} ms, spread of one variant's runs {max(here) - min(here):.3f} / {max(parent) - min(parent):.3f} ms")
        else:
            lines.append("  parent commit: NOT recorded (no --parent-tree)")
    lines.append("note: synthetic inputs and random weights; nothing here was measured about mIoU")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
