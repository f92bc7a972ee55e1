"""Cost of the fusion-statistics pass beside the forward step it sits behind.

Times segmif_amd.utils.fusion_metrics.fusion_stats alone on 64 pairs of 480 x 640 with hip events (warm-up, >= 20 repeats),
for a diagonal-heavy input (smooth images: the joint histograms collide) and for uniform noise (the histograms spread out:
the flush is the largest), and prints the result beside the forward step's `ms_per_step` (bench.py's headline line, measured in
the same session: pass the file holding its output with --bench-json, or the number with --step-ms).  Budget: the worse of
the two inputs below 2 % of the step.

    python bench.py --gpus 1 --steps 10 --warmup 3 > bench.out
    python tools/fusion_stats_bench.py --bench-json bench.out --out profiles/fusion_stats_bench.txt
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def smooth_inputs(rng, B, H, W):
    """one smooth field under all three images plus a little noise: neighbouring pixels and the three images are close"""
    coarse = rng.uniform(20, 235, (B, (H + 7) // 8, (W + 7) // 8))
    base = np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :H, :W]
    for ax in (1, 2):
        base = (base + np.roll(base, 1, axis=ax) + np.roll(base, 2, axis=ax) + np.roll(base, 3, axis=ax)) / 4
    u8 = lambda x: np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return (u8(base[..., None] + rng.normal(0, 1.5, (B, H, W, 3))), u8(base[..., None] + rng.normal(0, 2, (B, H, W, 3))),
            u8(base + rng.normal(0, 2, (B, H, W))))


def noise_inputs(rng, B, H, W):
    return (rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8),
            rng.integers(0, 256, (B, H, W), dtype=np.uint8))


def time_stats(inputs, warmup, repeats):
    from segmif_amd.utils.fusion_metrics import fusion_stats
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs]
    out = fusion_stats(*dev)
    for _ in range(warmup):
        fusion_stats(*dev, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fusion_stats(*dev, out=out)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    occupied = int((out.joint_fa[0] > 0).sum())
    return np.array(ms), occupied


def headline_ms(path):
    """ms_per_step of the last JSON line in `path` that has one at its top level"""
    found = None
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            try:
                rec = json.loads(line)
            except ValueError:
                continue
            if "ms_per_step" in rec:
                found = float(rec["ms_per_step"])
    if found is None:
        raise RuntimeError(f"no JSON line with ms_per_step in {path}")
    return found


def clock_state():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        lines = [l for l in r.stdout.splitlines() if "GPU[0]" in l]
        return "\n".join(lines) if lines else "rocm-smi printed nothing for GPU[0]"
    except (OSError, subprocess.SubprocessError) as e:
        return f"clock state not available ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--bench-json", help="file holding bench.py's output of the same session")
    ap.add_argument("--step-ms", type=float, help="the forward step's ms_per_step, if not read from --bench-json")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fusion_stats_bench needs the MI355X: a CPU run gives no time")
    if args.repeats < 20:
        raise RuntimeError("--repeats must be at least 20")
    step = args.step_ms if args.step_ms is not None else (headline_ms(args.bench_json) if args.bench_json else None)
    B, H, W = args.batch, args.height, args.width
    rng = np.random.default_rng(0)
    rows = []
    for name, make in (("diagonal-heavy (smooth)", smooth_inputs), ("uniform noise", noise_inputs)):
        ms, occupied = time_stats(make(rng, B, H, W), args.warmup, args.repeats)
        rows.append((name, ms, occupied))
    lines = [f"fusion_stats alone, {B} pairs of {H} x {W}, hip events, {args.warmup} warm-up + {args.repeats} timed calls",
             f"device: {torch.cuda.get_device_name(0)}", "clock state:", clock_state(), "",
             f"{'input':<26}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'bins of image 0 in use':>25}"]
    for name, ms, occupied in rows:
        lines.append(f"{name:<26}{np.median(ms):>11.4f}{ms.min():>9.4f}{ms.max():>9.4f}{occupied:>25d}")
    worst = max(float(np.median(ms)) for _, ms, _ in rows)
    lines.append("")
    if step is None:
        lines.append("forward step: not measured in this run (pass --bench-json or --step-ms)")
    else:
        ratio = worst / step
        lines += [f"forward step (bench.py headline, same session): {step:.3f} ms",
                  f"stats pass, worse input, over the step: {100 * ratio:.3f} %  (budget: below 2 %) -> {'within' if ratio < 0.02 else 'OVER'} budget"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if step is None or worst / step < 0.02 else 1


if __name__ == "__main__":
    sys.exit(main())
