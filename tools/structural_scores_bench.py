"""Cost of the structural-scores pass (Qabf, SSIM, VIF) per call, beside fusion_stats on the same inputs.

Times segmif_amd.utils.fusion_metrics.structural_stats and fusion_stats with device events (warm-up, >= 20 timed calls each,
the two alternating inside one process) at (8, 480, 640) and (64, 480, 640) on smooth and on uniform-noise images, and
prints the medians beside the pair forward the pass sits behind (--pair-ms: the README's 195 ms per 64 pairs, scaled to the
batch).  No target is set: a cost above a few per cent of the pair forward is printed as a finding.  --errors FILE appends
the observed test errors (the lines tests/test_gpu_structural_scores.py prints with -s) under the table.

    python tools/structural_scores_bench.py --out profiles/structural_scores_bench.txt [--errors structural_tests.log]
"""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def time_both(inputs, warmup, repeats):
    from segmif_amd.utils.fusion_metrics import fusion_stats, structural_stats
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs]
    outs = {"structural_stats": structural_stats(*dev), "fusion_stats": fusion_stats(*dev)}
    fns = {"structural_stats": structural_stats, "fusion_stats": fusion_stats}
    for _ in range(warmup):
        for name, fn in fns.items():
            fn(*dev, out=outs[name])
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(*dev, out=outs[name])
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: np.array(v) for name, v in ms.items()}


def observed_errors(path):
    """the largest printed error per score over the log of the GPU tests"""
    worst = {}
    pat = re.compile(r"^\.*(Qabf|SSIM_ir|SSIM_vis|SSIM|VIF_ir|VIF_vis|VIF) (.*): max (relative|absolute) error ([0-9.e+-]+) \(gate ([0-9.e+-]+)\)")
    for line in open(path):
        m = pat.match(line.strip())
        if m and "evaluator" not in m.group(2):
            k, e = m.group(1), float(m.group(4))
            if k not in worst or e > worst[k][0]:
                worst[k] = (e, m.group(2), m.group(3), m.group(5))
    return worst


def main():
    from fusion_stats_bench import clock_state, noise_inputs, smooth_inputs
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--pair-ms", type=float, default=195.0, help="the pair forward's time per 64 pairs (README)")
    ap.add_argument("--errors", help="log of the GPU tests run with -s: their largest observed errors are appended")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("structural_scores_bench needs the MI355X: a CPU run gives no time")
    if args.repeats < 20:
        raise RuntimeError("--repeats must be at least 20")
    H, W = args.height, args.width
    lines = [f"structural_stats (Qabf, SSIM, VIF) and fusion_stats, images of {H} x {W}, device events, {args.warmup} warm-up + "
             f"{args.repeats} timed calls each, alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", "clock state:", clock_state(), "",
             f"{'batch':>5}  {'input':<24}{'call':<18}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'% of pair forward':>19}"]
    rng = np.random.default_rng(0)
    worst_share = 0.0
    for B in args.batches:
        pair = args.pair_ms * B / 64.0
        for name, make in (("smooth", smooth_inputs), ("uniform noise", noise_inputs)):
            for call, ms in time_both(make(rng, B, H, W), args.warmup, args.repeats).items():
                share = 100.0 * float(np.median(ms)) / pair
                if call == "structural_stats":
                    worst_share = max(worst_share, share)
                lines.append(f"{B:>5}  {name:<24}{call:<18}{np.median(ms):>11.4f}{ms.min():>9.4f}{ms.max():>9.4f}{share:>18.2f}%")
    lines += ["", f"pair forward: {args.pair_ms:.1f} ms per 64 pairs (README), scaled to the batch; not measured in this run",
              f"structural_stats, worst case: {worst_share:.2f} % of the pair forward"
              + ("  -> FINDING: above a few per cent" if worst_share > 3.0 else "")]
    if args.errors:
        lines += ["", "largest observed errors of tests/test_gpu_structural_scores.py against the float64 restatement:"]
        for k, (e, what, kind, gate) in observed_errors(args.errors).items():
            lines.append(f"  {k:<9}{e:.3e} {kind} (gate {gate}; {what})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
