"""Times the optimizer step on the MI355X, three ways, over the parameters of Network3('mit_b3') and of Fusion_Network3_ac
with seeded random gradients:

    plain     FusedAdamW.step()                                          one multi-tensor launch
    guarded   FusedAdamW(max_grad_norm=1, skip_nonfinite=True).step()    norm (two launches) + guarded update
    torchclip torch.nn.utils.clip_grad_norm_ then the plain step         torch's foreach chain, then one launch

Device events around a window of --steps steps (so the host's share of a step - building and uploading the table - is inside the
figure, as it is in training), --warmup steps first, --repeats windows per variant with the variants alternating; the table
reports the median and the spread per step.  The byte counts are what the algorithm moves: the update reads p, g, m, v and
writes p, m, v (seven streams of 4 bytes per element), the norm reads g once more.

    python tools/guarded_step_bench.py [--out profiles/guarded_step_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def bench(name, module, args, lines):
    from segmif_amd.utils.optimizer import FusedAdamW
    params = [p for p in module.parameters() if p.requires_grad]
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
    n = sum(p.numel() for p in params)
    kw = dict(lr=1e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    plain, guarded, after_clip = FusedAdamW(params, **kw), FusedAdamW(params, max_grad_norm=1.0, skip_nonfinite=True, **kw), FusedAdamW(params, **kw)

    def torchclip():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        after_clip.step()

    variants = [("plain", plain.step), ("guarded", guarded.step), ("torchclip", torchclip)]
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in variants}
    for _ in range(args.repeats):
        for k, fn in variants:
            times[k].append(window(fn, args.steps))
    st = guarded.grad_stats()
    assert st["skipped"] == 0 and st["attempts"] == args.warmup + args.repeats * args.steps, st
    lines.append(f"{name}: {len(params)} tensors, {n} elements; update traffic {7 * 4 * n / 1e6:.1f} MB, norm pass {4 * n / 1e6:.1f} MB more")
    base = statistics.median(times["plain"])
    for k, _ in variants:
        t = times[k]
        med = statistics.median(t)
        lines.append(f"  {k:<10} median {med:8.4f} ms/step   min {min(t):8.4f}   max {max(t):8.4f}   x{med / base:5.3f} of plain")
    lines.append(f"  guarded run: norm {st['norm']:.4f} clipped {st['clipped']} of {st['attempts']} steps")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9, help="windows per variant (alternating)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guarded_step_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("guarded_step_bench needs the MI355X: a timing from anywhere else says nothing about it")
    from segmif_amd.core import Fusion_Network3_ac, Network3
    torch.manual_seed(0)
    lines = [f"optimizer step, device events over {args.repeats} windows of {args.steps} steps after {args.warmup} warm-up steps, "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    bench("Network3('mit_b3')", Network3("mit_b3", 9, pretrained=None).cuda(), args, lines)
    bench("Fusion_Network3_ac", Fusion_Network3_ac().cuda(), args, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
