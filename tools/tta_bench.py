"""Cost of multi-scale + flip inference, measured with device events.

(a) ops.tta_vote on the default 12 views of 480 x 640 frames - quarter-resolution logit maps, 9 classes, 64 images - beside
    the same composition from torch operators on the device (per view: F.interpolate to full size, softmax, flip, add; then
    the division and the argmax), the two alternating inside one process, labels compared.
(b) Network3.predict_labels_tta (default TTA) beside predict_labels for mit_b3 on 8 frames of 480 x 640, seeded random weights,
    with the range guard's statistics of the multi-view scope.

No target is set.  --errors FILE appends the lines tests/test_gpu_tta.py prints with -s (observed errors and yardsticks).

    python tools/tta_bench.py --out profiles/tta_bench.txt [--errors tta_tests.log]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, warmup, repeats):
    """fns: name -> callable; -> name -> np.array of ms per call (device events; the callables alternate)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: np.array(v) for name, v in ms.items()}


def torch_vote(views, flips, OH, OW):
    total = None
    for x, f in zip(views, flips):
        p = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).softmax(1)
        if f:
            p = p.flip(3)
        total = p if total is None else total.add_(p)
    return total.div_(len(views)).argmax(1)


def row(name, ms):
    return f"  {name:<34}{np.median(ms):>11.3f}{ms.min():>10.3f}{ms.max():>10.3f}"


def main():
    from segmif_amd import ops
    from segmif_amd.tta import TTA
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--vote-batch", type=int, default=64)
    ap.add_argument("--net-batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--backbone", default="mit_b3")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-net", action="store_true", help="part (a) only")
    ap.add_argument("--errors", help="log of tests/test_gpu_tta.py run with -s: its printed figures are appended")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tta_bench needs the MI355X: a CPU run gives no time")
    H, W, C, tta = args.height, args.width, args.classes, TTA()
    plan = tta.plan(H, W)
    flips = [f for _, _, f in plan]
    head = f"  {'call':<34}{'median ms':>11}{'min ms':>10}{'max ms':>10}"
    lines = [f"multi-scale + flip inference, frames of {H} x {W}, {len(plan)} views {[(h, w) for h, w, f in plan if not f]} (each also "
             f"mirrored: {tta.flip}), device events, {args.warmup} warm-up + {args.repeats} timed calls each, alternating in one process",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    B = args.vote_batch
    g = torch.Generator(device="cuda").manual_seed(0)
    views = [3.0 * torch.randn(B, h // 4, w // 4, C, device="cuda", generator=g) for h, w, _ in plan]
    moved = 4.0 * (sum(v.numel() for v in views) + B * H * W)
    ms = timed({"ops.tta_vote": lambda: ops.tta_vote(views, flips, H, W),
                "torch operators": lambda: torch_vote(views, flips, H, W)}, args.warmup, args.repeats)
    differ = int((ops.tta_vote(views, flips, H, W) != torch_vote(views, flips, H, W)).sum())
    lines += [f"(a) the vote: {B} images, {C} classes, logits N(0, 3^2); the kernel reads {moved / 1e6:.0f} MB of logits + writes labels "
              "(from the shapes)", head] + [row(k, v) for k, v in ms.items()]
    lines += [f"  ratio of the medians (torch operators / ops.tta_vote): {np.median(ms['torch operators']) / np.median(ms['ops.tta_vote']):.1f}",
              f"  labels that differ between the two: {differ} of {B * H * W}", ""]
    del views

    if not args.skip_net:
        from segmif_amd import guard
        from segmif_amd.core import Network3
        torch.manual_seed(0)
        net = Network3(args.backbone, C, pretrained=None).cuda().eval()
        B = args.net_batch
        fused = torch.rand(B, 3, H, W, device="cuda", generator=g)
        with torch.no_grad():
            before = guard.range_stats()
            ms = timed({"predict_labels": lambda: net.predict_labels(fused),
                        "predict_labels_tta": lambda: net.predict_labels_tta(fused, tta=tta)}, args.warmup, args.repeats)
            after = guard.range_stats()
            moved_px = float((net.predict_labels(fused) != net.predict_labels_tta(fused, tta=tta)).float().mean())
        lines += [f"(b) {args.backbone}, {B} frames, seeded random weights (torch.manual_seed(0)), uniform random frames", head]
        lines += [row(k, v) for k, v in ms.items()]
        lines += [f"  ratio of the medians (predict_labels_tta / predict_labels): "
                  f"{np.median(ms['predict_labels_tta']) / np.median(ms['predict_labels']):.1f}"
                  f"  (sum of the views' areas / the frame's: {sum(h * w for h, w, _ in plan) / (H * W):.1f})",
                  f"  pixels whose label the vote changes (random weights: no statement about accuracy): {100 * moved_px:.1f} %",
                  "  range guard over these calls: " + ", ".join(f"{k} +{after[k] - before[k]}" for k in
                                                                ("scopes", "images", "images_repeated", "images_repeated_fp32conv", "slot_rows_shared")), ""]

    if args.errors:
        lines += ["figures printed by tests/test_gpu_tta.py (float64 restatement tests/_tta_ref.py):"]
        for line in open(args.errors):
            line = line.strip().lstrip(".")
            if line.startswith(("tta_vote C=", "stand-in chain:")):
                lines.append("  " + line)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
