"""One FusionTrainer step of an ablation fusion net (core/variants.py) at 480 x 640, B = 2, for profiling:
    python tools/variant_train_step.py Fusion_Network3_Average [--steps 3]
Warms up two steps, then times --steps steps with device events and prints the mean step time (ms).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/variant_train_step.py NAME` for the kernel table."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import detweights as dw  # noqa: E402
from segmif_amd.core import Network3, model_fusion as mf  # noqa: E402
from segmif_amd.train import FusionTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    seg = Network3("mit_b1", 9, pretrained=None)
    dw.load_det_weights(seg, seed=0)
    seg = seg.cuda().eval()
    fus = getattr(mf, a.name)()
    dw.load_det_weights(fus, seed=0)
    fus = fus.cuda().train()
    opt = torch.optim.AdamW(fus.parameters(), lr=1e-5)
    tr = FusionTrainer(seg, fus, opt, torch.nn.CrossEntropyLoss(ignore_index=255), iter_=2)
    B, H, W = a.batch, a.height, a.width
    ir3 = dw.det_input("vts_ir", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
    vis3 = dw.det_input("vts_vis", (B, 3, H, W)).cuda()
    mask3 = dw.det_input("vts_mask", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
    labels = dw.det_labels("vts_y", (B, H, W), 9).cuda()
    for _ in range(2):
        tr.step(ir3, vis3, mask3, labels)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        loss = tr.step(ir3, vis3, mask3, labels)
    t1.record()
    torch.cuda.synchronize()
    print(f"{a.name} B={B} {H}x{W}: {t0.elapsed_time(t1) / a.steps:.2f} ms per FusionTrainer step (mean of {a.steps}), "
          f"loss {float(loss):.6f}", flush=True)


if __name__ == "__main__":
    main()
