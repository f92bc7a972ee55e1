"""Records tests/golden/seg_objectives.npz: what the upstream reference's core/loss.py gives for the segmentation objectives that
segmif_amd evaluates through csrc/seg_objective.hip (NormalLoss, SoftmaxFocalLoss, OhemCELoss).  Generator only - it needs a
checkout of the reference, which the tests do not:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_seg_objectives.py

The REAL reference classes are built and called on CPU float32 tensors (oracle/make_golden_train.py's loaders, imported, not
edited: .cuda() is the identity while they run).  The fixture holds arrays only, no program text:

    logits (2,9,29,41) = randn * 2, labels (2,29,41) uniform in [0, 9) with about 15 % set to 255
    value:CASE, grad:CASE   value and gradient w.r.t. the logits of
        normal                          NormalLoss()
        focal_g2, focal_g05             SoftmaxFocalLoss(2.0), SoftmaxFocalLoss(0.5)
        ohem_thresh                     OhemCELoss(0.7, n_gt // 4)               threshold branch
        ohem_thresh_low                 OhemCELoss(0.05, n_gt(0.05) // 4)        threshold branch, a high threshold on the loss
        ohem_topk_valid                 OhemCELoss(0.7, (n_gt + n_valid) // 2)   top-k branch, the k-th value is a valid pixel's
        ohem_topk_ignored               OhemCELoss(0.7, rows - 100)              top-k branch, the k-th value is an ignored pixel's 0
    thresh:CASE, n_min:CASE for the OHEM cases
    margin, seed    OHEM selects pixels: the inputs are reseeded until, in float64, no pixel's loss is within MARGIN = 1e-4 of
                    either threshold -log(0.7), -log(0.05) and the k-th and (k+1)-th sorted losses of ohem_topk_valid differ by at
                    least MARGIN - far above float32 rounding of a loss of a few units - so a float32 evaluation selects the same
                    pixels and the gradients can be compared element-wise.  margin is the smallest gap found.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SHAPE, CLASSES = (2, 29, 41), 9
MARGIN = 1e-4
T_HI, T_LO = 0.7, 0.05


def inputs(seed):
    B, H, W = SHAPE
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, CLASSES, H, W, generator=g, dtype=torch.float32) * 2.0
    labels = torch.randint(0, CLASSES, (B, H, W), generator=g, dtype=torch.int64)
    labels[torch.rand(B, H, W, generator=g) < 0.15] = 255
    return logits, labels


def neg_log(thresh):
    return float(-torch.log(torch.tensor(thresh, dtype=torch.float)))


def plan(logits, labels):
    """the four OHEM cases' (thresh, n_min) for these inputs and the float64 selection margin"""
    l = torch.nn.functional.cross_entropy(logits.double(), labels, ignore_index=255, reduction="none").view(-1)
    rows, n_valid = l.numel(), int((labels != 255).sum())
    n_hi, n_lo = int((l > neg_log(T_HI)).sum()), int((l > neg_log(T_LO)).sum())
    cases = {"ohem_thresh": (T_HI, n_hi // 4), "ohem_thresh_low": (T_LO, n_lo // 4),
             "ohem_topk_valid": (T_HI, (n_hi + n_valid) // 2), "ohem_topk_ignored": (T_HI, rows - 100)}
    s, _ = torch.sort(l, descending=True)
    k = cases["ohem_topk_valid"][1]
    margin = min(float((l - neg_log(T_HI)).abs().min()), float((l - neg_log(T_LO)).abs().min()), float(s[k - 1] - s[k]))
    ok = n_hi // 4 >= 1 and n_lo // 4 >= 1 and n_hi < k <= n_valid and n_valid < rows - 100
    return cases, margin, ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "seg_objectives.npz"))
    args = ap.parse_args()
    import refload
    from make_golden_train import cuda_is_identity, load_reference_losses, npy
    refload.load_reference()
    with cuda_is_identity():
        _, loss_mod = load_reference_losses()
    for seed in range(1000):
        logits, labels = inputs(seed)
        cases, margin, ok = plan(logits, labels)
        print(f"seed {seed}: margin {margin:.3e}{'' if ok else ' (case sizes do not fit)'}")
        if ok and margin >= MARGIN:
            break
    else:
        raise RuntimeError("no seed meets the selection margin")
    rec = {"logits": npy(logits), "labels": npy(labels), "margin": np.float64(margin), "seed": np.int64(seed)}
    build = {"normal": lambda: loss_mod.NormalLoss(), "focal_g2": lambda: loss_mod.SoftmaxFocalLoss(2.0),
             "focal_g05": lambda: loss_mod.SoftmaxFocalLoss(0.5)}
    for name, (thresh, n_min) in cases.items():
        build[name] = lambda thresh=thresh, n_min=n_min: loss_mod.OhemCELoss(thresh, n_min)
        rec["thresh:" + name], rec["n_min:" + name] = np.float64(thresh), np.int64(n_min)
    for name, make in build.items():
        with cuda_is_identity():
            fn = make()
            x = logits.clone().requires_grad_(True)
            v = fn(x, labels)
            (g,) = torch.autograd.grad(v, x)
        rec["value:" + name], rec["grad:" + name] = np.float64(v.detach()), npy(g)
        print(f"{name}: {float(v.detach()):.8f}  max |grad| {float(g.abs().max()):.3e}  nonzero grad pixels {int((g.abs().sum(1) > 0).sum())}")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
