"""Records tests/golden/structural_scores.npz: what the upstream reference's pytorch_ssim.ssim gives for the planes that
segmif_amd's structural scores are computed on.  Generator only - it runs on the CPU and needs a checkout of the reference,
which the tests do not:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_structural_scores.py [--reference DIR]

The fixture holds arrays only, no program text.  For each kind K of ("smooth", "noise"), from tests/_fusion_ref.make_inputs(K, 2,
64, 96):

    K:fused, K:vis (2, 64, 96, 3) uint8, K:ir (2, 64, 96) uint8
    K:ssim_ir, K:ssim_vis (2,) float32   pytorch_ssim.ssim(f / 255, a / 255) and (f / 255, v / 255) per image on float32 tensors
                                         of shape (1, 1, 64, 96), f = L(fused), v = L(vis), a = ir

Qabf and VIF are not recorded: the reference has neither.  The largest distance of the record from the float64 restatement
(tests/_structural_ref.py) is printed; tests/test_structural_scores_host.py holds it below 2e-6.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KINDS = ("smooth", "noise")
SHAPE = (2, 64, 96)


def main():
    import refload
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", default=refload.REF_ROOT, help="checkout of the reference (holds pytorch_ssim/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "structural_scores.npz"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(args.reference, "pytorch_ssim")):
        raise RuntimeError(f"{args.reference} holds no pytorch_ssim/: the record can only be made where the reference is present")
    sys.path.insert(0, args.reference)
    import pytorch_ssim
    from _fusion_ref import luma, make_inputs
    from _structural_ref import ssim_map

    rec, worst = {}, 0.0
    for kind in KINDS:
        fused, vis, ir = make_inputs(kind, *SHAPE)
        f, v, a = luma(fused), luma(vis), ir.astype(np.int64)
        t = lambda x: (torch.from_numpy(x.astype(np.float32)) / 255.0)[None, None]
        s_ir = np.array([float(pytorch_ssim.ssim(t(f[b]), t(a[b]))) for b in range(SHAPE[0])], dtype=np.float32)
        s_vis = np.array([float(pytorch_ssim.ssim(t(f[b]), t(v[b]))) for b in range(SHAPE[0])], dtype=np.float32)
        rec.update({f"{kind}:fused": fused, f"{kind}:vis": vis, f"{kind}:ir": ir, f"{kind}:ssim_ir": s_ir, f"{kind}:ssim_vis": s_vis})
        for b in range(SHAPE[0]):
            d = max(abs(float(s_ir[b]) - ssim_map(f[b], a[b]).mean()), abs(float(s_vis[b]) - ssim_map(f[b], v[b]).mean()))
            worst = max(worst, d)
        print(f"{kind}: SSIM_ir {s_ir}  SSIM_vis {s_vis}")
    print(f"largest |record - float64 restatement| = {worst:.3e}")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
