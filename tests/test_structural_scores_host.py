"""Host-side checks of the structural fusion scores (Qabf, SSIM, VIF): the float64 restatement against the reference's recorded
pytorch_ssim values, structural_scores on hand-made statistics, the size rule and the rejections of the C entry points, the
score names and the command's flag.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _fusion_ref import luma
from _structural_ref import ssim_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The reference's float32 evaluation was measured at most 9.3e-7 (the issue: 5.2e-7) from the float64 definition on these
# kinds; 2e-6 leaves room for other float32 summation orders of the 121-tap convolutions.
RECORD_ATOL = 2e-6


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_restated_ssim_matches_the_reference_record(golden_dir):
    g = np.load(os.path.join(golden_dir, "structural_scores.npz"))
    worst = 0.0
    for kind in ("smooth", "noise"):
        fused, vis, ir = g[f"{kind}:fused"], g[f"{kind}:vis"], g[f"{kind}:ir"]
        assert fused.shape == (2, 64, 96, 3) and fused.dtype == np.uint8 and g[f"{kind}:ssim_ir"].dtype == np.float32
        for b in range(2):
            f, v, a = luma(fused[b]), luma(vis[b]), ir[b].astype(np.int64)
            for name, src in (("ssim_ir", a), ("ssim_vis", v)):
                err = abs(ssim_map(f, src).mean() - float(g[f"{kind}:{name}"][b]))
                worst = max(worst, err)
                assert err <= RECORD_ATOL, (kind, b, name, err)
    print(f"largest |restatement - reference record| = {worst:.3e} (gate {RECORD_ATOL:.0e})")


def test_structural_scores_on_hand_made_statistics():
    from segmif_amd.utils.fusion_metrics import StructuralStats, structural_scores
    qabf = np.array([[3.0, 4.0], [0.0, 0.0], [1.0, 8.0]])
    ssim = np.array([[60.0, 30.0], [120.0, 120.0], [-12.0, 0.0]])        # H W = 120
    vif = np.zeros((3, 2, 4, 2))
    vif[0, 0, :, 0], vif[0, 0, :, 1] = [1, 2, 3, 4], [2, 4, 6, 8]          # 10 / 20
    vif[0, 1, :, 0], vif[0, 1, :, 1] = [1, 0, 0, 0], [1, 1, 1, 1]          # 1 / 4
    vif[2, 0, :, 1] = [0, 0, 0, 2]                                         # 0 / 2; image 2's other source and image 1: den == 0
    s = structural_scores(StructuralStats(qabf, ssim, vif, (10, 12)))
    assert sorted(s) == sorted(("Qabf", "SSIM", "VIF", "SSIM_ir", "SSIM_vis", "VIF_ir", "VIF_vis"))
    assert all(v.shape == (3,) and v.dtype == np.float64 for v in s.values())
    assert s["Qabf"][0] == 0.75 and np.isnan(s["Qabf"][1]) and s["Qabf"][2] == 0.125
    assert np.array_equal(s["SSIM_ir"], [0.5, 1.0, -0.1]) and np.array_equal(s["SSIM_vis"], [0.25, 1.0, 0.0])
    assert np.array_equal(s["SSIM"], [0.375, 1.0, -0.05])                  # the mean of the two, not the sum
    assert s["VIF_ir"][0] == 0.5 and s["VIF_vis"][0] == 0.25 and s["VIF"][0] == 0.75
    assert np.isnan(s["VIF_ir"][1]) and np.isnan(s["VIF_vis"][1]) and np.isnan(s["VIF"][1])
    assert s["VIF_ir"][2] == 0.0 and np.isnan(s["VIF_vis"][2]) and np.isnan(s["VIF"][2])
    with pytest.raises(RuntimeError, match="shape"):
        structural_scores(StructuralStats(qabf, ssim, vif))
    with pytest.raises(RuntimeError, match="expected"):
        structural_scores(StructuralStats(qabf, ssim, vif[:, :, :3], (10, 12)))


def test_workspace_rule_and_rejections_without_a_gpu(lib):
    ws = lib.segmif_structural_stats_workspace_bytes
    assert ws(1, 40, 64) == 0 and ws(0, 64, 64) == 0 and ws(1, 64, 40) == 0
    assert ws(1, 41, 41) > 0 and ws(1, 41, 41) % 8 == 0
    assert ws(1, 32768, 32769) == 0                                        # H W > 2^30
    assert ws(2, 480, 640) == 2 * ws(1, 480, 640)
    p = 64  # any non-null, 8-byte aligned address: the arguments are validated before anything is touched
    fn = lib.segmif_structural_stats_u8
    assert fn(None, None, None, None, None, None, None, 1, 64, 64, None) == -22
    for hole in range(7):                                                  # each pointer null in turn
        args = [p] * 7
        args[hole] = None
        assert fn(*args, 1, 64, 64, None) == -22, hole
    assert fn(*[p] * 7, 1, 40, 64, None) == -22 and fn(*[p] * 7, 1, 64, 40, None) == -22   # below 41
    assert fn(*[p] * 7, 0, 64, 64, None) == -22                                             # B = 0
    assert fn(*[p] * 6, 68, 1, 64, 64, None) == -22                                         # workspace not 8-byte aligned


def test_score_names_are_disjoint_and_the_eight_are_unchanged():
    from segmif_amd.utils import fusion_metrics as fm
    assert fm.SCORE_NAMES == ("EN", "MI", "SD", "SF", "AG", "CC", "PSNR", "SCD")
    assert fm.STRUCTURAL_SCORE_NAMES == ("Qabf", "SSIM", "VIF")
    assert not set(fm.SCORE_NAMES) & set(fm.STRUCTURAL_SCORE_NAMES)
    assert fm.StructuralStats._fields == ("qabf", "ssim", "vif", "shape")


def test_device_entry_point_refuses_cpu_tensors():
    import torch
    from segmif_amd.utils import fusion_metrics as fm
    u = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.structural_stats(u, u, u[..., 0])


def test_help_lists_the_flag():
    r = subprocess.run([sys.executable, "-m", "segmif_amd.evaluate", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--structural-scores" in r.stdout
