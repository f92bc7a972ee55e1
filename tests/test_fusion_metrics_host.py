"""Host-side checks of the fusion-quality metrics: fusion_scores on hand-made statistics against closed forms, the descriptor
rejections of the new C entry points, and the MFNet palette against the reference's recorded one.  No kernel is launched."""
import json
import os

import numpy as np
import pytest

from _fusion_ref import ref_scores, ref_stats


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def stats_of(fused, vis, ir):
    """FusionStats built with numpy (tests/_fusion_ref.py) from (B, H, W[, 3]) uint8 images"""
    from segmif_amd.utils.fusion_metrics import FusionStats
    jfa, jfv, sums, ag = ref_stats(fused, vis, ir)
    return FusionStats(jfa, jfv, sums, ag, tuple(ir.shape[1:]))


def grey(plane):
    """(B, H, W) uint8 -> (B, H, W, 3) with R = G = B: its luma is the plane itself ((1000 g + 500) // 1000 = g)"""
    return np.repeat(plane[..., None], 3, axis=3)


def test_constant_image_scores():
    from segmif_amd.utils.fusion_metrics import SCORE_NAMES, fusion_scores
    f = np.full((2, 5, 7), 93, dtype=np.uint8)
    ir = np.arange(70, dtype=np.uint8).reshape(2, 5, 7)
    vis = grey((3 * np.arange(70) % 251).astype(np.uint8).reshape(2, 5, 7))
    s = fusion_scores(stats_of(grey(f), vis, ir))
    assert sorted(s) == sorted(SCORE_NAMES) and all(v.shape == (2,) and v.dtype == np.float64 for v in s.values())
    for k in ("EN", "SD", "SF", "AG"):
        assert np.array_equal(s[k], np.zeros(2)), k
    assert np.abs(s["MI"]).max() < 1e-14  # a constant f shares no information with anything (p_f sums to 1 up to rounding)
    assert np.isnan(s["CC"]).all()
    assert np.isfinite(s["PSNR"]).all() and np.isfinite(s["SCD"]).all()  # f - v and f - a vary: SCD is defined


def test_identical_images_scores():
    from segmif_amd.utils.fusion_metrics import fusion_scores
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (3, 9, 11), dtype=np.uint8)
    s = fusion_scores(stats_of(grey(f), grey(f), f))
    assert (s["EN"] > 3).all()
    np.testing.assert_allclose(s["MI"], 2 * s["EN"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(s["CC"], np.ones(3), rtol=1e-15, atol=0)
    assert np.isposinf(s["PSNR"]).all()
    assert np.isnan(s["SCD"]).all()  # f - v = f - a = 0: zero variance


def test_checkerboard_scores_worked_by_hand():
    """f[y][x] = 40 on even x + y, 100 on odd, H = 4, W = 6, d = 60.  Every horizontal and every vertical neighbour pair
    differs by d: RF^2 = H (W - 1) d^2 / (H W) = 20 * 3600 / 24 = 3000, CF^2 = (H - 1) W d^2 / (H W) = 18 * 3600 / 24 = 2700,
    SF = sqrt(5700).  Each of the (H - 1)(W - 1) = 15 gradient terms is sqrt((d^2 + d^2) / 2) = d, so AG = 60.  Twelve pixels
    of each level: EN = 1 bit, mean 70, SD = 30.  a = f: MI(f, a) = EN; v = 255 - f: MI(f, v) = EN, r(f, v) = -1, CC = 0.
    MSE(f, a) = 0, MSE(f, v) = (12 * 175^2 + 12 * 55^2) / 24 = 16 825, PSNR = 10 log10(65 025 / 8412.5).
    SCD = r(f - v, a) + r(f - a, v): f - v = 2 f - 255 correlates with a = f at +1; f - a = 0 is constant: NaN."""
    from segmif_amd.utils.fusion_metrics import fusion_scores
    yy, xx = np.mgrid[0:4, 0:6]
    f = np.where((yy + xx) % 2 == 0, 40, 100).astype(np.uint8)[None]
    s = fusion_scores(stats_of(grey(f), grey(255 - f), f))
    assert s["SF"][0] == pytest.approx(np.sqrt(5700.0), rel=1e-15)
    assert s["AG"][0] == 60.0 and s["SD"][0] == 30.0 and s["EN"][0] == 1.0
    assert s["MI"][0] == pytest.approx(2.0, rel=1e-15)
    assert s["CC"][0] == pytest.approx(0.0, abs=1e-16)
    assert s["PSNR"][0] == pytest.approx(10 * np.log10(65025 / 8412.5), rel=1e-15)
    assert np.isnan(s["SCD"][0])
    # and with an infrared image that is not f: both SCD terms defined; against the direct evaluation on the pixels
    ir = ((7 * xx + 13 * yy) % 256).astype(np.uint8)[None]
    got, ref = fusion_scores(stats_of(grey(f), grey(255 - f), ir)), ref_scores(grey(f), grey(255 - f), ir)
    for k in ref:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, err_msg=k)


def test_scores_refuse_a_record_without_its_shape():
    from segmif_amd.utils.fusion_metrics import FusionStats, fusion_scores
    z = np.zeros((1, 256, 256), dtype=np.int64)
    with pytest.raises(RuntimeError, match="shape"):
        fusion_scores(FusionStats(z, z, np.zeros((1, 4), dtype=np.int64), np.zeros(1)))


def test_new_entry_points_reject_bad_descriptors_without_a_gpu(lib):
    p = 64  # any non-null address: the arguments are validated before anything is touched
    assert lib.segmif_fusion_stats_workspace_bytes(64, 480, 640) == 64 * 8
    assert lib.segmif_fusion_stats_workspace_bytes(1, 1, 640) == 0 and lib.segmif_fusion_stats_workspace_bytes(0, 8, 8) == 0
    assert lib.segmif_fusion_stats_u8(p, p, p, p, p, p, p, p, 1, 1, 8, 0, None) == -22      # H = 1
    assert lib.segmif_fusion_stats_u8(p, p, p, p, p, p, p, p, 1, 8, 1, 0, None) == -22      # W = 1
    assert lib.segmif_fusion_stats_u8(p, p, p, p, p, p, p, p, 0, 8, 8, 0, None) == -22      # B = 0
    for hole in range(8):                                                                    # each pointer null in turn
        args = [p] * 8
        args[hole] = None
        assert lib.segmif_fusion_stats_u8(*args, 1, 8, 8, 0, None) == -22, hole
    assert lib.segmif_palette_u8(p, p, p, 16, 0, None) == -22                                # K = 0
    assert lib.segmif_palette_u8(p, p, p, 16, 257, None) == -22                              # K = 257
    assert lib.segmif_palette_u8(None, p, p, 16, 9, None) == -22
    assert lib.segmif_palette_u8(p, None, p, 16, 9, None) == -22 and lib.segmif_palette_u8(p, p, None, 16, 9, None) == -22
    assert lib.segmif_palette_u8(p, p, p, -1, 9, None) == -22


def test_mfnet_palette_is_the_reference_one(golden_dir):
    from segmif_amd.utils.fusion_metrics import MFNET_PALETTE
    g = json.load(open(os.path.join(golden_dir, "palette_mfnet.json")))
    assert MFNET_PALETTE.dtype == np.uint8 and MFNET_PALETTE.shape == (9, 3) and len(g["names"]) == 9
    assert np.array_equal(MFNET_PALETTE, np.array(g["palette"]))


def test_device_entry_points_refuse_cpu_tensors_and_pair_forward_flag_needs_the_roundtrip():
    import torch
    from segmif_amd.pipeline import PairForward
    from segmif_amd.utils import fusion_metrics as fm
    u = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.fusion_stats(u, u, u[..., 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fm.colorize(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        PairForward(None, None, return_u8=True)
    assert PairForward(None, None, uint8_roundtrip=True, return_u8=True).return_u8
