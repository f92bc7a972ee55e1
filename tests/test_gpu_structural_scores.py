"""GPU tests of the structural fusion scores (csrc/structural_stats.hip): Qabf, SSIM and the pixel-domain VIF against the
float64 numpy restatement (tests/_structural_ref.py, independent of the package), reproducibility, the out= and graph
interfaces, and the opt-in paths of the Evaluator and of the command line.

Gates (derived, not tuned; every test prints the largest error it saw):
  Qabf      rtol 1e-9: all terms positive, a sequential fp64 sum of <= 2^20 terms is bounded by 1.2e-10, libm differs by a few ulp
  SSIM_*    atol 1e-9: terms of mixed sign, values O(1)
  VIF_*     rtol 1e-7: a 289-tap fp64 moment of 255^2 values rounds by <= 2.1e-9 absolute, four moments feed a variance, the
            smallest local variance on these inputs is 0.36 -> 2.3e-8 per term, about 4 x more through g
VIF of all255 is left out: the formula is undefined for a constant non-zero plane (structural_scores' docstring)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import detweights as dw
from _fusion_ref import KINDS, SCORES, make_inputs
from _structural_ref import cached_case, ref_structural

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QABF_RTOL, SSIM_ATOL, VIF_RTOL, RECORD_ATOL = 1e-9, 1e-9, 1e-7, 2e-6
STRUCTURAL = ("Qabf", "SSIM", "VIF")
SMALL = [(1, 41, 41), (3, 45, 67), (2, 64, 96)]
CASES = [(k, s) for s in SMALL for k in KINDS] + [(k, (1, 480, 640)) for k in ("smooth", "noise")]


@pytest.fixture(scope="module")
def fm():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import fusion_metrics
    return fusion_metrics


def dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)  # (a copy: the shared cases are read-only)


def bits(st):
    return [t.cpu().numpy().view(np.int64) for t in (st.qabf, st.ssim, st.vif)]


def assert_scores(got, ref, what, vif=True):
    """got: structural_scores' dict, ref: the restatement's -> asserts every gate, NaN in the same places; prints the errors"""
    for k, rtol, atol in (("Qabf", QABF_RTOL, 0.0), ("SSIM_ir", 0.0, SSIM_ATOL), ("SSIM_vis", 0.0, SSIM_ATOL), ("SSIM", 0.0, SSIM_ATOL),
                          ("VIF_ir", VIF_RTOL, 0.0), ("VIF_vis", VIF_RTOL, 0.0), ("VIF", VIF_RTOL, 0.0)):
        if k.startswith("VIF") and not vif:
            continue
        g, r = got[k], ref[k]
        assert g.shape == r.shape and g.dtype == np.float64, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, k, g, r)
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok]) / (np.abs(r[ok]) if rtol else 1.0)
        print(f"{k} {what}: max {'relative' if rtol else 'absolute'} error {err.max() if err.size else 0.0:.3e} (gate {rtol or atol:.0e})")
        np.testing.assert_allclose(g[ok], r[ok], rtol=rtol, atol=atol, err_msg=f"{k} {what}")


@pytest.mark.parametrize("kind,shape", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_scores_against_the_restatement(fm, kind, shape):
    """The device sums through structural_scores against the float64 restatement on the same uint8 images.  Precondition of the
    VIF gate, asserted from the restatement: every local variance is <= 1e-12 or >= 1e-2, so no branch depends on rounding."""
    (fused, vis, ir), ref = cached_case(kind, *shape)
    vif = kind != "all255"
    if vif:
        var = ref["variances"]
        assert not ((var > 1e-12) & (var < 1e-2)).any(), (kind, shape, var[(var > 1e-12) & (var < 1e-2)][:4])
    st = fm.structural_stats(*dev(fused, vis, ir))
    assert st.shape == shape[1:] and st.qabf.dtype == torch.float64 and tuple(st.vif.shape) == (shape[0], 2, 4, 2)
    assert_scores(fm.structural_scores(st), ref, f"{kind} {shape}", vif=vif)
    again = fm.structural_stats(*dev(fused, vis, ir))
    for x, y in zip(bits(st), bits(again)):  # bit-identical run to run (NaN-free sums: den == 0 is a plain zero here)
        assert np.array_equal(x, y)


def test_an_image_does_not_depend_on_its_batch(fm):
    (fused, vis, ir), _ = cached_case("smooth", 3, 45, 67)
    f, v, a = dev(fused, vis, ir)
    whole = fm.structural_stats(f, v, a)
    one = fm.structural_stats(f[1:2], v[1:2], a[1:2])
    for x, y in zip(bits(whole), bits(one)):
        assert np.array_equal(x[1], y[0])


def test_out_buffers_are_reused_and_sizes_are_checked(fm):
    a = dev(*cached_case("noise", 3, 45, 67)[0])
    b = dev(*cached_case("smooth", 3, 45, 67)[0])
    first = fm.structural_stats(*a)
    ptrs = [t.data_ptr() for t in first[:3]]
    second = fm.structural_stats(*b, out=first)
    fresh = fm.structural_stats(*b)
    assert [t.data_ptr() for t in second[:3]] == ptrs
    for x, y in zip(bits(second), bits(fresh)):
        assert np.array_equal(x, y)
    with pytest.raises(RuntimeError, match="out.qabf"):
        fm.structural_stats(*dev(*cached_case("noise", 2, 64, 96)[0]), out=first)
    with pytest.raises(RuntimeError, match="H, W >= 41"):
        fm.structural_stats(*dev(*make_inputs("noise", 1, 40, 64)))
    with pytest.raises(RuntimeError, match="expects"):
        fm.structural_stats(a[0], a[1], a[2][:, :, :-1])


def test_statistics_inside_a_captured_graph(fm):
    """A captured call replayed equals the eager result bit for bit, also after the static inputs changed."""
    stat = [t.clone() for t in dev(*cached_case("smooth", 2, 64, 96)[0])]
    fm.structural_stats(*stat)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = fm.structural_stats(*stat)
    for kind in ("noise", "smooth"):
        new = dev(*cached_case(kind, 2, 64, 96)[0])
        for dst, src in zip(stat, new):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        eager = fm.structural_stats(*new)
        for x, y in zip(bits(st), bits(eager)):
            assert np.array_equal(x, y), kind


def test_device_ssim_matches_the_reference_record(fm, golden_dir):
    g = np.load(os.path.join(golden_dir, "structural_scores.npz"))
    for kind in ("smooth", "noise"):
        s = fm.structural_scores(fm.structural_stats(*dev(g[f"{kind}:fused"], g[f"{kind}:vis"], g[f"{kind}:ir"])))
        for name, rec in (("SSIM_ir", "ssim_ir"), ("SSIM_vis", "ssim_vis")):
            err = np.abs(s[name] - g[f"{kind}:{rec}"].astype(np.float64)).max()
            print(f"{name} {kind} against the reference record: {err:.3e} (gate {RECORD_ATOL:.0e})")
            assert err <= RECORD_ATOL, (kind, name, err)


# ---------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def nets(fm):
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def quantised_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "pair_b1_64x96.npz"))
    ir, vis, mask = (torch.from_numpy(g[k]).cuda() for k in ("ir", "vis", "mask"))
    q = lambda t: torch.from_numpy(np.uint8(255 * t.cpu().numpy())).cuda()
    return q(ir[:, 0]), q(vis.permute(0, 2, 3, 1)).contiguous(), q(mask[:, 0])


def test_evaluator_opt_in_on_the_golden_pair(nets, golden_dir):
    from segmif_amd.evaluate import Evaluator
    ir_u8, vis_u8, mask_u8 = quantised_golden(golden_dir)
    B = ir_u8.shape[0]
    ev = Evaluator(*nets, structural=True)
    fused_u8, _ = ev.update(ir_u8, vis_u8, mask_u8)
    res = ev.results()
    assert set(res["mean"]) == set(SCORES) | set(STRUCTURAL) and len(res["mean"]) == 11
    ref = ref_structural(fused_u8.cpu().numpy(), vis_u8.cpu().numpy(), ir_u8.cpu().numpy())
    var = ref["variances"]
    assert not ((var > 1e-12) & (var < 1e-2)).any()
    for k, rtol, atol in (("Qabf", QABF_RTOL, 0.0), ("SSIM", 0.0, SSIM_ATOL), ("VIF", VIF_RTOL, 0.0)):
        assert res[k].shape == (B,) and np.isfinite(ref[k]).all()
        err = (np.abs(res[k] - ref[k]) / (np.abs(ref[k]) if rtol else 1.0)).max()
        print(f"evaluator {k}: max {'relative' if rtol else 'absolute'} error {err:.3e} (gate {rtol or atol:.0e})")
        np.testing.assert_allclose(res[k], ref[k], rtol=rtol, atol=atol, err_msg=k)
        assert res["mean"][k] == pytest.approx(ref[k].mean(), rel=1e-6)
    plain = Evaluator(*nets)
    plain.update(ir_u8, vis_u8, mask_u8)
    res0 = plain.results()
    assert set(res0["mean"]) == set(SCORES) and not set(STRUCTURAL) & set(res0)
    for k in SCORES:
        assert np.array_equal(res0[k], res[k], equal_nan=True)


def test_evaluate_command_line_with_structural_scores(fm, tmp_path):
    """One run in a fresh child process on three 64 x 96 .npy pairs: the JSON carries the three extra lists of length 3 and
    eleven means, and the summary line names the three scores."""
    from _fusion_ref import luma
    for sub in ("ir", "vis", "mask"):
        os.makedirs(tmp_path / sub)
    for i in range(3):
        fused, vis, ir = make_inputs("smooth", 1, 64, 96, seed=20 + i)
        np.save(tmp_path / "ir" / f"{i:03d}.npy", ir[0])
        np.save(tmp_path / "vis" / f"{i:03d}.npy", vis[0])
        np.save(tmp_path / "mask" / f"{i:03d}.npy", luma(fused[0]).astype(np.uint8))
    cmd = [sys.executable, "-m", "segmif_amd.evaluate", "--ir", str(tmp_path / "ir"), "--vis", str(tmp_path / "vis"),
           "--mask", str(tmp_path / "mask"), "--out", str(tmp_path / "out"), "--backbone", "mit_b1", "--batch", "2",
           "--json", str(tmp_path / "res.json"), "--structural-scores"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    doc = json.load(open(tmp_path / "res.json"))
    assert all(len(doc[k]) == 3 for k in SCORES + STRUCTURAL)
    assert set(doc["mean"]) == set(SCORES) | set(STRUCTURAL)
    assert all(np.isfinite(doc[k]).all() for k in STRUCTURAL)
    summary = [l for l in r.stdout.splitlines() if l.startswith("[evaluate] EN ")]
    assert len(summary) == 1 and all(f"  {k} " in summary[0] for k in STRUCTURAL)
