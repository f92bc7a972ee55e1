"""GPU tests of the fusion-quality statistics (csrc/fusion_stats.hip), the scores built on them, the palette rendering,
PairForward(return_u8=True) and the Evaluator / its command line.  The numpy side (tests/_fusion_ref.py) is independent
of the package: the luma, the histograms and the definitions are written out there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import detweights as dw
from _fusion_ref import KINDS, SCORES, make_inputs, ref_scores, ref_stats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 2, 2), (3, 37, 53), (2, 480, 640), (64, 96, 128), (1, 1024, 1024)]
# ag: sqrtf is specified at <= 1 ulp of fp32 (2^-24 relative to a term), the halving is exact, the accumulation of <= 2^26
# non-negative terms in fp64 adds < 2^-26; 4 ulp of fp32 = 2^-21 bounds that with room.  Derived, not measured.
AG_RTOL = 2.0 ** -21


@pytest.fixture(scope="module")
def fm():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import fusion_metrics
    return fusion_metrics


def dev(*arrays):
    return tuple(torch.from_numpy(a).cuda() for a in arrays)


def host(st):
    return st.joint_fa.cpu().numpy(), st.joint_fv.cpu().numpy(), st.sums.cpu().numpy(), st.ag.cpu().numpy()


def assert_ag(got, ref, what):
    err = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    print(f"ag {what}: max relative error {err.max():.3e} (bound {AG_RTOL:.3e})")
    assert np.array_equal(got[ref == 0], ref[ref == 0]) and err.max() <= AG_RTOL, (what, err.max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_raw_statistics_are_exact(fm, kind, shape):
    """joint_fa, joint_fv and sums equal an independent numpy evaluation: integers, no tolerance.  ag within 2^-21 relative
    of a float64 numpy sum, and bit-identical run to run."""
    fused, vis, ir = make_inputs(kind, *shape)
    st = fm.fusion_stats(*dev(fused, vis, ir))
    jfa, jfv, sums, ag = host(st)
    rfa, rfv, rsums, rag = ref_stats(fused, vis, ir)
    assert jfa.dtype == np.int64 and sums.dtype == np.int64 and ag.dtype == np.float64 and st.shape == shape[1:]
    assert np.array_equal(jfa, rfa) and np.array_equal(jfv, rfv)
    assert np.array_equal(sums, rsums)
    assert_ag(ag, rag, f"{kind} {shape}")
    again = fm.fusion_stats(*dev(fused, vis, ir))
    assert np.array_equal(host(again)[3].view(np.int64), ag.view(np.int64))
    assert torch.equal(again.joint_fa, st.joint_fa) and torch.equal(again.sums, st.sums)


def test_out_buffers_are_reused_and_cleared_by_the_entry_point(fm):
    """out= only reuses buffers: a second call into buffers that hold another input's counts gives the plain result."""
    a = dev(*make_inputs("noise", 2, 37, 53, seed=1))
    b = dev(*make_inputs("smooth", 2, 37, 53, seed=2))
    first = fm.fusion_stats(*a)
    ptr = first.joint_fa.data_ptr()
    second = fm.fusion_stats(*b, out=first)
    fresh = fm.fusion_stats(*b)
    assert second.joint_fa.data_ptr() == ptr
    for x, y in zip(second[:4], fresh[:4]):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError, match="out.joint_fa"):
        fm.fusion_stats(*dev(*make_inputs("noise", 3, 37, 53)), out=first)


def test_accumulate_adds_to_what_the_buffers_hold(fm):
    """The C entry point with accumulate != 0: two calls sum; the pixel count and ag add up as the histograms do."""
    from segmif_amd import _lib
    lib = _lib.load()
    x, y = make_inputs("smooth", 2, 37, 53, seed=3), make_inputs("noise", 2, 37, 53, seed=4)
    st = fm.fusion_stats(*dev(*x))
    f, v, a = dev(*y)
    ws = torch.empty(lib.segmif_fusion_stats_workspace_bytes(2, 37, 53) // 8, dtype=torch.int64, device="cuda")
    code = lib.segmif_fusion_stats_u8(f.data_ptr(), v.data_ptr(), a.data_ptr(), st.joint_fa.data_ptr(), st.joint_fv.data_ptr(),
                                      st.sums.data_ptr(), st.ag.data_ptr(), ws.data_ptr(), 2, 37, 53, 1,
                                      torch.cuda.current_stream().cuda_stream)
    assert code == 0
    rx, ry = ref_stats(*x), ref_stats(*y)
    jfa, jfv, sums, ag = host(st)
    assert np.array_equal(jfa, rx[0] + ry[0]) and np.array_equal(jfv, rx[1] + ry[1]) and np.array_equal(sums, rx[2] + ry[2])
    assert_ag(ag, rx[3] + ry[3], "accumulated")


def test_statistics_inside_a_captured_graph(fm):
    """The pass allocates nothing the capture cannot hold and clears its outputs with memset nodes: replays on new inputs
    give the plain result each time."""
    stat = [t.clone() for t in dev(*make_inputs("smooth", 2, 96, 128, seed=5))]
    fm.fusion_stats(*stat)  # (warm-up: raises the kernel's LDS limit outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = fm.fusion_stats(*stat)
    for seed, kind in ((6, "noise"), (7, "smooth")):
        new = make_inputs(kind, 2, 96, 128, seed=seed)
        for dst, src in zip(stat, dev(*new)):
            dst.copy_(src)
        g.replay()
        rfa, rfv, rsums, rag = ref_stats(*new)
        jfa, jfv, sums, ag = host(st)
        assert np.array_equal(jfa, rfa) and np.array_equal(jfv, rfv) and np.array_equal(sums, rsums)
        assert_ag(ag, rag, f"graph replay {kind}")


def test_an_image_does_not_depend_on_its_batch(fm):
    """Row b of a batch of 64 equals the result of image b alone, bit for bit, for all four outputs."""
    fused, vis, ir = dev(*make_inputs("smooth", 64, 96, 128, seed=8))
    whole = fm.fusion_stats(fused, vis, ir)
    for b in range(64):
        one = fm.fusion_stats(fused[b:b + 1], vis[b:b + 1], ir[b:b + 1])
        assert torch.equal(one.joint_fa[0], whole.joint_fa[b]) and torch.equal(one.joint_fv[0], whole.joint_fv[b]), b
        assert torch.equal(one.sums[0], whole.sums[b]), b
        assert torch.equal(one.ag.view(torch.int64)[0], whole.ag.view(torch.int64)[b]), b


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_scores_against_numpy(fm, kind, shape):
    """fusion_scores of the device statistics against the float64 numpy evaluation of the definitions on the same uint8
    images: rtol 1e-12 (same integers, float64 on both sides, only the summation order differs), AG at the ag bound; NaN and
    inf in the same places."""
    fused, vis, ir = make_inputs(kind, *shape)
    got = fm.fusion_scores(fm.fusion_stats(*dev(fused, vis, ir)))
    ref = ref_scores(fused, vis, ir)
    assert sorted(got) == sorted(SCORES)
    for k in SCORES:
        g, r = got[k], ref[k]
        assert g.shape == (shape[0],) and g.dtype == np.float64
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r)), (k, g, r)
        ok = np.isfinite(r)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(r[ok] != 0, np.abs(g[ok] - r[ok]) / np.abs(r[ok]), np.abs(g[ok]))
        print(f"{k} {kind} {shape}: max relative error {err.max() if err.size else 0.0:.3e}")
        np.testing.assert_allclose(g[ok], r[ok], rtol=AG_RTOL if k == "AG" else 1e-12, atol=0, err_msg=f"{k} {kind} {shape}")


def test_palette(fm):
    """segmif_palette_u8 = palette[labels]; labels outside the palette (-1, 9, 255) are black; n not a multiple of the block."""
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 9, (3, 37, 53)).astype(np.int32)
    labels[0, 0, :6] = [-1, 9, 255, 8, 0, -2147483648]
    assert labels.size % 256 != 0
    ref = np.zeros(labels.shape + (3,), dtype=np.uint8)
    for cid in range(9):  # util/util.py:26-27
        ref[labels == cid] = fm.MFNET_PALETTE[cid]
    got = fm.colorize(torch.from_numpy(labels).cuda())
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)  # the largest palette, as a device tensor
    big = rng.integers(-3, 260, 1000).astype(np.int32)
    want = np.where(((big >= 0) & (big < 256))[:, None], pal[np.clip(big, 0, 255)], 0).astype(np.uint8)
    assert np.array_equal(fm.colorize(torch.from_numpy(big).cuda(), torch.from_numpy(pal).cuda()).cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def nets(fm):
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def golden_pair(golden_dir):
    g = np.load(os.path.join(golden_dir, "pair_b1_64x96.npz"))
    return tuple(torch.from_numpy(g[k]).cuda() for k in ("ir", "vis", "mask"))


def test_pair_forward_returns_the_uint8_image(nets, golden_dir):
    """return_u8: the third value de-quantises bit-equal to the float image of the same call, and both equal what
    PairForward(uint8_roundtrip=True) returns without the flag; labels equal."""
    from segmif_amd.pipeline import PairForward
    from segmif_amd.utils.metrics import dequantize_fused
    ir, vis, mask = golden_pair(golden_dir)
    fused0, labels0 = PairForward(*nets, uint8_roundtrip=True)(ir, vis, mask)
    out = PairForward(*nets, uint8_roundtrip=True, return_u8=True)(ir, vis, mask)
    assert len(out) == 3
    fused, labels, u8 = out
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (ir.shape[0], 64, 96, 3)
    assert torch.equal(dequantize_fused(u8), fused) and torch.equal(fused, fused0) and torch.equal(labels, labels0)
    pf = PairForward(*nets, uint8_roundtrip=True, return_u8=True).capture(ir, vis, mask)
    fused_g, labels_g, u8_g = pf(ir, vis, mask)
    assert torch.equal(dequantize_fused(u8_g), fused_g) and torch.equal(u8_g, u8) and torch.equal(labels_g, labels0)


def quantised_golden(golden_dir):
    ir, vis, mask = golden_pair(golden_dir)
    q = lambda t: torch.from_numpy(np.uint8(255 * t.cpu().numpy())).cuda()
    return q(ir[:, 0]), q(vis.permute(0, 2, 3, 1)).contiguous(), q(mask[:, 0])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_evaluator_on_the_golden_pair(nets, golden_dir, graph):
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.pipeline import PairForward
    from segmif_amd.utils.metrics import compute_results, dequantize_fused
    ir_u8, vis_u8, mask_u8 = quantised_golden(golden_dir)
    B = ir_u8.shape[0]
    label = dw.det_labels("evaluator_gt", (B, 64, 96), 9)
    ev = Evaluator(*nets, graph=graph)
    for _ in range(2):  # two batches: the confusion matrix accumulates, the graph is replayed
        fused_u8, labels = ev.update(ir_u8, vis_u8, mask_u8, label=label.cuda())
    assert fused_u8.dtype == torch.uint8 and fused_u8.is_cuda and labels.dtype == torch.int32 and labels.is_cuda
    ir = dequantize_fused(ir_u8.unsqueeze(3).contiguous())
    vis = dequantize_fused(vis_u8)
    mask3 = dequantize_fused(mask_u8.unsqueeze(3).contiguous()).repeat(1, 3, 1, 1)
    _, labels_h, u8_h = PairForward(*nets, uint8_roundtrip=True, return_u8=True)(ir, vis, mask3)
    assert torch.equal(fused_u8, u8_h) and torch.equal(labels, labels_h)
    res = ev.results()
    conf = np.zeros((9, 9), dtype=np.int64)
    np.add.at(conf, (label.numpy().ravel(), labels.cpu().numpy().ravel().astype(np.int64)), 2)
    iou = compute_results(conf)[2]
    assert np.array_equal(np.nan_to_num(res["iou"]), np.nan_to_num(iou)) and res["mIoU"] == float(np.mean(np.nan_to_num(iou)))
    ref = ref_scores(fused_u8.cpu().numpy(), vis_u8.cpu().numpy(), ir_u8.cpu().numpy())
    for k in SCORES:
        assert res[k].shape == (2 * B,)
        np.testing.assert_allclose(res[k], np.tile(ref[k], 2), rtol=AG_RTOL if k == "AG" else 1e-12, atol=0, err_msg=k)
        assert res["mean"][k] == pytest.approx(ref[k].mean(), rel=AG_RTOL if k == "AG" else 1e-11)


def test_evaluate_command_line(fm, tmp_path):
    """One run in a fresh child process on three .npy pairs: three fused files, three palette files and a JSON with the eight
    scores; without checkpoints it says that it runs on seeded weights."""
    rng = np.random.default_rng(10)
    for sub in ("ir", "vis", "mask", "label"):
        os.makedirs(tmp_path / sub)
    for i in range(3):
        fused, vis, ir = make_inputs("smooth", 1, 64, 96, seed=20 + i)
        np.save(tmp_path / "ir" / f"{i:03d}.npy", ir[0])
        np.save(tmp_path / "vis" / f"{i:03d}.npy", vis[0])
        np.save(tmp_path / "mask" / f"{i:03d}.npy", luma_u8(fused[0]))
        np.save(tmp_path / "label" / f"{i:03d}.npy", rng.integers(0, 9, (64, 96)).astype(np.uint8))
    cmd = [sys.executable, "-m", "segmif_amd.evaluate", "--ir", str(tmp_path / "ir"), "--vis", str(tmp_path / "vis"),
           "--mask", str(tmp_path / "mask"), "--label", str(tmp_path / "label"), "--out", str(tmp_path / "out"),
           "--backbone", "mit_b1", "--batch", "2", "--json", str(tmp_path / "res.json")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SEEDED RANDOM weights" in r.stdout
    for i in range(3):
        fused = np.load(tmp_path / "out" / "Fused" / f"{i:03d}.npy")
        seg = np.load(tmp_path / "out" / "Seg" / f"{i:03d}.npy")
        assert fused.shape == (64, 96, 3) and fused.dtype == np.uint8 and seg.shape == (64, 96, 3) and seg.dtype == np.uint8
        colours = {tuple(c) for c in seg.reshape(-1, 3)}
        assert colours <= {tuple(c) for c in fm.MFNET_PALETTE}
    doc = json.load(open(tmp_path / "res.json"))
    assert doc["names"] == ["000.npy", "001.npy", "002.npy"] and set(SCORES) <= set(doc) and "mIoU" in doc
    assert all(len(doc[k]) == 3 for k in SCORES) and set(doc["mean"]) == set(SCORES)


def luma_u8(rgb):
    from _fusion_ref import luma
    return luma(rgb).astype(np.uint8)
