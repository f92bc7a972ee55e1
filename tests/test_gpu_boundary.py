"""GPU tests of the contour statistics (csrc/boundary_stats.hip): the int64 tables of utils/metrics.boundary_stats against the
brute-force numpy restatement (tests/_boundary_ref.py), always as exact equality; batching, repeatability, zeroing, out=, the
refusals in Python and in the C entry point; the Evaluator's and the command line's opt-in paths.

The kernel works on BOUNDARY_TILE x BOUNDARY_TILE = 64 x 64 output tiles with a halo of max(d, theta + 1) <= 32.  Shapes: odd
sizes with W % 4 != 0; two tiles plus one pixel each way (129 x 129); a window larger than the frame; the largest widths;
theta = 0; K = 1, 9 and 32.  Every case but the 9 x 12 one holds the label values 255, -1, 256 and 2^40 + 3 and predictions of
-1 and K on valid pixels (asserted); the 9 x 12 one holds some ignored labels.

So that no comparison passes on empty tables, the restatement's own tables must show (`vacuity`): the ground truth's band holds
between 10 % and 90 % of the valid pixels; at least two classes have 0 < band_inter < min(g_band, p_band) and 0 < p_matched <
p_contour; an off-diagonal trimap entry is non-zero.  Three cases cannot meet all of that by construction and state what they
meet instead: a window larger than the frame puts EVERY valid pixel into the band; at d = 32 in an 80 x 96 frame only the
16 x 32 centre can have its 65 x 65 window inside the frame, so the band holds at least 93 % (the other conditions are asked
of one class); with K = 1 there is one class, no class confusion, and the band comes from the ignored regions and the
frame's border."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _boundary_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64  # asserted equal to utils/metrics.BOUNDARY_TILE (and by tests/test_boundary_host.py to the header's) below

#        name            B  H             W             K   d   theta seed  vacuity
CASES = {"odd":         (2, 37,           53,           9,  3,  2,    11,   "full"),
         "two_tiles_1": (1, 2 * TILE + 1, 2 * TILE + 1, 9,  5,  3,    2,    "full"),
         "window>frame": (1, 9,           12,           9,  8,  2,    3,    "all_band"),
         "widest":      (1, 80,           96,           9,  32, 31,   4,    "one_class"),
         "theta0":      (1, 37,           53,           9,  3,  0,    5,    "full"),
         "K1":          (1, 37,           53,           1,  3,  2,    6,    "K1"),
         "K32":         (1, 40,           70,           32, 2,  1,    7,    "full")}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> pred, label, cls, trimap of the restatement (read-only, computed once and shared)"""
    B, H, W, K, d, theta, seed, _ = CASES[name]
    pred, label = ref.synthetic(B, H, W, K, d, seed)
    cls, tri = ref.boundary_stats(pred, label, K, d, theta)
    for a in (pred, label, cls, tri):
        a.setflags(write=False)
    return pred, label, cls, tri


@pytest.fixture(scope="module")
def metrics():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import metrics as m
    assert m.BOUNDARY_TILE == TILE
    return m


def dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


def host(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def check_vacuity(name):
    B, H, W, K, d, theta, seed, kind = CASES[name]
    pred, label, cls, tri = case(name)
    valid = int(((label >= 0) & (label < K)).sum())
    c, t = cls.sum(axis=0), tri.sum(axis=0)
    frac = c[:, 0].sum() / valid
    inter = int(((c[:, 2] > 0) & (c[:, 2] < np.minimum(c[:, 0], c[:, 1]))).sum())
    match = int(((c[:, 6] > 0) & (c[:, 6] < c[:, 4])).sum())
    off = int(t.sum() - np.trace(t))
    print(f"{name}: band {frac:.3f} of {valid} valid pixels, {inter} classes with a partial band overlap, {match} with partial "
          f"matches, {off} off-diagonal trimap pixels")
    assert 0 < valid < label.size
    if kind != "all_band":  # (9 x 12 pixels are too few to be sure of every special value)
        assert (label == 255).any() and (label == -1).any() and (label == 256).any() and (label == 2 ** 40 + 3).any()
        assert ((pred == -1) & (label >= 0) & (label < K)).any() and ((pred == K) & (label >= 0) & (label < K)).any()
    if kind == "full":
        assert 0.10 <= frac <= 0.90 and inter >= 2 and match >= 2 and off > 0
    elif kind == "all_band":
        assert c[:, 0].sum() == valid and c[:, 1].sum() > 0
    elif kind == "one_class":
        assert 0.93 <= frac and inter >= 1 and match >= 1 and off > 0
    else:
        assert 0.10 <= frac <= 0.90 and 0 < c[0, 2] < min(c[0, 0], c[0, 1]) and 0 < c[0, 4]


@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_the_restatement(metrics, name):
    B, H, W, K, d, theta, _, _ = CASES[name]
    check_vacuity(name)
    pred, label, cls, tri = case(name)
    got_cls, got_tri = metrics.boundary_stats(*dev(pred, label), n_class=K, d=d, theta=theta)
    assert got_cls.dtype == torch.int64 and got_tri.dtype == torch.int64
    assert tuple(got_cls.shape) == (B, K, 8) and tuple(got_tri.shape) == (B, K, K)
    got_cls, got_tri = host(got_cls, got_tri)
    for i, col in enumerate(ref.COLUMNS):
        assert np.array_equal(got_cls[:, :, i], cls[:, :, i]), (name, col, got_cls[:, :, i], cls[:, :, i])
    assert np.array_equal(got_tri, tri), name


def test_predictions_on_ignored_pixels_do_not_matter(metrics):
    B, H, W, K, d, theta, _, _ = CASES["odd"]
    pred, label, cls, tri = case("odd")
    other = np.array(pred)
    ignored = ~((label >= 0) & (label < K))
    other[ignored] = np.random.default_rng(0).integers(-3, K + 3, int(ignored.sum()))
    assert (other != pred).any()
    got = host(*metrics.boundary_stats(*dev(other, label), n_class=K, d=d, theta=theta))
    assert np.array_equal(got[0], cls) and np.array_equal(got[1], tri)


def test_frames_are_independent_and_calls_repeat(metrics):
    B, H, W, K, d, theta, _, _ = CASES["odd"]
    pred, label, cls, tri = case("odd")
    p, l = dev(pred, label)
    first = host(*metrics.boundary_stats(p, l, n_class=K, d=d, theta=theta))
    again = host(*metrics.boundary_stats(p, l, n_class=K, d=d, theta=theta))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    for b in range(B):
        alone = host(*metrics.boundary_stats(p[b:b + 1], l[b:b + 1], n_class=K, d=d, theta=theta))  # (frame 1: an unaligned slice)
        assert np.array_equal(alone[0][0], cls[b]) and np.array_equal(alone[1][0], tri[b])


def test_the_call_zeroes_its_outputs(metrics):
    from segmif_amd import _lib
    B, H, W, K, d, theta, _, _ = CASES["odd"]
    pred, label, cls, tri = case("odd")
    p, l = dev(pred, label)
    out_cls = torch.full((B, K, 8), 12345, device="cuda", dtype=torch.int64)
    out_tri = torch.full((B, K, K), -7, device="cuda", dtype=torch.int64)
    rc = _lib.load().segmif_boundary_stats_i32(p.data_ptr(), l.data_ptr(), B, H, W, K, d, theta, out_cls.data_ptr(), out_tri.data_ptr(),
                                               metrics._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out_cls.cpu().numpy(), cls) and np.array_equal(out_tri.cpu().numpy(), tri)


def test_out_accumulates_two_batches(metrics):
    B, H, W, K, d, theta, _, _ = CASES["odd"]
    pred, label, cls, tri = case("odd")
    pred1, label1, cls1, tri1 = case("theta0")  # the same frame size; here run with the first case's widths
    cls1, tri1 = ref.boundary_stats(pred1, label1, K, d, theta)
    total = (torch.zeros((K, 8), device="cuda", dtype=torch.int64), torch.zeros((K, K), device="cuda", dtype=torch.int64))
    metrics.boundary_stats(*dev(pred, label), n_class=K, d=d, theta=theta, out=total)
    metrics.boundary_stats(*dev(pred1, label1), n_class=K, d=d, theta=theta, out=total)
    assert np.array_equal(total[0].cpu().numpy(), cls.sum(axis=0) + cls1.sum(axis=0))
    assert np.array_equal(total[1].cpu().numpy(), tri.sum(axis=0) + tri1.sum(axis=0))
    with pytest.raises(RuntimeError, match="out must be"):
        metrics.boundary_stats(*dev(pred, label), n_class=K, d=d, theta=theta, out=(total[1], total[0]))


def test_default_widths_follow_the_frame(metrics):
    """d = None, theta = None: boundary_widths(37, 53) = (1, 0)"""
    B, H, W, K, _, _, _, _ = CASES["odd"]
    pred, label, _, _ = case("odd")
    assert metrics.boundary_widths(H, W) == (1, 0)
    got = host(*metrics.boundary_stats(*dev(pred, label), n_class=K))
    want = ref.boundary_stats(pred, label, K, 1, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_python_refusals(metrics):
    pred, label, _, _ = case("odd")
    p, l = dev(pred, label)
    with pytest.raises(RuntimeError, match="contiguous"):
        metrics.boundary_stats(p.transpose(1, 2), l.transpose(1, 2).contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        metrics.boundary_stats(p, torch.zeros((2, 37, 56), device="cuda", dtype=torch.int64)[:, :, :53])  # (a pitched view)
    with pytest.raises(RuntimeError, match="int32"):
        metrics.boundary_stats(p.long(), l)
    with pytest.raises(RuntimeError, match="int64"):
        metrics.boundary_stats(p, l.int())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.boundary_stats(p.cpu(), l.cpu())
    with pytest.raises(RuntimeError, match="pred is"):
        metrics.boundary_stats(p[:, :-1].contiguous(), l)
    with pytest.raises(ValueError, match=r"37 x 53 .* d = 33.*pass d="):
        metrics.boundary_stats(p, l, d=33)
    with pytest.raises(ValueError, match=r"37 x 53 .* d = 0.*pass d="):
        metrics.boundary_stats(p, l, d=0)
    with pytest.raises(ValueError, match=r"37 x 53 .* theta = 32.*pass theta="):
        metrics.boundary_stats(p, l, theta=32)
    big = torch.zeros((1, 2160, 3840), device="cuda", dtype=torch.int32)  # the diagonal gives d = 88
    with pytest.raises(ValueError, match=r"2160 x 3840 .* d = 88.*pass d="):
        metrics.boundary_stats(big, big.long())


def test_entry_point_rejections(metrics):
    from segmif_amd import _lib
    lib = _lib.load()
    B, H, W, K, d, theta, _, _ = CASES["odd"]
    pred, label, _, _ = case("odd")
    p, l = dev(pred, label)
    cls = torch.zeros((B, K, 8), device="cuda", dtype=torch.int64)
    tri = torch.zeros((B, 32, 32), device="cuda", dtype=torch.int64)
    good = dict(pred=p.data_ptr(), label=l.data_ptr(), B=B, H=H, W=W, K=K, d=d, theta=theta, cls=cls.data_ptr(), trimap=tri.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.segmif_boundary_stats_i32(a["pred"], a["label"], a["B"], a["H"], a["W"], a["K"], a["d"], a["theta"], a["cls"], a["trimap"],
                                             metrics._stream())

    assert call() == 0
    bad = [dict(pred=None), dict(label=None), dict(cls=None), dict(trimap=None), dict(B=0), dict(H=0), dict(W=0), dict(B=-1),
           dict(K=0), dict(K=33), dict(d=0), dict(d=33), dict(d=-1), dict(theta=-1), dict(theta=32),
           dict(cls=cls.data_ptr() + 4), dict(trimap=tri.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == -22, kw
    assert call(K=32, d=32, theta=31, cls=torch.zeros((B, 32, 8), device="cuda", dtype=torch.int64).data_ptr()) == 0
    torch.cuda.synchronize()


# ---- through the Evaluator and the command line -------------------------------------------------------------------------------

EH, EW = 48, 64
PLAIN_KEYS = {"EN", "SD", "SF", "AG", "MI", "SCD", "CC", "PSNR", "mean", "precision", "recall", "iou", "mIoU"}


@pytest.fixture(scope="module")
def nets(metrics):
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def frames(seed, B):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:EH, 0:EW]
    ir = np.stack([np.uint8(127 + 100 * np.sin(yy / (3.0 + b) + seed) * np.cos(xx / 5.0)) for b in range(B)])
    vis = np.stack([np.stack([np.uint8(rng.integers(0, 40) + 2 * xx + yy), np.uint8(3 * yy + b), np.uint8(255 - 2 * xx)], axis=-1) for b in range(B)])
    mask = np.uint8((ir.astype(np.int32) + vis[..., 0]) // 2)
    _, label = ref.synthetic(B, EH, EW, 9, 2, seed)
    return ir, vis, mask, label


@pytest.mark.parametrize("mode", ["eager", "graph", "tta"])
def test_evaluator_accumulates_the_tables(metrics, nets, mode):
    """three batches: the scores equal boundary_scores of the restatement's summed tables on the labels the evaluator returned,
    to float64 equality; without boundary= the result has the keys and values it always had"""
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.tta import TTA
    kw = {"eager": {}, "graph": {"graph": True}, "tta": {"tta": TTA((1.0,), True, 8)}}[mode]
    ev, plain = Evaluator(*nets, boundary={}, **kw), Evaluator(*nets, **kw)
    d, theta = metrics.boundary_widths(EH, EW)
    assert (d, theta) == (2, 1)
    cls, tri = np.zeros((9, 8), dtype=np.int64), np.zeros((9, 9), dtype=np.int64)
    conf = np.zeros((9, 9), dtype=np.int64)
    for i in range(3):
        ir, vis, mask, label = frames(40 + i, 2)
        args = dev(ir, vis, mask, label)
        _, labels = ev.update(*args)
        plain.update(*args)
        pred = labels.cpu().numpy()
        assert pred.dtype == np.int32 and pred.shape == label.shape
        c, t = ref.boundary_stats(pred, label, 9, d, theta)
        cls += c.sum(axis=0)
        tri += t.sum(axis=0)
        ok = (label >= 0) & (label < 9)
        np.add.at(conf, (label[ok], pred[ok]), 1)
    assert cls[:, 0].sum() > 0
    res, res0 = ev.results(), plain.results()
    want = metrics.boundary_scores(cls, tri)
    for k in metrics.BOUNDARY_SCORE_NAMES:
        assert np.array_equal(np.asarray(res[k]), np.asarray(want[k]), equal_nan=True), (k, res[k], want[k])
    assert set(res0) == PLAIN_KEYS and set(res) == PLAIN_KEYS | set(metrics.BOUNDARY_SCORE_NAMES)
    for k in PLAIN_KEYS - {"mean"}:
        assert np.array_equal(np.asarray(res0[k]), np.asarray(res[k]), equal_nan=True), k
    assert res0["mean"] == res["mean"]
    assert np.array_equal(res0["iou"], metrics.compute_results(conf)[2], equal_nan=True)
    doc, doc0 = ev.document(["x"] * 6, []), plain.document(["x"] * 6, [])
    assert doc["boundary"] == {"d": 2, "theta": 1, "frame": [EH, EW]} and "boundary" not in doc0
    json.dumps(doc)
    if mode == "eager":
        small = dev(*(a[:, :40, :56].copy() for a in frames(50, 1)))
        with pytest.raises(RuntimeError, match="mix bands"):
            ev.update(*small)


def test_evaluate_command_line(metrics, tmp_path):
    """two runs in fresh child processes on three 48 x 64 .npy frames: with --boundary-scores the JSON carries the scores and the
    widths and the summary line names the three means; without it neither has any of them"""
    for sub in ("ir", "vis", "mask", "label"):
        os.makedirs(tmp_path / sub)
    ir, vis, mask, label = frames(60, 3)
    for i in range(3):
        for sub, a in (("ir", ir), ("vis", vis), ("mask", mask), ("label", label)):
            np.save(tmp_path / sub / f"{i:03d}.npy", a[i])
    docs = {}
    for flag in (True, False):
        path = tmp_path / f"res{int(flag)}.json"
        cmd = [sys.executable, "-m", "segmif_amd.evaluate", "--ir", str(tmp_path / "ir"), "--vis", str(tmp_path / "vis"),
               "--mask", str(tmp_path / "mask"), "--label", str(tmp_path / "label"), "--out", str(tmp_path / "out"), "--backbone", "mit_b1",
               "--batch", "2", "--json", str(path)] + (["--boundary-scores", "--bf-tolerance", "2"] if flag else [])
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        docs[flag] = json.load(open(path))
        summary = [l for l in r.stdout.splitlines() if l.startswith("[evaluate] EN ")]
        assert len(summary) == 1 and "  mIoU " in summary[0]
        assert all((f"  {k} " in summary[0]) == flag for k in ("mBIoU", "trimap", "mBF"))
    new = set(metrics.BOUNDARY_SCORE_NAMES) | {"boundary"}
    assert new <= set(docs[True]) and not new & set(docs[False]) and set(docs[True]) - new == set(docs[False])
    assert docs[True]["boundary"] == {"d": 2, "theta": 2, "frame": [EH, EW]}
    assert len(docs[True]["boundary_iou"]) == 9 and 0.0 <= docs[True]["mBIoU"] <= 1.0
    assert docs[True]["mIoU"] == docs[False]["mIoU"] and docs[True]["mean"] == docs[False]["mean"]
