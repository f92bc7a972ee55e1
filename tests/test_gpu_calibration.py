"""GPU tests of the calibration statistics (csrc/calibration_stats.hip, include/segmif_calib.h, utils/calibration.py) and of what
reads them: SelfTrainingStep(teacher_temperature=), PairForward(return_logits=), Evaluator(calibration=).  The seeded cases are
tests/_calibration_ref.py's (tests/test_calibration_host.py vets them on the CPU); every case runs in well under a second.

Gates.  conf, and the sums of NLL and Brier score relative to their size, against the float64 restatement: 4 x the error of
torch's own float32 evaluation of the same formulas on the same inputs (F.interpolate, exp, sum, log on the device), with a floor of
4 * 2^-23 - the gate of the neighbouring features.  The integer tables: exact equality with a numpy binning of the kernel's own
conf and pred; against the restatement's float64 tables after leaving out the pixels within 1e-5 of an edge or threshold or with
a top-2 gap below 1e-4 (at most 1 % of the valid pixels, asserted for the restatement alone on the CPU)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _calibration_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

FLOOR = 4 * 2.0 ** -23
NAMES = sorted(ref.CASES)


@pytest.fixture(scope="module")
def cal():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import calibration as c
    return c


def place(x, layout):
    """the case's logits on the device: dense, a pitched view (pitch 12 > C = 9) or a view that starts 4 bytes off a 16-byte boundary"""
    t = torch.from_numpy(x).cuda()
    if layout == "pitched":
        big = torch.full(x.shape[:3] + (12,), 7.0, device="cuda")
        big[..., :x.shape[3]] = t
        t = big[..., :x.shape[3]]
        assert t.stride(2) == 12
    elif layout == "misaligned":
        flat = torch.zeros(x.size + 1, device="cuda")
        flat[1:] = t.reshape(-1)
        t = flat[1:].view(x.shape)
        assert t.data_ptr() % 16 == 4
    return t


_RUNS = {}


def run(cal, name):
    """one case, computed once and shared: the kernel's table with conf and pred, the restatement's pixels"""
    if name not in _RUNS:
        c = ref.make_case(name)
        x, label = place(c["x"], c["layout"]), torch.from_numpy(c["label"]).cuda()
        table = cal.calibration_stats(x, label, c["temperatures"], c["edges"], c["thresholds"], return_conf=True)
        got = {k: getattr(table, k).cpu().numpy() for k in ("counts", "above", "totals", "sums", "conf", "pred")}
        _RUNS[name] = (c, x, label, got, ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"]))
    return _RUNS[name]


def torch_float32(c, x):
    """torch's own float32 evaluation of the rule's formulas on the device -> conf, nll, brier (NT, B, OH, OW) as float64 arrays"""
    v = F.interpolate(x.permute(0, 3, 1, 2), size=(c["OH"], c["OW"]), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    C = v.shape[-1]
    y = torch.from_numpy(np.where((c["label"] >= 0) & (c["label"] < C), c["label"], 0)).cuda()
    vmax = v.max(dim=-1).values
    vy = v.gather(-1, y[..., None])[..., 0]
    onehot = F.one_hot(y, C).float()
    out = []
    for T in c["temperatures"]:
        r = float(np.float32(1) / np.float32(T))
        e = torch.exp((v - vmax[..., None]) * r)
        s = e.sum(dim=-1)
        out.append((1.0 / s, torch.log(s) - (vy - vmax) * r, ((e / s[..., None] - onehot) ** 2).sum(dim=-1)))
    return [torch.stack([o[i] for o in out]).double().cpu().numpy() for i in range(3)]


@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_a_binning_of_the_kernels_own_values(cal, name):
    """check 1: counts, above and totals as integers - conf_q through conf * 2^32 too"""
    c, _, _, got, p = run(cal, name)
    conf, pred = got["conf"], got["pred"]
    valid = pred >= 0
    assert np.array_equal(np.isnan(conf), np.broadcast_to(~valid, conf.shape)) and conf.dtype == np.float32 and pred.dtype == np.int32
    C = c["x"].shape[3]
    labelled = (c["label"] >= 0) & (c["label"] < C)
    assert got["totals"].tolist() == [int(valid.sum()), int((~labelled).sum()), int((labelled & ~valid).sum())]
    assert got["totals"].tolist() == [int(p["valid"].sum()), int(p["ignored"].sum()), int(p["nonfinite"].sum())] and np.array_equal(valid, p["valid"])
    correct = valid & (pred == np.where(labelled, c["label"], -2))
    counts, above = ref.tables(np.where(valid, conf, 0).astype(np.float32), correct, np.broadcast_to(valid, conf.shape), c["edges"], c["thresholds"],
                               exact_q=True)
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["above"], above)
    assert got["counts"][:, :, 0].sum(axis=1).tolist() == [int(valid.sum())] * len(c["temperatures"])
    if name == "one_pixel":  # conf is 1, NLL and Brier are 0 and everything lands in the last bin
        assert conf.tolist() == [[[[1.0]]]] and got["sums"].tolist() == [[0.0, 0.0]]
        assert got["counts"][0, -1].tolist() == [1, 1, 2 ** 32] and got["counts"][0, :-1].sum() == 0 and got["above"].tolist() == [[[1, 1]]]
    if name == "small":
        assert len(c["temperatures"]) == 16 and len(c["thresholds"]) == 8 and got["totals"][1] >= 4
    if name == "nonfinite":
        assert got["totals"][2] > 0


@pytest.mark.parametrize("name", NAMES)
def test_pred_and_conf_against_the_neighbouring_kernels(cal, name):
    """check 2: pred is bilinear_argmax's and the float64 argmax wherever the float64 top-2 gap is at least 1e-4; at T = 1 conf is
    pseudo_label's by value, within the one gate that holds conf to the restatement"""
    from segmif_amd import ops
    c, x, _, got, p = run(cal, name)
    clear = p["valid"] & (p["gap"] >= 1e-4)
    assert clear.sum() >= 0.99 * p["valid"].sum()
    arg = ops.bilinear_argmax(x.nan_to_num(0.0, 0.0, 0.0) if name == "nonfinite" else x, c["OH"], c["OW"]).cpu().numpy()
    assert np.array_equal(got["pred"][clear], arg[clear]) and np.array_equal(got["pred"][clear], p["pred"][clear])
    if 1.0 in c["temperatures"] and name != "nonfinite":
        t = c["temperatures"].index(1.0)
        theirs = ops.pseudo_label(x, c["OH"], c["OW"], return_conf=True)[2].cpu().numpy().astype(np.float64)
        tc = torch_float32(c, x)[0][t]
        gate = max(4 * float(np.abs(tc - p["conf"][t])[p["valid"]].max()), FLOOR)
        worst = float(np.abs(theirs - got["conf"][t])[p["valid"]].max())
        print(f"{name}: conf against pseudo_label's: {worst:.3e} (gate: {gate:.3e})")
        assert worst <= gate


@pytest.mark.parametrize("name", NAMES)
def test_values_against_the_restatement(cal, name):
    """check 3; the largest errors observed on an MI355X are in the README's calibration paragraph"""
    c, x, _, got, p = run(cal, name)
    clean = x.nan_to_num(0.0, 0.0, 0.0) if name == "nonfinite" else x
    tc, tn, tb = torch_float32(c, clean)
    v = p["valid"]
    err = float(np.abs(got["conf"].astype(np.float64) - p["conf"])[:, v].max())
    gate = max(4 * float(np.abs(tc - p["conf"])[:, v].max()), FLOOR)
    print(f"{name}: conf error {err:.3e}, gate {gate:.3e}")
    assert err <= gate
    for j, (what, theirs) in enumerate((("nll", tn), ("brier", tb))):
        for t in range(len(c["temperatures"])):
            want = float(p[what][t][v].sum())
            e = abs(float(got["sums"][t, j]) - want)
            g = max(4 * abs(float(theirs[t][v].sum()) - want), FLOOR * abs(want))
            print(f"{name}: sum of {what} at T {c['temperatures'][t]:.4g}: {want:.6f}, error {e:.3e} ({e / max(abs(want), 1e-300):.3e} of it), gate {g:.3e}")
            assert e <= g


@pytest.mark.parametrize("name", NAMES)
def test_tables_against_the_restatements_tables(cal, name):
    """check 4: on the pixels that keep their distance from every edge, threshold and tie, n, correct and the counts above the
    thresholds are the float64 evaluation's; the confidence sums agree to the conf gate per pixel"""
    c, x, _, got, p = run(cal, name)
    keep = ref.stable(p, c["edges"], c["thresholds"])
    valid = int(p["valid"].sum())
    assert all(valid - int(k.sum()) <= 0.01 * valid for k in keep)
    want_counts, want_above = ref.tables(p["conf"], p["correct"], keep, c["edges"], c["thresholds"], exact_q=False)
    correct = (got["pred"] >= 0) & (got["pred"] == c["label"])
    counts, above = ref.tables(np.nan_to_num(got["conf"]).astype(np.float32), correct, keep, c["edges"], c["thresholds"], exact_q=True)
    assert np.array_equal(counts[:, :, :2], want_counts[:, :, :2]) and np.array_equal(above, want_above)
    tc = torch_float32(c, x.nan_to_num(0.0, 0.0, 0.0) if name == "nonfinite" else x)[0]
    gate = max(4 * float(np.abs(tc - p["conf"])[:, p["valid"]].max()), FLOOR)
    assert (np.abs(counts[:, :, 2] - want_counts[:, :, 2]) <= (gate * 2.0 ** 32) * counts[:, :, 0] + 1).all()


@pytest.mark.parametrize("name", ["small", "c32", "columns_plus_one"])
def test_runs_are_bit_identical_and_tables_add_up(cal, name):
    """check 5"""
    c, x, label, got, _ = run(cal, name)
    kw = dict(temperatures=c["temperatures"], edges=c["edges"], thresholds=c["thresholds"])
    again = cal.calibration_stats(x, label, return_conf=True, **kw)
    for k in ("counts", "above", "totals"):
        assert np.array_equal(getattr(again, k).cpu().numpy(), got[k]), k
    for k in ("sums", "conf"):
        assert np.array_equal(getattr(again, k).cpu().numpy().view(np.int64 if k == "sums" else np.int32), got[k].view(np.int64 if k == "sums" else np.int32)), k
    twice = cal.calibration_stats(x, label, out=cal.calibration_stats(x, label, **kw), **kw)
    for k in ("counts", "above", "totals"):
        assert np.array_equal(getattr(twice, k).cpu().numpy(), 2 * got[k]), k
    assert np.array_equal(twice.sums.cpu().numpy(), got["sums"] + got["sums"])  # (S + S is exact)
    with pytest.raises(ValueError, match="same temperatures"):
        cal.calibration_stats(x, label, out=twice, temperatures=(3.0,), edges=c["edges"], thresholds=c["thresholds"])
    if x.shape[0] > 1:  # a sample alone gives the integer tables of its share
        parts = [cal.calibration_stats(x[b:b + 1], label[b:b + 1].contiguous(), **kw) for b in range(x.shape[0])]
        for k in ("counts", "above", "totals"):
            assert np.array_equal(sum(getattr(t, k).cpu().numpy() for t in parts), got[k]), k


def test_scores_and_the_grid_fit(cal):
    """calibration_scores of a device table is the scores of its arrays; fit_temperature's answer has the lowest NLL of its grids and
    lies inside [lo, hi]"""
    c, x, label, got, p = run(cal, "small")
    table = cal.calibration_stats(x, label, c["temperatures"], c["edges"], c["thresholds"])
    s = cal.calibration_scores(table)
    N = int(p["valid"].sum())
    assert s["calibration_pixels"]["valid"] == N and np.array_equal(s["reliability_n"], got["counts"][:, :, 0])
    for t in range(len(c["temperatures"])):
        assert s["ece"][t] == pytest.approx(ref.ece(got["counts"][t], N), rel=1e-12)
        assert s["nll"][t] == got["sums"][t, 0] / N and s["accuracy"][t] == got["counts"][t, :, 1].sum() / N
    assert s["best"]["index"] == int(np.argmin(got["sums"][:, 0]))
    fit = cal.fit_temperature(x, label, lo=0.25, hi=8, passes=3)
    assert len(fit["passes"]) == 3 and 0.25 <= fit["temperature"] <= 8 and fit["nll"] == min(min(p["nll"]) for p in fit["passes"])
    assert any(fit["temperature"] in p["grid"] for p in fit["passes"]) and all(len(p["grid"]) == 16 for p in fit["passes"])
    # the last grid's points differ by a factor 32 ** ((2 / 15) ** 2 / 15) = 1.004: a list point cannot beat the fit by more than the NLL's
    # curvature over half of that
    assert fit["nll"] <= s["best"]["nll"] * (1 + 1e-3)
    with pytest.raises(ValueError, match="no valid pixel"):
        cal.fit_temperature(x, torch.full_like(label, 255))


# ---- self-training ----------------------------------------------------------------------------------------------------------------------------

B, H, W = 2, 64, 64


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def _st_setup():
    import segmif_amd.core as core
    net = core.Network3("mit_b1", 9, pretrained=None)
    dw.load_det_weights(net, seed=0)
    net = net.cuda().eval()
    xs = [dw.det_input(f"cal_x{t}", (B, 3, H, W)).cuda() for t in "LU"]
    y = dw.det_labels("cal_y", (B, H, W), 9)
    y[:, 3:9, 10:30] = 255
    return net, xs[0], y.cuda(), xs[1]


def test_self_training_temperature(cal):
    """check 6: teacher_temperature=1.0 gives the bits of the step without the argument; 2.0 is the composition by hand - the teacher's
    logits times float32(1 / 2) into ops.pseudo_label - in labels, weights and the unlabelled loss"""
    from segmif_amd import losses, ops
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
    from segmif_amd.train import make_seg_optimizer
    net, xL, yL, xU = _st_setup()
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with torch.no_grad():
        t_logits = net._segment_nhwc(xU).clone()
    tau = float(ops.pseudo_label(t_logits * 0.5, H, W, return_conf=True)[2].median())
    results = []
    for kw in ({}, {"teacher_temperature": 1.0}, {"teacher_temperature": 2.0}):
        n = copy.deepcopy(net)
        opt = make_seg_optimizer(n, iter_curr=10000, ema_decay=0.9)
        step = SelfTrainingStep(n, EmaTeacher(opt, n), opt, crit, tau=tau, **kw)
        yU, q = step.pseudo(xU)
        l_sup, l_unsup = step.step(xL, yL, xU)
        results.append((yU, q, l_sup, l_unsup, [p.detach().clone() for p in n.parameters()], step.confident_share()))
    plain, one, two = results
    assert torch.equal(plain[0], one[0]) and all(torch.equal(bits(a), bits(b)) for a, b in zip(plain[1:4], one[1:4]))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plain[4], one[4]))
    labels, count = ops.pseudo_label(t_logits * float(np.float32(1.0) / np.float32(2.0)), H, W, tau=tau)
    assert torch.equal(two[0], labels) and torch.equal(bits(two[1]), bits(ops.pseudo_weight(count, H, W)))
    assert torch.equal(two[0], plain[0]) and not torch.equal(two[1], plain[1])  # the argmax does not move, the confident share does
    assert 0.2 < two[5] < 0.8 and two[5] != plain[5]
    twin = copy.deepcopy(net)
    want = twin._loss(xU, labels, losses.SegObjective(reduction="mean_all"), sample_weight=ops.pseudo_weight(count, H, W)).detach()
    assert abs(float(two[3]) - float(want)) <= 1e-5 * abs(float(want))


# ---- the pair forward and the evaluator -------------------------------------------------------------------------------------------------------

EH, EW = 48, 64
PLAIN_KEYS = {"EN", "SD", "SF", "AG", "MI", "SCD", "CC", "PSNR", "mean", "precision", "recall", "iou", "mIoU"}


@pytest.fixture(scope="module")
def nets(cal):
    import segmif_amd.core as core
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    return seg.cuda().eval(), fus.cuda().eval()


def frames(seed, n):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:EH, 0:EW]
    ir = np.stack([np.uint8(127 + 100 * np.sin(yy / (3.0 + b) + seed) * np.cos(xx / 5.0)) for b in range(n)])
    vis = np.stack([np.stack([np.uint8(rng.integers(0, 40) + 2 * xx + yy), np.uint8(3 * yy + b), np.uint8(255 - 2 * xx)], axis=-1) for b in range(n)])
    mask = np.uint8((ir.astype(np.int32) + vis[..., 0]) // 2)
    label = rng.integers(0, 9, (n, EH // 8, EW // 8)).repeat(8, axis=1).repeat(8, axis=2).astype(np.int64)
    label[:, :3, :7] = 255
    return [torch.from_numpy(a).cuda() for a in (ir, vis, mask, label)]


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_pair_forward_hands_out_the_logits(cal, nets, mode):
    """check 7, PairForward: the last element is _segment_nhwc's logits of the returned fused image, the labels are their
    bilinear_argmax; without the argument the tuple is what it was, bit for bit"""
    from segmif_amd import ops
    from segmif_amd.evaluate import _dequantize
    from segmif_amd.pipeline import PairForward
    ir_u8, vis_u8, mask_u8, _ = frames(70, 2)
    with torch.no_grad():
        ir, vis = _dequantize(ir_u8.unsqueeze(3)), _dequantize(vis_u8)
        mask3 = _dequantize(mask_u8.unsqueeze(3)).repeat(1, 3, 1, 1)
        with_logits, plain = PairForward(*nets, return_logits=True), PairForward(*nets)
        seen, inner = [], nets[0]._segment_nhwc
        nets[0]._segment_nhwc = lambda fused: (seen.append(inner(fused)), seen[-1])[1]  # what _segment_nhwc returned INSIDE this forward
        try:
            if mode == "captured":
                with_logits.capture(ir, vis, mask3)
            out = with_logits(ir, vis, mask3)
        finally:
            del nets[0]._segment_nhwc
        if mode == "captured":
            plain.capture(ir, vis, mask3)
        out0 = plain(ir, vis, mask3)
        assert len(out) == 3 and len(out0) == 2
        assert torch.equal(bits(out[0]), bits(out0[0])) and torch.equal(out[1], out0[1])
        logits = out[2]
        assert tuple(logits.shape) == (2, EH // 4, EW // 4, 9) and logits.dtype == torch.float32
        # (a call of _segment_nhwc on its own opens a guarded scope of its own, whose f16x3 range slots are not the pair forward's:
        # its bits may differ in the last places, so the comparison is with the call the pair forward itself made)
        # (more than one call: capture()'s warm-ups, or the range guard computed flagged pairs again - all of them: the last call's
        # result is returned; some: they were patched into the first call's tensor in place)
        assert any(t.shape == logits.shape and torch.equal(bits(logits), bits(t)) for t in seen)
        assert torch.equal(ops.bilinear_argmax(logits, EH, EW), out[1])
        both = PairForward(*nets, uint8_roundtrip=True, return_u8=True, return_logits=True)(ir, vis, mask3)
        assert len(both) == 4 and both[2].dtype == torch.uint8 and tuple(both[3].shape) == tuple(logits.shape)


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_evaluator_sums_one_table(cal, nets, mode):
    """check 7, Evaluator: three labelled batches - the table equals calibration_stats summed over the pair forward's own logits;
    without calibration= the result keys and document() are what they were"""
    import json
    from segmif_amd.evaluate import Evaluator, _dequantize
    kw = {"graph": True} if mode == "graph" else {}
    settings = dict(bins=10, temperatures=(1.0, 1.5), thresholds=(0.5, 0.968))
    ev, plain = Evaluator(*nets, calibration=settings, **kw), Evaluator(*nets, **kw)
    want = None
    for i in range(3):
        ir_u8, vis_u8, mask_u8, label = frames(80 + i, 2)
        _, labels = ev.update(ir_u8, vis_u8, mask_u8, label)
        _, labels0 = plain.update(ir_u8, vis_u8, mask_u8, label)
        assert torch.equal(labels, labels0)
        with torch.no_grad():
            ir, vis = _dequantize(ir_u8.unsqueeze(3)), _dequantize(vis_u8)
            mask3 = _dequantize(mask_u8.unsqueeze(3)).repeat(1, 3, 1, 1)
            out = ev.pair.replay(ir, vis, mask3) if mode == "graph" else ev.pair.eager(ir, vis, mask3)
        assert torch.equal(out[1], labels)
        want = cal.calibration_stats(out[3], label, temperatures=(1.0, 1.5), edges=cal.uniform_edges(10), thresholds=(0.5, 0.968), out=want)
    for k in ("counts", "above", "totals"):
        assert torch.equal(getattr(ev._calibration, k), getattr(want, k)), k
    assert torch.equal(ev._calibration.sums.view(torch.int64), want.sums.view(torch.int64))
    assert int(want.totals.sum()) == 3 * 2 * EH * EW and int(want.totals[1]) == 3 * 2 * 21
    res, res0 = ev.results(), plain.results()
    assert set(res0) == PLAIN_KEYS and set(res) == PLAIN_KEYS | set(cal.CALIBRATION_SCORE_NAMES)
    for k in PLAIN_KEYS - {"mean"}:
        assert np.array_equal(np.asarray(res0[k]), np.asarray(res[k]), equal_nan=True), k
    assert res0["mean"] == res["mean"]
    scores = cal.calibration_scores(want)
    for k in ("ece", "mce", "nll", "brier", "accuracy", "confidence", "above_coverage", "above_precision"):
        assert np.array_equal(res[k], scores[k], equal_nan=True), k
    assert res["best"] == scores["best"] and res["temperatures"].tolist() == [1.0, 1.5]
    doc, doc0 = ev.document(["x"] * 6, []), plain.document(["x"] * 6, [])
    assert doc["calibration"] == {"bins": 10, "edges": [float(v) for v in cal.uniform_edges(10)], "temperatures": [1.0, 1.5],
                                  "thresholds": [0.5, float(np.float32(0.968))]}
    assert "calibration" not in doc0 and set(doc0) == PLAIN_KEYS | {"names", "seeded_weights"}
    json.dumps(doc)
