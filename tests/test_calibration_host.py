"""CPU-only checks of the calibration statistics (csrc/calibration_stats.hip behind utils/calibration.py, the Evaluator's
calibration= and the --calibration / --st-temperature flags; ABI in include/segmif_calib.h).  No kernel is launched here.

  - the header's part of what tests/test_abi_and_host.py and tests/test_abi_contract_host.py check for every header: the symbols it
    is expected to declare, its constants, workspace_bytes, and that the contract table holds every case of its EINVAL list
  - calibration_scores on hand-made tables, uniform_edges, the parser errors, the loud failures of the Python layers
  - the restatement tests/_calibration_ref.py against F.interpolate + softmax in float64 and an ECE worked by hand, and the
    seeded cases of the GPU tests: the restatement alone leaves at most 1 % of the valid pixels of every case out"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _abi_contract_table as table
import _abi_headers as headers
import _calibration_ref as ref
from test_abi_contract_host import check_rejected, records  # noqa: F401 - the fixture: the contract child's records

NAME = "segmif_calibration_stats_f32"


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_these_symbols_and_its_source_is_built():
    from segmif_amd import build
    assert headers.declared("segmif_calib.h") == [NAME, "segmif_calibration_workspace_bytes"]
    assert "calibration_stats.hip" in build.SOURCES


def test_the_headers_constants_and_the_descriptors_fields(tmp_path):
    from segmif_amd import _lib
    got = headers.c_ints("segmif_calib.h", ["SEGMIF_CALIB_MAX_TEMPERATURES", "SEGMIF_CALIB_MAX_EDGES", "SEGMIF_CALIB_MAX_THRESHOLDS",
                                            "SEGMIF_CALIB_BLOCK_COLUMNS", "SEGMIF_CALIB_BLOCK_ROWS", "SEGMIF_CALIB_MAX_GRID"], tmp_path)
    assert got == [_lib.CALIB_MAX_TEMPERATURES, _lib.CALIB_MAX_EDGES, _lib.CALIB_MAX_THRESHOLDS, 256, 4, 65535]
    assert [f for f, _ in _lib.SegmifCalib._fields_] == ["n_temperatures", "n_edges", "n_thresholds", "reserved0", "temperatures", "edges",
                                                         "thresholds", "reserved"]


def test_workspace_bytes_is_positive_for_legal_sizes_and_zero_for_refused_ones(lib):
    size = lib.segmif_calibration_workspace_bytes
    assert size(1, 1, 1, 1) == 16                         # one block, one temperature, two doubles
    assert size(2, 11, 19, 16) == 2 * 3 * 16 * 2 * 8      # 3 blocks of 4 rows per sample
    assert size(1, 129, 257, 2) == 2 * 33 * 2 * 2 * 8     # 2 column blocks x 33 row blocks
    assert size(64, 480, 640, 16) == 64 * 120 * 3 * 16 * 2 * 8
    assert size(65535, 65535, 1, 1) > 0
    for B, OH, OW, NT in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 17), (-1, 1, 1, 1), (65536, 1, 1, 1), (1, 65536, 1, 1)):
        assert size(B, OH, OW, NT) == 0, (B, OH, OW, NT)


# ---- rejections: the cases of the header's EINVAL list, each a row of tests/_abi_contract_table.py that the contract child sent -------

MUTATIONS = [("desc", None), ("x", None), ("label", None), ("counts", None), ("totals", None), ("sums", None), ("workspace", None),
             ("above", None),  # NK = 2 > 0
             ("C", 0), ("C", -1), ("C", 33), ("ldx", 8),
             ("NT", 0), ("NT", -1), ("NT", 17), ("NE", -1), ("NE", 32), ("NK", -1), ("NK", 9),
             ("temperatures", (1.0, 0.0)), ("temperatures", (-1.0, 2.0)), ("temperatures", (math.inf, 2.0)), ("temperatures", (1.0, math.nan)),
             ("edges", (0.25, 0.25, 0.75)), ("edges", (0.5, 0.25, 0.75)), ("edges", (0.0, 0.5, 0.75)), ("edges", (0.25, 0.5, 1.0)),
             ("edges", (-0.5, 0.5, 0.75)), ("edges", (0.25, math.nan, 0.75)),
             ("thresholds", (0.9, 1.5)), ("thresholds", (-0.1, 0.968)), ("thresholds", (math.nan, 0.968)),
             ("B", 0), ("B", -2), ("IH", 0), ("IW", 0), ("OH", 0), ("OW", 0), ("OW", -19),
             ("B", 65536), ("OH", 65536)]
FIELD = {"NT": "n_temperatures", "NE": "n_edges", "NK": "n_thresholds"}  # the header's names for the descriptor's counts


def test_the_cases_cover_the_headers_einval_list():
    args = {a for a, _ in MUTATIONS}
    assert {"desc", "x", "label", "counts", "totals", "sums", "workspace", "above", "C", "ldx", "NT", "NE", "NK", "temperatures", "edges",
            "thresholds", "B", "IH", "IW", "OH", "OW"} <= args
    assert ("B", 65536) in MUTATIONS and ("OH", 65536) in MUTATIONS  # the grid limits


@pytest.mark.parametrize("case", MUTATIONS, ids=[f"{NAME}:{arg}={value}" for arg, value in MUTATIONS])
def test_rejected(records, case):
    check_rejected(records, table.find(NAME, FIELD.get(case[0], case[0]), case[1]))


# ---- scores on hand-made tables ---------------------------------------------------------------------------------------------------------------

Q = 2 ** 32


def _table(counts, above, totals, sums, temperatures=(1.0,), edges=(0.5,), thresholds=(0.9,)):
    from segmif_amd.utils.calibration import CalibrationTable
    return CalibrationTable(np.asarray(counts, dtype=np.int64), np.asarray(above, dtype=np.int64).reshape(len(temperatures), len(thresholds), 2),
                            np.asarray(totals, dtype=np.int64), np.asarray(sums, dtype=np.float64), temperatures, edges, thresholds)


def test_scores_of_a_table_worked_by_hand():
    from segmif_amd.utils.calibration import CALIBRATION_SCORE_NAMES, calibration_scores
    # 10 valid pixels: bin 0 holds 4 (1 correct, mean confidence 0.375), bin 1 holds 6 (5 correct, mean confidence 0.75)
    t = _table([[[4, 1, int(1.5 * Q)], [6, 5, int(4.5 * Q)]]], [[[3, 3]]], [10, 2, 1], [[5.0, 2.5]])
    s = calibration_scores(t)
    assert sorted(s) == sorted(CALIBRATION_SCORE_NAMES)
    assert s["accuracy"][0] == 0.6 and s["confidence"][0] == 0.6
    gap0, gap1 = abs(1 / 4 - 0.375), abs(5 / 6 - 0.75)
    assert s["ece"][0] == pytest.approx(0.4 * gap0 + 0.6 * gap1, rel=1e-15) and s["mce"][0] == max(gap0, gap1)
    assert s["ece"][0] == pytest.approx(ref.ece(np.asarray(t.counts[0]), 10), rel=1e-15)
    assert s["nll"][0] == 0.5 and s["brier"][0] == 0.25
    assert s["reliability_n"].tolist() == [[4, 6]] and s["reliability_accuracy"].tolist() == [[0.25, 5 / 6]]
    assert s["reliability_confidence"].tolist() == [[0.375, 0.75]] and s["bin_edges"].tolist() == [0.0, 0.5, 1.0]
    assert s["above_coverage"].tolist() == [[0.3]] and s["above_precision"].tolist() == [[1.0]]
    assert s["thresholds"].tolist() == [float(np.float32(0.9))] and s["temperatures"].tolist() == [1.0]
    assert s["calibration_pixels"] == {"valid": 10, "ignored": 2, "nonfinite": 1}
    assert s["best"] == {"index": 0, "temperature": 1.0, "nll": 0.5, "ece": s["ece"][0], "mce": s["mce"][0], "brier": 0.25, "accuracy": 0.6,
                         "confidence": 0.6}


def test_scores_an_empty_bin_an_empty_threshold_and_no_pixel_at_all():
    from segmif_amd.utils.calibration import calibration_scores
    s = calibration_scores(_table([[[0, 0, 0], [8, 6, 6 * Q]]], [[[0, 0]]], [8, 0, 0], [[1.0, 1.0]]))
    assert math.isnan(s["reliability_accuracy"][0, 0]) and math.isnan(s["reliability_confidence"][0, 0])
    assert s["ece"][0] == 0.0 and s["mce"][0] == 0.0  # the bin that holds pixels is perfectly calibrated: 0 EXACTLY
    assert s["above_coverage"][0, 0] == 0.0 and math.isnan(s["above_precision"][0, 0])
    s = calibration_scores(_table([[[0, 0, 0], [0, 0, 0]]], [[[0, 0]]], [0, 5, 0], [[0.0, 0.0]]))
    for k in ("accuracy", "confidence", "ece", "mce", "nll", "brier"):
        assert math.isnan(s[k][0]), k
    assert math.isnan(s["above_coverage"][0, 0]) and math.isnan(s["above_precision"][0, 0]) and s["best"] is None


def test_scores_a_perfectly_calibrated_table_has_ece_zero_exactly_and_best_is_the_lowest_nll():
    from segmif_amd.utils.calibration import calibration_scores
    counts = [[[4, 1, 1 * Q], [8, 6, 6 * Q]], [[2, 1, Q], [10, 6, 7 * Q]]]
    s = calibration_scores(_table(counts, [[[8, 6], [2, 2]], [[10, 6], [0, 0]]], [12, 0, 0], [[6.0, 3.0], [3.0, 6.0]], temperatures=(1.0, 2.0),
                                  thresholds=(0.5, 0.95)))
    assert s["ece"][0] == 0.0 and s["mce"][0] == 0.0
    assert s["ece"][1] == pytest.approx((10 / 12) * 0.1, rel=1e-12) and s["mce"][1] == pytest.approx(0.1, rel=1e-12)
    assert s["above_coverage"].tolist() == [[8 / 12, 2 / 12], [10 / 12, 0.0]]
    assert s["above_precision"][0].tolist() == [0.75, 1.0] and s["above_precision"][1, 0] == 0.6 and math.isnan(s["above_precision"][1, 1])
    assert s["best"]["index"] == 1 and s["best"]["temperature"] == 2.0 and s["best"]["nll"] == 0.25 and s["best"]["brier"] == 0.5


def test_uniform_edges_and_default_temperatures():
    from segmif_amd.utils import calibration as cal
    e = cal.uniform_edges()
    assert e.dtype == np.float32 and e.size == 14 and all(e[k - 1] == np.float32(k) / np.float32(15) for k in range(1, 15))
    assert cal.uniform_edges(1).size == 0 and cal.uniform_edges(32).size == 31 and np.array_equal(cal.uniform_edges(15), ref.uniform_edges(15))
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="bins"):
            cal.uniform_edges(bad)
    T = cal.DEFAULT_TEMPERATURES
    assert len(T) == 16 and T[0] == 1.0 and T[1] == pytest.approx(0.5) and T[-1] == pytest.approx(4.0)
    assert np.allclose(np.diff(np.log(T[1:])), math.log(8.0) / 14) and T == ref.T16


def test_settings_fail_loudly():
    from segmif_amd.utils.calibration import CalibrationTable, calibration_stats
    Z = lambda **kw: CalibrationTable.zeros("cpu", **kw)
    for bad in ((), (0.0,), (-1.0,), (math.inf,), (math.nan,), tuple(range(1, 18))):
        with pytest.raises(ValueError, match="temperatures"):
            Z(temperatures=bad)
    for bad in ((0.5, 0.5), (0.5, 0.25), (0.0,), (1.0,), (math.nan,), tuple(np.linspace(0.01, 0.99, 32))):
        with pytest.raises(ValueError, match="edges"):
            Z(edges=bad)
    for bad in ((1.5,), (-0.1,), (math.nan,), (0.5,) * 9):
        with pytest.raises(ValueError, match="thresholds"):
            Z(thresholds=bad)
    t = Z(temperatures=(1.0, 2.0), edges=(), thresholds=())
    assert tuple(t.counts.shape) == (2, 1, 3) and tuple(t.above.shape) == (2, 0, 2) and t.settings()["bins"] == 1
    assert t.same_settings((1.0, 2.0), (), ()) and not t.same_settings((1.0, 2.5), (), ()) and not t.same_settings((1.0, 2.0), None, ())
    with pytest.raises(RuntimeError):  # no CPU fallback
        calibration_stats(torch.zeros(1, 2, 2, 9), torch.zeros(1, 8, 8, dtype=torch.int64))


def test_evaluator_and_pair_forward_refuse_what_is_not_built():
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.pipeline import PairForward
    from segmif_amd.tta import TTA
    with pytest.raises(NotImplementedError, match="not built"):
        Evaluator(None, None, tta=TTA((1.0,), True), calibration={})
    with pytest.raises(ValueError, match="bins, temperatures and thresholds"):
        Evaluator(None, None, calibration={"edges": (0.5,)})
    with pytest.raises(ValueError, match="bins"):
        Evaluator(None, None, calibration={"bins": 40})
    with pytest.raises(ValueError, match="no logit map"):
        PairForward(None, None, tta=TTA((1.0,), True), return_logits=True)
    ev = Evaluator(None, None, calibration={})
    assert ev.pair.return_logits and not Evaluator(None, None).pair.return_logits and not PairForward(None, None).return_logits


def test_self_training_step_refuses_a_bad_temperature():
    import inspect
    from segmif_amd.selftrain import SelfTrainingStep
    assert inspect.signature(SelfTrainingStep.__init__).parameters["teacher_temperature"].default == 1.0
    for bad in (0.0, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="teacher_temperature"):
            SelfTrainingStep(None, None, None, None, teacher_temperature=bad)
    assert SelfTrainingStep(None, None, None, None, teacher_temperature=2).teacher_temperature == 2.0


# ---- parsers --------------------------------------------------------------------------------------------------------------------------------------

EVAL = ["--ir", "a", "--vis", "b", "--mask", "c", "--out", "o"]


def _eval_refused(argv, capsys):
    from segmif_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_evaluate_parser(capsys):
    from segmif_amd import evaluate
    assert "--calibration compares the confidence with the ground truth: it needs --label" in _eval_refused(EVAL + ["--calibration"], capsys)
    for flag, values in (("--calibration-bins", ["10"]), ("--calibration-temperatures", ["1", "2"]), ("--calibration-thresholds", ["0.9"])):
        assert f"{flag} only with --calibration" in _eval_refused(EVAL + ["--label", "l", flag] + values, capsys)
    on = EVAL + ["--label", "l", "--calibration"]
    assert "not built" in _eval_refused(on + ["--flip"], capsys) and "not built" in _eval_refused(on + ["--ms-scales", "0.5", "1"], capsys)
    assert "bins" in _eval_refused(on + ["--calibration-bins", "33"], capsys)
    assert "temperatures" in _eval_refused(on + ["--calibration-temperatures", "0"], capsys)
    assert "thresholds" in _eval_refused(on + ["--calibration-thresholds", "1.5"], capsys)
    args, tta = evaluate.parse_args(EVAL)
    assert evaluate.calibration_settings(args) is None and tta is None
    args, _ = evaluate.parse_args(on)
    assert evaluate.calibration_settings(args) == {}
    args, _ = evaluate.parse_args(on + ["--calibration-bins", "10", "--calibration-temperatures", "1", "1.5", "--calibration-thresholds", "0.9", "0.99"])
    assert evaluate.calibration_settings(args) == {"bins": 10, "temperatures": (1.0, 1.5), "thresholds": (0.9, 0.99)}


TRAIN = ["--synthetic", "8", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2", "--backbone", "mit_b1", "--crop-size", "64",
         "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", "somewhere"]


def test_train_parser_and_plan(capsys):
    from segmif_amd import train

    def checked(argv):
        ap = train.build_parser()
        args = ap.parse_args(argv)
        train.check_args(args, ap.error)
        train.resolve_defaults(args)
        return args

    def refused(argv):
        with pytest.raises(SystemExit) as e:
            checked(argv)
        assert e.value.code == 2
        return capsys.readouterr().err

    assert "--st-temperature belongs to --self-training, which is not given" in refused(TRAIN + ["--st-temperature", "2"])
    st = TRAIN + ["--ema-decay", "0.9", "--self-training"]
    for bad in ("0", "-1", "inf", "nan"):
        assert f"--st-temperature {float(bad)}: must be a finite number > 0" in refused(st + ["--st-temperature", bad])
    off = train.make_plan(checked(st))
    assert off.st_kw == dict(tau=0.968, below="keep", unsup_weight=1.0)  # what it was
    assert train.make_plan(checked(st + ["--st-temperature", "1"])).st_kw == off.st_kw
    on = train.make_plan(checked(st + ["--st-temperature", "1.75"]))
    assert on.st_kw == dict(tau=0.968, below="keep", unsup_weight=1.0, teacher_temperature=1.75)
    assert any("teacher_temperature 1.75" in line for line in on.say) and not any("teacher_temperature" in line for line in off.say)


# ---- the restatement, on the CPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,size", [((1, 1, 1, 1), (1, 1)), ((2, 3, 5, 9), (11, 19)), ((1, 7, 6, 4), (7, 6)), ((1, 5, 4, 13), (3, 9))])
def test_restatement_against_interpolate_and_softmax(shape, size):
    rng = np.random.default_rng(7)
    x = (3 * rng.standard_normal(shape)).astype(np.float32)
    label = rng.integers(0, shape[3], (shape[0],) + size)
    temps = (0.25, 1.0, 8.0, 1.7)
    p = ref.pixels(x, label, size[0], size[1], temps)
    v = F.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert float((torch.from_numpy(ref.interp(x, *size)) - v).abs().max()) <= 1e-5  # (the rule's float32 coordinates against float64 ones)
    y = torch.from_numpy(label)
    assert np.array_equal(p["pred"], v.argmax(-1).numpy()) and p["valid"].all()
    for t, T in enumerate(temps):
        q = torch.softmax(v / T, dim=-1)
        assert np.allclose(p["conf"][t], q.max(-1).values.numpy(), rtol=0, atol=2e-5)
        assert np.allclose(p["nll"][t], F.cross_entropy((v / T).permute(0, 3, 1, 2), y, reduction="none").numpy(), rtol=1e-5, atol=2e-5)
        assert np.allclose(p["brier"][t], ((q - F.one_hot(y, shape[3])) ** 2).sum(-1).numpy(), rtol=0, atol=4e-5)


def test_restatement_tables_and_an_ece_worked_by_hand():
    conf = np.array([[0.2, 0.4, 0.5, 0.9, 0.95, 1.0]], dtype=np.float32)
    correct = np.array([False, True, False, True, True, True])
    counts, above = ref.tables(conf, correct, np.ones((1, 6), dtype=bool), np.array([0.5], dtype=np.float32), (0.9, 0.5), exact_q=True)
    q = lambda *v: int(sum(int(np.float64(np.float32(c)) * 2 ** 32) for c in v))
    assert counts.tolist() == [[[2, 1, q(0.2, 0.4)], [4, 3, q(0.5, 0.9, 0.95, 1.0)]]]  # conf >= edge: 0.5 belongs to the upper bin
    assert above.tolist() == [[[2, 2], [3, 3]]]                                        # conf > tau: strict
    want = (2 / 6) * abs(0.5 - 0.3) + (4 / 6) * abs(0.75 - 0.8375)
    assert ref.ece(counts[0], 6) == pytest.approx(want, rel=1e-6)
    assert ref.bins(np.array([0.0, 1.0], dtype=np.float32), np.array([], dtype=np.float32)).tolist() == [0, 0]


def test_restatement_ignored_labels_nonfinite_logits_and_one_pixel():
    c = ref.make_case("one_pixel")
    p = ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"])
    assert p["conf"].tolist() == [[[[1.0]]]] and p["nll"].tolist() == [[[[0.0]]]] and p["brier"].tolist() == [[[[0.0]]]] and p["correct"].all()
    assert ref.bins(p["conf"].astype(np.float32), c["edges"]).tolist() == [[[[14]]]]  # everything lands in the last bin
    c = ref.make_case("small")
    p = ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"])
    for odd in ref.ODD_LABELS:
        assert (c["label"] == odd).any() and p["ignored"][c["label"] == odd].all()
    assert p["ignored"].sum() == np.isin(c["label"], ref.ODD_LABELS).sum() and not p["nonfinite"].any()
    c = ref.make_case("nonfinite")
    p = ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"])
    assert 0 < p["nonfinite"].sum() < p["valid"].sum() and (p["conf"][:, p["nonfinite"]] == 0).all() and (p["pred"][p["nonfinite"]] == -1).all()
    assert p["valid"].sum() + p["ignored"].sum() + p["nonfinite"].sum() == c["label"].size
    c = ref.make_case("extreme")
    p = ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"])
    assert np.isfinite(p["nll"]).all() and p["nll"].max() > 300 and (np.abs(c["x"]) == 80).any()


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_the_seeded_cases_keep_the_restatement_inside_the_cap(name):
    """check 4 of the GPU tests leaves out the pixels whose float64 confidence lies within 1e-5 of an edge or threshold or whose
    top-2 gap is below 1e-4: at most 1 % of the valid pixels, per temperature, by the restatement alone"""
    c = ref.make_case(name)
    p = ref.pixels(c["x"], c["label"], c["OH"], c["OW"], c["temperatures"])
    keep = ref.stable(p, c["edges"], c["thresholds"])
    valid = int(p["valid"].sum())
    assert valid > 0
    for t in range(len(c["temperatures"])):
        left_out = valid - int(keep[t].sum())
        assert left_out <= 0.01 * valid, (name, t, left_out, valid)
