"""CPU-only checks of the object-level statistics (csrc/objects.hip behind utils/objects.py, the Evaluator's objects= and the
--object-* flags; ABI in include/segmif_objects.h).  No kernel is launched here.

  - the restatement tests/_objects_ref.py (min-propagation to a fixed point) against scipy.ndimage.label per class, components
    canonicalised to their minimum index, on every case of CASES under both connectivities; and against three cases worked by hand
  - object_scores on a table written by hand: an empty class, P + R = 0, the means, a bad coverage, a set status word
  - the header's part of what tests/test_abi_and_host.py and tests/test_abi_contract_host.py check for every header: the symbols it
    is expected to declare, its constants, workspace_bytes, and that the contract table holds every case of its EINVAL list
  - the evaluate parser's new errors; Evaluator(objects=) refuses unknown keys"""
import math
import os

import numpy as np
import pytest

import _abi_contract_table as table
import _abi_headers as headers
import _objects_ref as ref
from test_abi_contract_host import check_rejected, records  # noqa: F401 - the fixture: the contract child's records

NAME = "segmif_object_stats_i32"


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------

def scipy_roots(m, conn):
    """(H, W) map with IGN -> the minimum linear index of each pixel's component by scipy.ndimage.label per class"""
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    H, W = m.shape
    idx = np.arange(H * W).reshape(H, W)
    out = np.full((H, W), -1, dtype=np.int32)
    for c in np.unique(m[m != ref.IGN]):
        lab, n = ndi.label(m == c, structure=structure)
        if n:
            lo = ndi.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int64)
            out[lab > 0] = lo[lab[lab > 0] - 1]
    return out


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_restatement_against_scipy_label(name, conn):
    pytest.importorskip("scipy")
    c = ref.case(name, conn)
    g, p = ref.maps(c["pred"], c["label"], c["K"])
    for b in range(len(g)):
        assert np.array_equal(c["root_g"][b], scipy_roots(g[b], conn)), (name, conn, "g")
        assert np.array_equal(c["root_p"][b], scipy_roots(p[b], conn)), (name, conn, "p")
    # the tables count each component once and every valid pixel once
    for side, m in enumerate((g, p)):
        roots = c["root_g"] if side == 0 else c["root_p"]
        for b in range(len(g)):
            assert c["obj"][b, side].sum() == len(np.unique(roots[b][roots[b] >= 0]))
            assert c["mass"][b, side, :, :, 0].sum() == (m[b] != ref.IGN).sum()
            assert c["mass"][b, side, :, :, 1].sum() == ((m[b] != ref.IGN) & (g[b] == p[b])).sum()


def test_the_cases_hold_what_they_are_there_for():
    K4, K8 = ref.case("checkerboard_66", 4), ref.case("checkerboard_66", 8)
    assert K4["obj"][0, 0].sum() == 66 * 66 and K8["obj"][0, 0].sum() == 2
    assert ref.case("diagonal_130", 8)["obj"][0, 0, 1].sum() == 1 and ref.case("diagonal_130", 4)["obj"][0, 0, 1].sum() == 130
    assert ref.case("antidiagonal_130", 8)["obj"][0, 0, 1].sum() == 1 and ref.case("antidiagonal_130", 4)["obj"][0, 0, 1].sum() == 130
    for name in ("serpentine_64", "serpentine_130"):
        c = ref.case(name)
        n = int(name.split("_")[1])
        assert c["obj"][0, 0, 1].sum() == 1 and c["mass"][0, 0, 1, :, 0].sum() == (c["label"] == 1).sum() >= n * n // 2
    c = ref.case("constant_130")
    assert c["obj"][0, 0].sum() == 1 and c["mass"][0, 0, 2, 2, 0] == 130 * 130 and (c["root_g"] == 0).all()
    c = ref.case("all_ign")
    assert not c["obj"].any() and not c["mass"].any() and (c["root_g"] == -1).all() and (c["root_p"] == -1).all()
    c = ref.case("odd_labels")
    for v in ref.ODD_LABELS:
        assert (c["label"] == v).any() and (c["root_g"][c["label"] == v] == -1).all() and (c["root_p"][c["label"] == v] == -1).all()
    c = ref.case("pred_out_of_range")
    bad = (c["pred"] < 0) | (c["pred"] >= 9)
    assert bad.sum() > 100 and (c["root_p"][bad] == -1).all() and (c["root_g"][bad] >= 0).any()
    c = ref.case("ignored_stripe")
    assert c["obj"][0, 1, 3].sum() == 2 and c["obj"][0, 0, 3].sum() == 2  # the stripe cuts the predicted blob (and the object) in two


def test_a_diagonal_pair_joins_under_8_and_splits_under_4():
    label = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 0]]], dtype=np.int64)
    pred = label.astype(np.int32)
    r8 = ref.object_stats(pred, label, 2, 8, ())
    r4 = ref.object_stats(pred, label, 2, 4, ())
    assert r8[0][0].tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 1]]  # the 1s: root 0; the 0s: one component, root 1
    assert r4[0][0].tolist() == [[0, 1, 1], [1, 4, 1], [1, 1, 1]]  # two 1s of their own; the zeros go round through the corner (2, 2)
    assert r8[2][0, 0, 1, 0, 10] == 1 and r8[2][0, 0, 1].sum() == 1 and r4[2][0, 0, 1, 0, 10] == 2
    assert r8[3][0, 0, 1, 0].tolist() == [2, 2] and r4[3][0, 0, 0, 0].tolist() == [7, 7]


def test_a_half_covered_object_has_decile_5_and_a_covered_one_10():
    label = np.zeros((1, 4, 6), dtype=np.int64)
    label[0, 1:3, 1:5] = 1              # 8 pixels
    pred = np.zeros((1, 4, 6), dtype=np.int32)
    pred[0, 1:3, 1:3] = 1               # 4 of them
    _, _, obj, mass = ref.object_stats(pred, label, 2, 8, (8,))
    assert obj[0, 0, 1, 1].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and obj[0, 0, 1, 0].sum() == 0  # area 8 >= edge 8: bucket 1
    assert mass[0, 0, 1, 1].tolist() == [8, 4]
    assert obj[0, 1, 1, 0, 10] == 1 and mass[0, 1, 1, 0].tolist() == [4, 4]  # the predicted blob lies inside the object: hit == area
    assert obj[0, 0, 0].sum() == 1 and obj[0, 0, 0, 1, 10] == 1              # the background is covered whole (16 of 16)
    assert obj[0, 1, 0, 1, 8] == 1 and mass[0, 1, 0, 1].tolist() == [20, 16]  # the predicted background: 16 of 20 -> decile 8
    R, P, F = ref.scores(obj[0], 0.5)
    assert R.tolist() == [1.0, 1.0] and P.tolist() == [1.0, 1.0]              # detected at 0.5 ...
    assert ref.scores(obj[0], 0.6)[0].tolist() == [1.0, 0.0]                  # ... and not at 0.6


# ---- scores on a table written by hand ------------------------------------------------------------------------------------------------------

def _table(obj, status=(0, 0), edges=(10,)):
    from segmif_amd.utils.objects import ObjectTable
    obj = np.asarray(obj, dtype=np.int64)
    return ObjectTable(obj, np.zeros(obj.shape[:-1] + (2,), dtype=np.int64), np.asarray(status, dtype=np.int32), obj.shape[-3], 8, edges)


def _hand():
    obj = np.zeros((2, 4, 2, 11), dtype=np.int64)
    # class 0: 4 objects (3 small: deciles 10, 5, 4; 1 large: decile 9), 2 predictions (deciles 5 and 0)
    obj[0, 0, 0, 10] = obj[0, 0, 0, 5] = obj[0, 0, 0, 4] = obj[0, 0, 1, 9] = 1
    obj[1, 0, 0, 5] = obj[1, 0, 1, 0] = 1
    # class 1: objects, none found; predictions, none right: P + R = 0
    obj[0, 1, 0, 0] = 2
    obj[1, 1, 0, 3] = 1
    # class 2: objects but no prediction: an empty denominator.  class 3: empty on both sides
    obj[0, 2, 1, 10] = 5
    return obj


def test_scores_of_a_table_worked_by_hand():
    from segmif_amd.utils.objects import OBJECT_SCORE_NAMES, object_scores
    s = object_scores(_table(_hand()), 0.5)
    assert sorted(s) == sorted(OBJECT_SCORE_NAMES)
    assert s["obj_recall"][:3].tolist() == [0.75, 0.0, 1.0] and math.isnan(s["obj_recall"][3])
    assert s["obj_precision"][:2].tolist() == [0.5, 0.0] and math.isnan(s["obj_precision"][2]) and math.isnan(s["obj_precision"][3])
    assert s["obj_f1"][0] == 2 * 0.5 * 0.75 / 1.25 and s["obj_f1"][1] == 0.0 and math.isnan(s["obj_f1"][2]) and math.isnan(s["obj_f1"][3])
    assert s["mObjRecall"] == (0.75 + 0 + 1 + 0) / 4 and s["mObjPrecision"] == 0.5 / 4 and s["mObjF1"] == s["obj_f1"][0] / 4
    assert s["n_gt_objects"].tolist() == [[3, 1], [2, 0], [0, 5], [0, 0]] and s["n_pred_objects"].tolist() == [[1, 1], [1, 0], [0, 0], [0, 0]]
    assert s["obj_recall_by_size"][0].tolist() == [2 / 3, 1.0] and s["obj_precision_by_size"][0].tolist() == [1.0, 0.0]
    assert math.isnan(s["obj_recall_by_size"][1, 1]) and s["obj_recall_by_size"][2, 1] == 1.0
    R, P, F = ref.scores(_hand(), 0.5)
    for k, want in (("obj_recall", R), ("obj_precision", P), ("obj_f1", F)):
        assert np.array_equal(s[k], want, equal_nan=True), k
    assert object_scores(_table(_hand()), 1.0)["obj_recall"][:3].tolist() == [0.25, 0.0, 1.0]
    assert object_scores(_table(_hand()), 0.1)["obj_precision"][:2].tolist() == [0.5, 1.0]
    per_frame = _table(np.stack([_hand(), 2 * _hand()]))  # per-frame tables are summed first
    assert np.array_equal(object_scores(per_frame, 0.5)["n_gt_objects"], 3 * s["n_gt_objects"])
    assert np.array_equal(object_scores(per_frame, 0.5)["obj_recall"], s["obj_recall"], equal_nan=True)


def test_scores_refuse_a_bad_coverage_and_a_set_status_word():
    from segmif_amd.utils.objects import object_scores
    for bad in (0.0, 0.05, 0.55, 1.1, -0.5, 5):
        with pytest.raises(ValueError, match="0.1, 0.2 ... 1.0"):
            object_scores(_table(_hand()), bad)
    for ok in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1):
        object_scores(_table(_hand()), ok)
    with pytest.raises(RuntimeError, match="iteration cap"):
        object_scores(_table(_hand(), status=(1, 0)))


def test_settings_fail_loudly():
    import torch
    from segmif_amd.utils import objects as ob
    assert ob.DEFAULT_SIZE_EDGES == (1024, 9216) == ref.DEFAULT_SIZE_EDGES
    Z = ob.ObjectTable.zeros
    for bad in ((5, 5), (9, 3), (0, 4), (-1,), (1, 2, 3, 4), (1.5,)):
        with pytest.raises(ValueError, match="size_edges"):
            Z("cpu", size_edges=bad)
    for bad in (0, 6, 16, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            Z("cpu", connectivity=bad)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="n_class"):
            Z("cpu", n_class=bad)
    t = Z("cpu", 3, 4, ())
    assert tuple(t.obj.shape) == (2, 3, 1, 11) and tuple(t.mass.shape) == (2, 3, 1, 2) and t.status.dtype == torch.int32
    assert t.same_settings(3, 4, ()) and not t.same_settings(3, 8, ()) and not t.same_settings(3, 4, (7,))
    assert t.settings() == {"connectivity": 4, "size_edges": []}
    assert tuple(Z("cpu", batch=5).obj.shape) == (5, 2, 9, 3, 11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ob.object_stats(torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ob.connected_components(torch.zeros(1, 4, 4, dtype=torch.int32), 2)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_these_symbols_and_its_source_is_built():
    from segmif_amd import build
    assert headers.declared("segmif_objects.h") == [NAME, "segmif_object_workspace_bytes"]
    assert "objects.hip" in build.SOURCES


def test_the_headers_constants_and_the_descriptors_fields(tmp_path):
    from segmif_amd import _lib
    got = headers.c_ints("segmif_objects.h", ["SEGMIF_OBJECTS_TILE", "SEGMIF_OBJECTS_RUN", "SEGMIF_OBJECTS_MAX_EDGES", "SEGMIF_OBJECTS_DECILES",
                                              "SEGMIF_OBJECTS_MAX_FRAMES", "SEGMIF_OBJECTS_WORKSPACE_PER_PIXEL"], tmp_path)
    assert got == [64, 8, _lib.OBJECTS_MAX_EDGES, _lib.OBJECTS_DECILES, _lib.OBJECTS_MAX_FRAMES, _lib.OBJECTS_WORKSPACE_PER_PIXEL]
    assert [f for f, _ in _lib.SegmifObjects._fields_] == ["connectivity", "n_edges", "edges", "reserved"]


def test_workspace_bytes_is_positive_for_legal_sizes_and_zero_for_refused_ones(lib):
    size = lib.segmif_object_workspace_bytes
    assert size(1, 1, 1) == 32                       # 26 bytes, rounded up to a multiple of 8
    assert size(1, 7, 5) == 912 and size(3, 65, 129) == 3 * 65 * 129 * 26 + 2
    assert size(64, 480, 640) == 64 * 480 * 640 * 26
    assert size(32767, 1, 1) > 0 and size(1, 46340, 46340) == 46340 * 46340 * 26
    for B, H, W in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (32768, 1, 1), (1, 65536, 32768), (1, 46341, 46341)):
        assert size(B, H, W) == 0, (B, H, W)


# ---- rejections: the cases of the header's EINVAL list, each a row of tests/_abi_contract_table.py that the contract child sent -------

MUTATIONS = [("desc", None), ("pred", None), ("label", None), ("obj", None), ("mass", None), ("status", None), ("workspace", None),
             ("K", 0), ("K", -1), ("K", 33),
             ("connectivity", 0), ("connectivity", 6), ("connectivity", -8), ("connectivity", 16),
             ("n_edges", -1), ("n_edges", 4),
             ("edges", (1024, 1024)), ("edges", (9216, 1024)), ("edges", (0, 9216)), ("edges", (-5, 9216)),
             ("B", 0), ("B", -2), ("H", 0), ("H", -37), ("W", 0), ("W", -53),
             ("HW", (65536, 32768)), ("HW", (46341, 46341)), ("HW", (2, 2 ** 30)),  # H * W >= 2^31
             ("B", 32768)]  # the grid's z holds 2 B


def test_the_cases_cover_the_headers_einval_list():
    args = {a for a, _ in MUTATIONS}
    assert {"desc", "pred", "label", "obj", "mass", "status", "workspace", "K", "connectivity", "n_edges", "edges", "B", "H", "W", "HW"} <= args
    assert ("B", 32768) in MUTATIONS  # the grid limit


@pytest.mark.parametrize("case", MUTATIONS, ids=[f"{NAME}:{arg}={value}" for arg, value in MUTATIONS])
def test_rejected(records, case):
    check_rejected(records, table.find(NAME, ("H", "W") if case[0] == "HW" else case[0], case[1]))


# ---- the parser and the Evaluator -----------------------------------------------------------------------------------------------------------

EVAL = ["--ir", "a", "--vis", "b", "--mask", "c", "--out", "o"]


def _eval_refused(argv, capsys):
    from segmif_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_evaluate_parser(capsys):
    from segmif_amd import evaluate
    assert "--object-scores compares the label maps' objects with the ground truth's: it needs --label" in _eval_refused(EVAL + ["--object-scores"], capsys)
    for flag, values in (("--object-connectivity", ["4"]), ("--object-size-edges", ["10", "20"]), ("--object-coverage", ["0.7"])):
        assert f"{flag} only with --object-scores" in _eval_refused(EVAL + ["--label", "l", flag] + values, capsys)
    on = EVAL + ["--label", "l", "--object-scores"]
    assert "invalid choice" in _eval_refused(on + ["--object-connectivity", "6"], capsys)
    assert "size_edges" in _eval_refused(on + ["--object-size-edges", "20", "10"], capsys)
    assert "size_edges" in _eval_refused(on + ["--object-size-edges", "1", "2", "3", "4"], capsys)
    assert "coverage" in _eval_refused(on + ["--object-coverage", "0.55"], capsys)
    args, tta = evaluate.parse_args(EVAL)
    assert evaluate.object_settings(args) is None and tta is None
    args, _ = evaluate.parse_args(on)
    assert evaluate.object_settings(args) == {}
    args, tta = evaluate.parse_args(on + ["--object-connectivity", "4", "--object-size-edges", "3", "50", "4000", "--object-coverage", "0.7", "--flip"])
    assert evaluate.object_settings(args) == {"connectivity": 4, "size_edges": (3, 50, 4000), "coverage": 0.7} and tta is not None


def test_evaluator_refuses_unknown_keys_and_bad_settings():
    from segmif_amd.evaluate import Evaluator
    from segmif_amd.tta import TTA
    with pytest.raises(ValueError, match="connectivity, size_edges and coverage"):
        Evaluator(None, None, objects={"edges": (5,)})
    with pytest.raises(ValueError, match="connectivity"):
        Evaluator(None, None, objects={"connectivity": 6})
    with pytest.raises(ValueError, match="size_edges"):
        Evaluator(None, None, objects={"size_edges": (9, 3)})
    with pytest.raises(ValueError, match="coverage"):
        Evaluator(None, None, objects={"coverage": 0.25})
    ev = Evaluator(None, None, objects={}, tta=TTA((1.0,), True))  # with tta= alike: it only reads the label maps
    assert ev.objects == {} and ev._objects_kw == dict(n_class=9, connectivity=8, size_edges=(1024, 9216)) and ev._objects_coverage == 0.5
    assert Evaluator(None, None).objects is None
