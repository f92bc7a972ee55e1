"""Host-side checks of the class-balance code (no kernel is launched): the three weight rules against values worked out by hand,
the refusal of a label outside the classes, the sampler's distribution, candidates, determinism and sequential share, the
entry points' rejections and every new refusal of the training command line."""
import ctypes
import math
import random

import numpy as np
import pytest

# 4 frames, 4 classes: class 3 is absent, class 2 lives in frame 0 only; frame 0 also holds 7 ignored pixels
TABLE = np.zeros((4, 257), dtype=np.int64)
TABLE[:, :4] = [[60, 30, 10, 0], [80, 20, 0, 0], [100, 0, 0, 0], [50, 50, 0, 0]]
TABLE[0, 255] = 7
NAMES4 = ["a", "b", "c", "d"]


def stats4():
    from segmif_amd.data import LabelStats
    return LabelStats(TABLE, NAMES4, n_class=4)


def test_table_fields():
    s = stats4()
    assert s.pixels.dtype == np.int64 and s.pixels.tolist() == [290, 100, 10, 0]
    assert s.frames.tolist() == [4, 3, 1, 0]
    assert s.valid.tolist() == [100, 100, 100, 100]  # (the ignored pixels are not labelled pixels)
    assert np.array_equal(s.freq, np.array([290, 100, 10, 0]) / 400.0)
    rows = s.table()
    assert len(rows) == 5 and "pixels" in rows[0] and rows[3].split()[:2] == ["2", "10"] and rows[3].split()[3] == "1"


def test_weight_rules_against_hand_values():
    s = stats4()
    # inverse: 1 / f = 40/29, 4, 40; their mean is 1316/87
    assert np.allclose(s.class_weights("inverse"), [30 / 329, 87 / 329, 870 / 329, 0.0], rtol=1e-13, atol=0)
    assert abs(s.class_weights("inverse")[:3].mean() - 1.0) < 1e-13
    # median: phi = 290/400 (every frame holds class 0), 100/300 (frames 0, 1, 3), 10/100 (frame 0 only); the median is 1/3
    assert np.allclose(s.class_weights("median"), [40 / 87, 1.0, 10 / 3, 0.0], rtol=1e-13, atol=0)
    assert np.allclose(s.class_weights("enet"), [1 / math.log(1.745), 1 / math.log(1.27), 1 / math.log(1.045), 0.0], rtol=1e-13, atol=0)
    for rule in ("inverse", "median", "enet"):
        w = s.class_weights(rule)
        assert w.dtype == np.float64 and w.shape == (4,) and w[3] == 0.0
    with pytest.raises(ValueError, match="rule"):
        s.class_weights("sqrt")


def test_a_label_outside_the_classes_is_refused():
    from segmif_amd.data import LabelStats
    counts = np.zeros((3, 257), dtype=np.int64)
    counts[:, 0] = 50
    counts[:, 255] = 3
    LabelStats(counts, ["x", "y", "z"], n_class=9)
    counts[2, 9] = 5
    counts[2, 11] = 1
    with pytest.raises(ValueError, match=r"frame 2 \(z\) holds 5 pixels of value 9"):
        LabelStats(counts, ["x", "y", "z"], n_class=9)
    counts[1, 256] = 2
    with pytest.raises(ValueError, match=r"frame 1 \(y\).*outside 0\.\.255"):
        LabelStats(counts, ["x", "y", "z"], n_class=9)


def table9():
    """6 frames, 9 classes: class 7's best frame holds EXACTLY 40 pixels, class 8 is absent"""
    rng = np.random.default_rng(5)
    counts = np.zeros((6, 257), dtype=np.int64)
    counts[:, 0] = rng.integers(5000, 9000, 6)
    for c in range(1, 7):
        counts[:, c] = rng.integers(0, 400 * c, 6) * (rng.random(6) < 0.7)
        counts[c % 6, c] = 100 + 50 * c
    counts[:, 7] = [0, 40, 12, 0, 40, 3]
    return counts


def sampler9(**kw):
    from segmif_amd.data import LabelStats, RareClassSampler
    stats = LabelStats(table9(), [f"f{i}" for i in range(6)])
    kw.setdefault("temperature", 0.2)
    kw.setdefault("min_pixels", 40)
    return stats, RareClassSampler(stats, range(6), **kw)


def test_probabilities_follow_the_formula_and_the_strict_rule_drops():
    stats, s = sampler9()
    assert s.dropped == [7, 8]  # 40 pixels is not MORE than 40; class 8 has none
    assert s.classes == list(range(7))
    f = stats.pixels / stats.pixels.sum()
    z = (1.0 - f[:7]) / 0.2
    want = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
    assert np.allclose(s.prob[:7], want, rtol=1e-14, atol=0) and s.prob[7] == s.prob[8] == 0.0 and abs(s.prob.sum() - 1.0) < 1e-14
    assert sampler9(min_pixels=39)[1].dropped == [8]
    for c in range(9):
        assert s.candidates[c] == [i for i in range(6) if table9()[i, c] > 40]
    # DAFormer's temperature: the rarest remaining class takes nearly everything, and the arithmetic stays finite
    sharp = sampler9(temperature=0.01)[1]
    assert np.isfinite(sharp.prob).all() and abs(sharp.prob.sum() - 1.0) < 1e-14 and int(np.argmax(sharp.prob)) == int(np.argmin(f[:7]))
    from segmif_amd.data import RareClassSampler
    with pytest.raises(ValueError, match="nothing to sample"):
        RareClassSampler(stats, range(6), min_pixels=10 ** 6)
    # a slice of the frames: candidates come from the slice, the frequencies from the whole table
    part = RareClassSampler(stats, [1, 2], temperature=0.2, min_pixels=11)
    assert part.candidates[7] == [1, 2] and all(set(c) <= {1, 2} for c in part.candidates)
    assert np.allclose(part.prob[part.classes], np.exp((1 - f[part.classes]) / 0.2) / np.exp((1 - f[part.classes]) / 0.2).sum(), rtol=1e-12)


def test_draws_candidates_determinism_and_untouched_global_generators():
    random.seed(123), np.random.seed(123)
    py_state, np_state = random.getstate(), np.random.get_state()
    _, a = sampler9(seed=3)
    _, b = sampler9(seed=3)
    _, c = sampler9(seed=4)
    da, db, dc = a.draw(500), b.draw(500), c.draw(500)
    assert da == db and da != dc
    assert all(cls in a.classes and idx in a.candidates[cls] for idx, cls in da)
    assert random.getstate() == py_state
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))


def test_shares_over_20000_draws_lie_within_5_standard_deviations():
    _, s = sampler9(seed=1)
    n = 20000
    got = np.bincount([cls for _, cls in s.draw(n)], minlength=9)
    assert got.sum() == n
    for c in range(9):
        p = s.prob[c]
        assert abs(got[c] - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (c, got[c], n * p)


def test_fraction_mixes_in_the_slice_front_to_back():
    from segmif_amd.data import LabelStats, RareClassSampler
    stats = LabelStats(table9(), [f"f{i}" for i in range(6)])
    s = RareClassSampler(stats, [1, 2, 3, 4], temperature=0.2, min_pixels=11, fraction=0.25, seed=2)
    d = s.draw(4000)
    seq = [i for i, cls in d if cls < 0]
    assert seq == [[1, 2, 3, 4][k % 4] for k in range(len(seq))]  # the cursor moves for sequential samples only
    assert abs(len(seq) - 3000) <= 5 * math.sqrt(4000 * 0.25 * 0.75)
    assert all(i in s.candidates[cls] for i, cls in d if cls >= 0)
    assert s.crop_threshold(48 * 64, 96 * 128) == math.floor(11 * 0.5 * (48 * 64) / (96 * 128)) == 1


def test_want_tables_are_checked_on_the_host():
    from segmif_amd import ops
    assert ops.check_want([[-1, 0], [254, 7]]).dtype == np.int32
    for bad in ([[255, 0]], [[3, -1]], [[300, 5]], [3, 4], [[1.5, 2.0]], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            ops.check_want(bad)
    with pytest.raises(ValueError):
        ops.check_want([[1, 2]], B=2)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from segmif_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    lab, cnt = ctypes.create_string_buffer(64), (ctypes.c_int64 * 257)()
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    for fn in (lib.segmif_label_stats_u8, lib.segmif_label_stats_i64):
        assert fn(None, 1, 8, p(cnt), None) == -22 and fn(p(lab), 1, 8, None, None) == -22
        assert fn(p(lab), 0, 8, p(cnt), None) == -22 and fn(p(lab), 1, 0, p(cnt), None) == -22
    rec, tab, want, got = (ctypes.create_string_buffer(256) for _ in range(4))
    args = lambda **kw: [kw.get("label", p(lab)), 1, 4, 4, kw.get("rec", p(rec)), p(tab), 16, kw.get("B", 1), 4, 4, kw.get("want", p(want)),
                         kw.get("got", p(got)), None, kw.get("n_tally", 0), None]
    for kw in (dict(label=None), dict(rec=None), dict(want=None), dict(got=None), dict(B=0), dict(n_tally=-1)):
        assert lib.segmif_augment_pick_class_u8(*args(**kw)) == -22, kw


REFUSED = [(["--seg-class-weights-from", "median"], "--seg-loss weighted"),
           (["--seg-loss", "focal", "--seg-class-weights-from", "enet"], "--seg-loss weighted"),
           (["--seg-loss", "weighted", "--seg-class-weights-from", "median", "--seg-class-weights"] + ["1"] * 9, "one of the two"),
           (["--seg-loss", "weighted"], "--seg-class-weights-from"),
           (["--seg-loss", "weighted", "--seg-class-weights-from", "sqrt"], "invalid choice"),
           (["--rcs-temperature", "0.01"], "--rare-class-sampling"), (["--rcs-min-pixels", "100"], "--rare-class-sampling"),
           (["--rcs-min-crop-ratio", "0.5"], "--rare-class-sampling"), (["--rcs-fraction", "0.5"], "--rare-class-sampling"),
           (["--rcs-phases", "both"], "--rare-class-sampling"),
           (["--rare-class-sampling", "--rcs-temperature", "0"], "--rcs-temperature"),
           (["--rare-class-sampling", "--rcs-temperature", "nan"], "--rcs-temperature"),
           (["--rare-class-sampling", "--rcs-min-pixels", "-1"], "--rcs-min-pixels"),
           (["--rare-class-sampling", "--rcs-min-crop-ratio", "-0.5"], "--rcs-min-crop-ratio"),
           (["--rare-class-sampling", "--rcs-fraction", "0"], "--rcs-fraction"),
           (["--rare-class-sampling", "--rcs-fraction", "1.5"], "--rcs-fraction"),
           (["--rare-class-sampling", "--rcs-phases", "val"], "invalid choice")]


@pytest.mark.parametrize("argv,needle", REFUSED)
def test_train_refuses_before_the_device_check(argv, needle, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--synthetic", "4"] + argv)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "error:" in err and needle in err


def test_command_line_help_names_the_flags(capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    for flag in ("--seg-class-weights-from {inverse,median,enet}", "--rare-class-sampling", "--rcs-temperature", "--rcs-min-pixels",
                 "--rcs-min-crop-ratio", "--rcs-fraction", "--rcs-phases {seg,fusion,both}", "NOT the reference's loader"):
        assert flag in out, flag
