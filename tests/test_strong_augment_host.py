"""Host-side checks of the strong augmentation (no kernel is launched): the numpy restatement of the rule against colorsys, scipy
and values worked out by hand, the taps, the policy's draws, the table check, the record's layout, the entry points' rejections
and the training command's new flags."""
import colorsys
import ctypes
import os
import random

import numpy as np
import pytest

import _abi_headers as headers
import _strong_aug_ref as sr
F64 = np.float64


def _pixels():
    rng = np.random.RandomState(5)
    fixed = [(0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.7, 0.7, 0.2), (0.3, 0.9, 0.9), (0.6, 0.1, 0.6),  # grey, black, white, two equal maxima
             (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.2, 0.4, 0.4), (3 / 255, 3 / 255, 4 / 255)]
    return np.array(fixed + [tuple(p) for p in rng.rand(200, 3)] + [tuple(p) for p in rng.randint(0, 256, (200, 3)) / 255.0])


@pytest.mark.parametrize("fh", [0.0, 0.1, -0.2, 0.5, -0.5])
def test_hue_step_against_colorsys_pixel_by_pixel(fh):
    px = _pixels()
    v = px.T.reshape(3, 1, -1).astype(F64)
    h, s, V = sr.rgb_to_hsv(v)
    got = sr.hue(v, fh)
    for n, (r, g, b) in enumerate(px):
        ch, cs, cv = colorsys.rgb_to_hsv(r, g, b)
        assert abs(h[0, n] - ch) < 1e-14 or abs(abs(h[0, n] - ch) - 1.0) < 1e-14
        assert abs(s[0, n] - cs) < 1e-14 and V[0, n] == cv
        want = colorsys.hsv_to_rgb((ch + fh) % 1.0, cs, cv)
        assert np.abs(got[:, 0, n] - want).max() < 1e-13, (n, px[n], fh)
    if fh == 0.0:  # the conversion there and back is the identity up to rounding, grey and black included
        assert np.abs(got - v).max() < 1e-14


def test_blur_against_scipy_mirror():
    ndimage = pytest.importorskip("scipy.ndimage")
    from segmif_amd import ops
    rng = np.random.RandomState(2)
    for (h, w), sigma in (((9, 12), 2.0), ((12, 16), 0.15), ((33, 20), 1.15), ((17, 70), 0.6)):
        R, taps = ops.strong_taps(sigma)
        assert R <= min(h, w) - 1
        v = rng.rand(3, h, w)
        full = np.concatenate([taps[R:0:-1], taps[:R + 1]]).astype(F64)
        want = ndimage.correlate1d(ndimage.correlate1d(v, full, axis=2, mode="mirror"), full, axis=1, mode="mirror")
        assert np.abs(sr.blur(v, taps, R) - want).max() < 1e-14
    assert sr.reflect_index(5, 3).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert sr.reflect_index(9, 8).tolist() == list(range(8, 0, -1)) + list(range(9)) + list(range(7, -1, -1))


def test_brightness_contrast_and_saturation_by_hand():
    v = np.array([[[0.5, 0.25]], [[0.5, 0.75]], [[0.5, 1.0]]], dtype=F64)  # a grey pixel and (0.25, 0.75, 1.0)
    assert sr.brightness(v, 1.8).tolist() == [[[0.9, 0.45]], [[0.9, 1.0]], [[0.9, 1.0]]]  # the clamp bites: 1.35 and 1.8 -> 1
    c = [float(np.float32(k)) for k in (0.299, 0.587, 0.114)]
    lum = sr.luma(v)
    assert abs(lum[0, 0] - 0.5 * sum(c)) < 1e-15 and abs(lum[0, 1] - (0.25 * c[0] + 0.75 * c[1] + c[2])) < 1e-15
    m = sr.luma_mean(v)
    assert abs(m - (lum[0, 0] + lum[0, 1]) / 2) < 1e-15
    got = sr.contrast(v, 0.5, 0.6)  # 0.5 v + 0.5 * 0.6
    assert np.abs(got - np.array([[[0.55, 0.425]], [[0.55, 0.675]], [[0.55, 0.8]]])).max() < 1e-15
    assert np.abs(sr.contrast(v, 2.0, 0.6) - np.array([[[0.4, 0.0]], [[0.4, 0.9]], [[0.4, 1.0]]])).max() < 1e-15  # -0.1 -> 0, 1.4 -> 1
    assert np.array_equal(sr.saturation(v, 1.0), v)
    grey = sr.saturation(v, 0.0)  # every channel becomes the luma
    assert np.abs(grey - lum[None]).max() < 1e-15
    half = sr.saturation(v, 0.5)
    assert np.abs(half - (0.5 * v + 0.5 * lum[None])).max() < 1e-15
    # the whole rule on one sample: the mean is the brightness-adjusted one and a sample without jitter has mean 0
    y, mean = sr.strong_augment(v[None], [sr.record(jitter=(1.8, 1.0, 1.0, 0.0))], F64)
    bright = sr.brightness(v, float(np.float32(1.8)))  # (a record holds its factors in float32)
    assert abs(mean[0] - sr.luma_mean(bright)) < 1e-15 and np.abs(y[0] - bright).max() < 1e-14
    y, mean = sr.strong_augment(v[None], [sr.record()], F64)
    assert mean[0] == 0 and np.array_equal(y[0], v)
    # a radius the frame cannot hold, or one past 8, is no blur
    assert sr.effective_radius(9, 64, 64) == 0 and sr.effective_radius(4, 4, 64) == 0 and sr.effective_radius(3, 4, 64) == 3
    assert sr.effective_radius(-1, 64, 64) == 0 and sr.effective_radius(8, 9, 12) == 8


def test_float32_restatement_stays_close_to_float64():
    from segmif_amd import ops
    rng = np.random.RandomState(11)
    worst = 0.0
    for n in range(12):
        h, w = int(rng.randint(12, 40)), 4 * int(rng.randint(3, 10))
        x = rng.rand(2, 3, h, w).astype(np.float32)
        if n % 3 == 0:
            x = (np.round(x * 255) / 255).astype(np.float32)
            x[:, :, :4] = x[:, :1, :4]  # a grey band
        R, taps = ops.strong_taps(rng.uniform(0.15, 2.0))
        recs = [sr.record(jitter=(rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(0.0, 2.0), rng.uniform(-0.5, 0.5)),
                          radius=R if R <= min(h, w) - 1 else 0, taps=taps) for _ in range(2)]
        y64, m64 = sr.strong_augment(x, recs, F64)
        y32, m32 = sr.strong_augment(x, recs, np.float32)
        assert y32.dtype == np.float32 and m32.dtype == np.float32
        worst = max(worst, float(np.abs(y32 - y64).max()), float(np.abs(m32 - m64).max()))
    assert worst < 1e-5, worst  # (observed about 1e-6: the map is continuous, no pixel needs excluding)


def test_strong_taps_sum_symmetry_and_radius():
    from segmif_amd import ops
    for sigma, R in ((0.15, 1), (0.25, 1), (0.26, 2), (0.5, 2), (1.0, 4), (1.15, 5), (1.9, 8), (2.0, 8)):
        r, taps = ops.strong_taps(sigma)
        assert r == R and taps.dtype == np.float32 and taps.shape == (9,) and not taps[R + 1:].any() and (taps[:R + 1] > 0).all()
        assert (np.diff(taps[:R + 1]) < 0).all()
        full = np.concatenate([taps[R:0:-1], taps[:R + 1]]).astype(F64)
        assert np.array_equal(full, full[::-1]) and abs(full.sum() - 1.0) < (2 * R + 1) * 2.0 ** -24
        k = np.arange(-R, R + 1)
        want = np.exp(-k * k / (2 * sigma * sigma))
        assert np.array_equal(taps[:R + 1], (want / want.sum())[R:].astype(np.float32))
    for bad in (0.0, -1.0, 2.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.strong_taps(bad)


def test_draws_of_the_policy():
    from segmif_amd import ops
    from segmif_amd.data import StrongAugment
    random.seed(77), np.random.seed(77)
    py_state, np_state = random.getstate(), np.random.get_state()
    ta, tb = [StrongAugment(seed=4).draw(4) for _ in range(2)]
    assert ta.dtype == ops.strong_rec_dtype() and ta.shape == (4,) and ta.tobytes() == tb.tobytes()
    assert StrongAugment(seed=5).draw(4).tobytes() != ta.tobytes() and StrongAugment(seed=4, rank=1).draw(4).tobytes() != ta.tobytes()
    assert random.getstate() == py_state and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))
    ops.check_strong_table(ta, 4)
    # seven draws per sample whatever the coins: the factors of "always" are those a hand-made generator gives, and the samples
    # that "never" touches are copies while its stream stays the same
    always, never = StrongAugment(jitter_prob=1.0, blur_prob=1.0, seed=9), StrongAugment(jitter_prob=0.0, blur_prob=0.0, seed=9)
    a, n = always.draw(6), never.draw(6)
    rng = random.Random("StrongAugment 9 0")
    for b in range(6):
        rng.random()
        fb, fc, fs = (rng.uniform(0.8, 1.2) for _ in range(3))
        fh = rng.uniform(-0.2, 0.2)
        rng.random()
        R, taps = ops.strong_taps(rng.uniform(0.15, 1.15))
        assert a["jitter_on"][b] == 1 and [a["fb"][b], a["fc"][b], a["fs"][b], a["fh"][b]] == [np.float32(v) for v in (fb, fc, fs, fh)]
        assert a["radius"][b] == R and np.array_equal(a["taps"][b], taps) and a["reserved"][b] == 0
        assert n["jitter_on"][b] == 0 and n["radius"][b] == 0 and [n["fb"][b], n["fc"][b], n["fs"][b], n["fh"][b]] == [1, 1, 1, 0]
        assert n["taps"][b].tolist() == [1.0] + [0.0] * 8
    assert always._py.getstate() == never._py.getstate() == rng.getstate()  # (private, but this is the claim: the streams stay in step)
    seen_j = seen_b = 0
    pol = StrongAugment(seed=1)
    for _ in range(200):
        t = pol.draw(5)
        seen_j, seen_b = seen_j + int(t["jitter_on"].sum()), seen_b + int((t["radius"] > 0).sum())
        assert (np.abs(t["fb"] - 1) <= 0.2001).all() and (np.abs(t["fh"]) <= 0.2001).all() and (t["radius"] <= 5).all()
    assert 700 < seen_j < 900 and 400 < seen_b < 600  # 1000 coins at 0.8 and at 0.5, more than 6 standard deviations of room
    for bad in (dict(jitter_prob=1.5), dict(blur_prob=-0.1), dict(strength=1.5), dict(hue=0.6), dict(sigma=(0.0, 1.0)), dict(sigma=(1.0, 0.5)),
                dict(sigma=(0.5, 2.5))):
        with pytest.raises(ValueError):
            StrongAugment(**bad)
    with pytest.raises(ValueError):
        pol.draw(0)


def test_strong_tables_are_checked_on_the_host():
    from segmif_amd import ops
    dt = ops.strong_rec_dtype()
    assert dt.itemsize == 64
    good = sr.to_table([sr.record(jitter=(1.8, 0.0, 2.0, -0.5), radius=8, taps=ops.strong_taps(2.0)[1]), sr.record()], dt)
    t = ops.check_strong_table(good, 2)
    assert t.dtype == dt and t.shape == (2,) and t.flags["C_CONTIGUOUS"] and t.tobytes() == good.tobytes()
    back = sr.from_table(t)
    assert back[0]["jitter"] == (float(np.float32(1.8)), 0.0, 2.0, -0.5) and back[0]["radius"] == 8 and back[1]["jitter"] is None
    for field, value in (("fb", -0.1), ("fc", float("nan")), ("fs", float("inf")), ("fh", 0.51), ("fh", -0.51), ("fh", float("nan")),
                         ("radius", 9), ("radius", -1), ("reserved", 1)):
        bad = good.copy()
        bad[field][1] = value
        with pytest.raises(ValueError):
            ops.check_strong_table(bad, 2)
    bad = good.copy()
    bad["taps"][0, 3] = float("nan")
    for table, B in ((bad, 2), (good, 3), (good[:1], 2), (good.view(np.int32).reshape(2, 16), 2), (good, 0)):
        with pytest.raises(ValueError):
            ops.check_strong_table(table, B)


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_record_layout_matches_c(lib, tmp_path):
    """ops' numpy record against the C struct's ctypes mirror (which tests/test_abi_and_host.py::test_struct_layouts_match_c holds to
    the header, field by field), and the tile constants against the header"""
    from segmif_amd import _lib, ops
    names = ("jitter_on", "fb", "fc", "fs", "fh", "radius", "taps", "reserved")
    rec, dt = _lib.SegmifStrongAugRec, ops.strong_rec_dtype()
    assert [f for f, _ in rec._fields_] == list(names)
    assert [ctypes.sizeof(rec)] + [getattr(rec, n).offset for n in names] == [dt.itemsize] + [dt.fields[n][1] for n in names]
    assert ctypes.sizeof(rec) == 64 == 4 * ops.STRONG_REC_WORDS
    assert headers.c_ints("segmif_hip.h", ["SEGMIF_STRONG_TILE_H", "SEGMIF_STRONG_TILE_W"], tmp_path) == list(ops.STRONG_TILE)


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(addr)


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    assert lib.segmif_strong_augment_blocks(4, 4) == 1 and lib.segmif_strong_augment_blocks(16, 256) == 1
    assert lib.segmif_strong_augment_blocks(16, 260) == 2 and lib.segmif_strong_augment_blocks(512, 512) == 32
    assert lib.segmif_strong_augment_blocks(4096, 4096) == 32
    for h, w in ((0, 4), (4, 0), (4, 6), (4, 2), (-1, 8)):
        assert lib.segmif_strong_augment_blocks(h, w) == -22
    keep, ptr = zip(*(_aligned(4096) for _ in range(5)))
    names = ("x", "y", "rec", "partial", "mean")
    p = dict(zip(names, ptr))
    args = lambda **kw: [kw.get(n, p[n]) for n in names] + [kw.get("B", 2), kw.get("h", 4), kw.get("w", 8), None]
    off = lambda q, n: ctypes.c_void_p(q.value + n)
    bad = [{n: None} for n in names] + [dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0), dict(w=2), dict(w=6), dict(w=10)]
    bad += [dict(x=off(p["x"], 4)), dict(x=off(p["x"], 8)), dict(y=off(p["y"], 8)), dict(partial=off(p["partial"], 4)),
            dict(rec=off(p["rec"], 2)), dict(mean=off(p["mean"], 2))]
    for kw in bad:
        assert lib.segmif_strong_augment_f32(*args(**kw)) == -22, kw
    del keep


SELF = ["--ema-decay", "0.9", "--self-training"]
STRONG = SELF + ["--st-strong"]
REFUSED = [(["--st-strong"], "--st-strong belongs to --self-training, which is not given"),
           (["--ema-decay", "0.9", "--st-strong"], "--st-strong belongs to --self-training"),
           (SELF + ["--st-jitter-prob", "0.5"], "--st-jitter-prob belongs to --st-strong, which is not given"),
           (SELF + ["--st-jitter-strength", "0.5"], "--st-jitter-strength belongs to --st-strong"),
           (SELF + ["--st-jitter-hue", "0.1"], "--st-jitter-hue belongs to --st-strong"),
           (SELF + ["--st-blur-prob", "0.5"], "--st-blur-prob belongs to --st-strong"),
           (SELF + ["--st-blur-sigma", "0.2", "0.4"], "--st-blur-sigma belongs to --st-strong"),
           (["--st-blur-prob", "0.5"], "--st-blur-prob belongs to --st-strong"),
           (STRONG + ["--st-jitter-prob", "1.5"], "--st-jitter-prob 1.5: must lie in [0, 1]"),
           (STRONG + ["--st-jitter-prob", "nan"], "--st-jitter-prob nan: must lie"),
           (STRONG + ["--st-jitter-strength", "1.2"], "--st-jitter-strength 1.2: must lie in [0, 1]"),
           (STRONG + ["--st-jitter-hue", "0.6"], "--st-jitter-hue 0.6: must lie in [0, 0.5]"),
           (STRONG + ["--st-jitter-hue", "-0.1"], "--st-jitter-hue -0.1: must lie"),
           (STRONG + ["--st-blur-prob", "-0.5"], "--st-blur-prob -0.5: must lie in [0, 1]"),
           (STRONG + ["--st-blur-sigma", "0", "1"], "needs 0 < LO <= HI <= 2"),
           (STRONG + ["--st-blur-sigma", "1", "0.5"], "needs 0 < LO <= HI <= 2"),
           (STRONG + ["--st-blur-sigma", "1", "2.5"], "needs 0 < LO <= HI <= 2"),
           (STRONG + ["--st-blur-sigma", "1"], "expected 2 arguments")]


@pytest.mark.parametrize("argv,needle", REFUSED)
def test_train_refuses_before_the_device_check(argv, needle, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--synthetic", "4"] + argv)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "error:" in err and needle in err


def _plan(argv):
    from segmif_amd import train
    ap = train.build_parser()
    args = ap.parse_args(["--synthetic", "8"] + argv)
    train.check_args(args, ap.error)
    train.resolve_defaults(args)
    return train.make_plan(args)


def test_plan_and_announcement_of_the_new_flags():
    off = _plan(SELF)
    assert off.st_kw == dict(tau=0.968, below="keep", unsup_weight=1.0) and not any("--st-strong" in line for line in off.say)
    plan = _plan(STRONG)
    daformer = dict(jitter_prob=0.8, strength=0.2, hue=0.2, blur_prob=0.5, sigma=(0.15, 1.15))
    assert plan.st_kw == dict(tau=0.968, below="keep", unsup_weight=1.0, strong_kw=daformer) and plan.st_mix_kw is None
    line = [s for s in plan.say if s.startswith("[train] --self-training (")]
    assert len(line) == 1 and "\n" not in line[0]
    assert ("(tau 0.968, below keep, unsup_weight 1.0; {unlabelled} unlabelled frames; --st-strong jitter_prob 0.8, strength 0.2, hue 0.2, "
            "blur_prob 0.5, sigma (0.15, 1.15):") in line[0] and "NOT the reference's training" in line[0]
    plan = _plan(STRONG + ["--st-mix", "--st-jitter-prob", "1", "--st-jitter-strength", "0.4", "--st-jitter-hue", "0.5", "--st-blur-prob", "0",
                           "--st-blur-sigma", "0.5", "2"])
    assert plan.st_kw["strong_kw"] == dict(jitter_prob=1.0, strength=0.4, hue=0.5, blur_prob=0.0, sigma=(0.5, 2.0))
    line = [s for s in plan.say if s.startswith("[train] --self-training (")][0]
    assert line.index("--st-mix prob 1.0") < line.index("--st-strong jitter_prob 1.0")
    from segmif_amd.data import StrongAugment
    StrongAugment(seed=3, **plan.st_kw["strong_kw"]).draw(2)  # the plan's keywords are the policy's


def test_command_line_help_names_the_flags(capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    for flag in ("--st-strong ", "--st-jitter-prob P", "--st-jitter-strength S", "--st-jitter-hue H", "--st-blur-prob P", "--st-blur-sigma LO HI"):
        assert flag in out, flag


def test_step_takes_the_policy_as_its_last_keyword():
    """SelfTrainingStep's signature: strong comes last and defaults to None (the device tests run the step)"""
    import inspect
    from segmif_amd.selftrain import SelfTrainingStep
    sig = inspect.signature(SelfTrainingStep.__init__)
    assert sig.parameters["strong"].default is None and list(sig.parameters)[-1] == "strong"
