"""Host-side checks of ClassMix (no kernel is launched): the numpy restatement of the rule against values worked out by hand, the
policy's draws, the table check, the entry points' rejections and every new refusal of the training command line."""
import ctypes
import math
import random

import numpy as np
import pytest

import _class_mix_ref as mr

KEYS = [8, 0, 7, 1, 6, 2, 5, 3, 4]  # class 1 has the smallest key, then 3, 5, 7, 8, 6, 4, 2, 0


def _row(donor, force=-1, keys=KEYS):
    return [donor, force] + list(keys)


def _counts(*rows):
    c = np.zeros((len(rows), 257), dtype=np.int64)
    for r, row in zip(c, rows):
        for k, v in row.items():
            r[k] = v
    return c


def test_half_of_the_present_classes_by_hand():
    # receiver 0 takes from donor 1, receiver 1 from donor 0
    five, four = {0: 10, 1: 20, 2: 30, 3: 40, 4: 50, 255: 99}, {0: 5, 2: 6, 4: 7, 6: 8}
    sel, pasted, chosen = mr.select(_counts(four, five), [_row(1), _row(0)], 9, 0)
    assert chosen == [[1, 3, 4], [4, 6]]  # 5 present: k = 3, keys 0, 1, 6 of classes 1, 3, 4; 4 present: k = 2, keys 5, 6 of 6, 4
    assert pasted.tolist() == [110, 15] and pasted.dtype == np.int64
    assert sel.dtype == np.int32 and sel.shape == (2, 8)
    assert sel[0].tolist() == [0b11010, 0, 0, 0, 0, 0, 0, 0] and sel[1].tolist() == [0b1010000, 0, 0, 0, 0, 0, 0, 0]
    one, none = {7: 3, 255: 50}, {255: 64}
    sel, pasted, chosen = mr.select(_counts(none, one), [_row(1), _row(0)], 9, 0)
    assert chosen == [[7], []] and pasted.tolist() == [3, 0] and not sel[1].any()
    assert np.array_equal(mr.tally(_counts(four, five), [_row(1), _row(0)], [[1, 3, 4], [4, 6]], 9),
                          [[0, 0], [1, 20], [0, 0], [1, 40], [2, 57], [0, 0], [1, 8], [0, 0], [0, 0]])


def test_strict_threshold_force_and_unmixed_samples_by_hand():
    d = {2: 7, 3: 8, 5: 100}
    cnt = _counts({}, d)
    assert mr.select(cnt, [_row(1), _row(1)], 9, 7)[2] == [[3], []]          # n == min_pixels is absent, min_pixels + 1 present:
    assert mr.select(cnt, [_row(1), _row(1)], 9, 6)[2] == [[3, 5], []]       # {3, 5} -> k 1 -> 3; {2, 3, 5} -> k 2 -> 3, 5
    assert mr.select(cnt, [_row(1, force=5), _row(1)], 9, 7)[2] == [[5], []]  # force present
    sel, pasted, chosen = mr.select(cnt, [_row(1, force=2), _row(1)], 9, 7)  # force absent (7 pixels are not more than 7)
    assert chosen == [[], []] and not sel.any() and not pasted.any()
    sel, pasted, chosen = mr.select(cnt, [_row(1, force=4), _row(1)], 9, 0)  # force nowhere in the donor
    assert chosen == [[], []]
    sel, pasted, chosen = mr.select(_counts(d, d), [_row(0), _row(1)], 9, 0)  # donor == b
    assert chosen == [[], []] and not sel.any() and not pasted.any()


def test_apply_by_hand_and_values_outside_the_classes():
    label = np.full((2, 2, 4), 255, dtype=np.int64)
    label[1] = [[3, 3, 0, 2 ** 40 + 3], [-1, 256, 3, 0]]
    label[0] = [[1, 1, 1, 1], [2, 2, 2, 255]]
    cnt = mr.counts(label, 9)
    assert cnt[1].tolist() == [2, 0, 0, 3, 0, 0, 0, 0, 0] and cnt[0].tolist() == [0, 4, 3, 0, 0, 0, 0, 0, 0]  # 2^40 + 3 is not a 3
    planes = [np.arange(2 * 3 * 2 * 4, dtype=np.int32).reshape(2, 3, 2, 4) + 1000 * q for q in range(3)]
    keep = [p.copy() for p in planes]
    table = [_row(1, force=3), _row(1)]
    sel, pasted, chosen = mr.select(cnt, table, 9, 0)
    assert chosen == [[3], []] and pasted.tolist() == [3, 0]
    out, lab, M = mr.apply(planes, label, [1, 1], sel)
    assert M[0].tolist() == [[True, True, False, False], [False, False, True, False]] and not M[1].any() and M.sum() == pasted.sum()
    assert lab[0].tolist() == [[3, 3, 1, 1], [2, 2, 3, 255]] and np.array_equal(lab[1], label[1])
    for p, o, k in zip(planes, out, keep):
        assert np.array_equal(p, k) and np.array_equal(o[1], p[1])
        assert np.array_equal(o[0][:, M[0]], p[1][:, M[0]]) and np.array_equal(o[0][:, ~M[0]], p[0][:, ~M[0]])
    # every class of the donor selected: the values outside the classes still stay out
    sel_all = np.zeros((2, 8), dtype=np.int32)
    sel_all[0, 0] = 0b1001
    _, lab, M = mr.apply(planes, label, [1, 1], sel_all)
    assert M[0].tolist() == [[True, True, True, False], [False, False, True, True]]
    # nothing selected: the output is the receiver
    out, lab, M = mr.apply(planes, label, [1, 0], np.zeros((2, 8), dtype=np.int32))
    assert not M.any() and np.array_equal(lab, label) and all(np.array_equal(o, p) for o, p in zip(out, planes))
    # a chain pastes ORIGINAL pixels: 0 <- 1 <- 0 with everything selected swaps the two labelled crops
    lab2 = np.stack([np.full((2, 4), 1), np.full((2, 4), 2)]).astype(np.int64)
    both = np.zeros((2, 8), dtype=np.int32)
    both[:, 0] = 0b110
    assert np.array_equal(mr.apply([], lab2, [1, 0], both)[1], lab2[::-1])


def test_draws_of_the_policy():
    from segmif_amd.data import ClassMix
    random.seed(77), np.random.seed(77)
    py_state, np_state = random.getstate(), np.random.get_state()
    a, b, c = ClassMix(prob=0.5, seed=4), ClassMix(prob=0.5, seed=4), ClassMix(prob=0.5, seed=5)
    ta, tb, tc = [a.draw(4) for _ in range(50)], [b.draw(4) for _ in range(50)], [c.draw(4) for _ in range(50)]
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb)) and not all(np.array_equal(x, y) for x, y in zip(ta, tc))
    assert not all(np.array_equal(x, y) for x, y in zip(ta, [ClassMix(prob=0.5, seed=4, rank=1).draw(4) for _ in range(50)]))
    assert random.getstate() == py_state
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))
    mixed = 0
    for t in ta:
        assert t.dtype == np.int32 and t.shape == (4, 11) and (t[:, 1] == -1).all()
        assert (np.sort(t[:, 2:], axis=1) == np.arange(9)).all()
        mixed += int((t[:, 0] != np.arange(4)).sum())
    assert 0 < mixed < 200
    every, never = ClassMix(prob=1.0, seed=1), ClassMix(prob=1e-12, seed=1)
    for _ in range(1000):
        assert (every.draw(3)[:, 0] != np.arange(3)).all()  # the donor is never the sample itself
        assert (never.draw(3)[:, 0] == np.arange(3)).all()
    # the stream does not depend on the outcomes: the permutations of prob 1 and of a tiny prob are the same
    assert np.array_equal(ClassMix(prob=1.0, seed=9).draw(6)[:, 2:], ClassMix(prob=1e-12, seed=9).draw(6)[:, 2:])
    with pytest.raises(ValueError):
        every.draw(1)
    for bad in (dict(prob=0.0), dict(prob=1.5), dict(min_pixels=-1), dict(n_class=0), dict(n_class=256), dict(classes="all")):
        with pytest.raises(ValueError):
            ClassMix(**bad)


def test_donor_shares_over_20000_draws_lie_within_5_standard_deviations():
    from segmif_amd.data import ClassMix
    m, n, B = ClassMix(prob=1.0, seed=2), 20000, 5
    got = np.zeros((B, B), dtype=np.int64)
    for _ in range(n):
        for b, d in enumerate(m.draw(B)[:, 0]):
            got[b, d] += 1
    p = 1.0 / (B - 1)
    for b in range(B):
        assert got[b, b] == 0 and got[b].sum() == n
        for d in range(B):
            if d != b:
                assert abs(got[b, d] - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (b, d, got[b, d])


def test_wanted_maps_the_donors_class_into_force():
    from segmif_amd.data import ClassMix
    m = ClassMix(prob=1.0, classes="wanted", seed=3)
    wanted = [7, -1, 2, 5]
    seen = set()
    for _ in range(200):
        t = m.draw(4, wanted)
        for b in range(4):
            assert t[b, 1] == wanted[t[b, 0]]
            seen.add(int(t[b, 1]))
    assert seen == {7, -1, 2, 5}
    with pytest.raises(ValueError, match="wanted"):
        m.draw(4)
    assert (ClassMix(prob=1.0, classes="half", seed=3).draw(4, wanted)[:, 1] == -1).all()


def test_mix_tables_are_checked_on_the_host():
    from segmif_amd import ops
    good = [_row(1), _row(0, force=8)]
    t = ops.check_mix_table(good, 2, 9)
    assert t.dtype == np.int32 and t.shape == (2, 11) and t.flags["C_CONTIGUOUS"] and t.tolist() == good
    assert ops.check_mix_table(np.asarray(good, dtype=np.int64), 2, 9).dtype == np.int32
    for bad in ([_row(2), _row(0)], [_row(-1), _row(0)], [_row(1, force=9), _row(0)], [_row(1, force=-2), _row(0)],
                [_row(1, keys=[0] * 9), _row(0)], [_row(1, keys=list(range(1, 10))), _row(0)], [_row(1)], [_row(1)[:-1], _row(0)[:-1]],
                np.asarray(good, dtype=np.float64), _row(1)):
        with pytest.raises(ValueError):
            ops.check_mix_table(bad, 2, 9)
    with pytest.raises(ValueError):
        ops.check_mix_table(good, 2, 8)
    with pytest.raises(ValueError):
        ops.check_mix_table(good, 2, 256)


def _aligned(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(addr)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import os
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    keep, ptr = zip(*(_aligned(4096) for _ in range(13)))
    counts, table, sel, pasted, tally = ptr[:5]
    sargs = lambda **kw: [kw.get("counts", counts), kw.get("table", table), kw.get("B", 2), kw.get("n_class", 9), kw.get("min_pixels", 0),
                          kw.get("sel", sel), kw.get("pasted", pasted), kw.get("tally", tally), None]
    off = lambda p, n: ctypes.c_void_p(p.value + n)
    for kw in (dict(counts=None), dict(table=None), dict(sel=None), dict(pasted=None), dict(B=0), dict(n_class=0), dict(n_class=256),
               dict(min_pixels=-1), dict(sel=off(sel, 4)), dict(pasted=off(pasted, 4)), dict(tally=off(tally, 4)), dict(counts=off(counts, 4))):
        assert lib.segmif_class_mix_select(*sargs(**kw)) == -22, kw
    names = ("ir3", "vis3", "mask3", "label", "table", "sel", "ir3_out", "vis3_out", "mask3_out", "label_out")
    p = dict(zip(names, ptr[3:]))
    aargs = lambda **kw: ([kw.get(n, p[n]) for n in names[:6]] + [kw.get("B", 2), kw.get("h", 4), kw.get("w", 8), kw.get("n_class", 9)]
                          + [kw.get(n, p[n]) for n in names[6:]] + [None])
    bad = [{n: None} for n in names] + [dict(B=0), dict(n_class=0), dict(n_class=256), dict(w=6), dict(w=0), dict(h=0)]
    bad += [{n: off(p[n], 8)} for n in names if n not in ("table", "sel")] + [dict(sel=off(p["sel"], 4))]
    for kw in bad:
        assert lib.segmif_class_mix_apply_f32(*aargs(**kw)) == -22, kw
    del keep


BASE = ["--class-mix"]
REFUSED = [(["--class-mix-prob", "0.5"], "--class-mix,"), (["--class-mix-min-pixels", "3"], "--class-mix,"),
           (["--class-mix-classes", "half"], "--class-mix,"), (["--class-mix-phases", "both"], "--class-mix,"),
           (BASE + ["--class-mix-prob", "0"], "--class-mix-prob 0.0: must lie"), (BASE + ["--class-mix-prob", "1.5"], "--class-mix-prob 1.5: must lie"),
           (BASE + ["--class-mix-prob", "nan"], "--class-mix-prob nan: must lie"),
           (BASE + ["--class-mix-min-pixels", "-1"], "--class-mix-min-pixels -1: must be"),
           (BASE + ["--class-mix-classes", "wanted"], "--class-mix-classes wanted pastes"),
           (BASE + ["--class-mix-classes", "wanted", "--rare-class-sampling", "--class-mix-phases", "both"], "the fusion phase has no rare-class sampling"),
           (BASE + ["--class-mix-classes", "wanted", "--rare-class-sampling", "--rcs-phases", "fusion"], "the seg phase has no rare-class sampling"),
           (BASE + ["--class-mix-classes", "all"], "invalid choice"), (BASE + ["--class-mix-phases", "val"], "invalid choice"),
           (BASE + ["--samples-per-gpu", "2"], "--samples-per-gpu 2: the loaders"), (BASE + ["--samples-per-gpu", "3"], "--samples-per-gpu 3: the loaders"),
           # (what needs no device is refused before the device check too)
           (["--root", "somewhere"], "give either --root DIR --name-lists DIR or --synthetic N"),
           (["--fusion-loss", "Nothing"], "--fusion-loss Nothing: one of Fusionloss"), (["--backbone", "mit_b0"], "--backbone mit_b0: Fusion_Network3_ac")]


@pytest.mark.parametrize("argv,needle", REFUSED)
def test_train_refuses_before_the_device_check(argv, needle, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--synthetic", "4"] + argv)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "error:" in err and needle in err


def test_train_refuses_a_root_without_name_lists_before_the_device_check(capsys):
    """(the one refusal the cases above cannot reach: they all train on --synthetic frames)"""
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--root", "somewhere"])
    assert exc.value.code == 2 and "error: --root needs --name-lists" in capsys.readouterr().err


def test_command_line_help_names_the_flags(capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    for flag in ("--class-mix ", "--class-mix-prob P", "--class-mix-min-pixels N", "--class-mix-classes {half,wanted}",
                 "--class-mix-phases {seg,fusion,both}", "NOT the reference's loader"):
        assert flag in out, flag
    assert out.count("NOT the reference's loader") >= 2  # rare-class sampling's and this one
