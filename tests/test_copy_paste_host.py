"""CPU-only checks of instance copy-paste (csrc/copy_paste.hip behind ops.object_boxes / object_pack / copy_paste, data.ObjectBank and
data.CopyPaste, the --copy-paste flags; ABI in include/segmif_paste.h).  No kernel is launched here.

  - the restatement tests/_copy_paste_ref.py: its cases worked by hand, and its boxes against scipy.ndimage.find_objects per class
  - the header's part of what tests/test_abi_and_host.py and tests/test_abi_contract_host.py check for every header: the symbols it
    is expected to declare, its constants against _lib and ops, workspace_bytes, and cases of its EINVAL list in the contract table
  - CopyPaste.draw: a fixed number of draws per sample, centres inside the crop, steps and sizes within the kernel's domain for boxes of
    1 and of 4096, reproducible from the seed and different per rank; ops.check_paste_table
  - the parser's errors and the unchanged default plan"""
import os
import random
import types

import numpy as np
import pytest

import _abi_contract_table as table
import _abi_headers as headers
import _copy_paste_ref as ref
import _objects_ref as objects_ref
from test_abi_contract_host import check_rejected, records  # noqa: F401 - the fixture: the contract child's records


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------

def test_the_restatement_holds_its_cases_worked_by_hand():
    ref.self_checks()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["7x5", "65x129", "serpentine_130", "checkerboard_66", "blocky_K32", "odd_labels", "all_ign"])
def test_restated_boxes_against_scipy_find_objects(name, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    c = objects_ref.case(name, conn)
    K = c["K"]
    label = np.where((c["label"] >= 0) & (c["label"] < K), c["label"], 255).astype(np.uint8)
    root = ref.roots_of(label, K, conn)
    assert np.array_equal(root, c["root_g"])
    got = ref.boxes(root, label, K, 0xffffffff, 1, 1 << 40)
    structure = np.ones((3, 3), dtype=int) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    want = []
    for f in range(len(label)):
        W = label.shape[2]
        for cls in range(K):
            lab, n = ndi.label(label[f] == cls, structure=structure)
            for i, (sy, sx) in enumerate(ndi.find_objects(lab)):
                ys, xs = np.where(lab == i + 1)
                want.append((f, int((ys * W + xs).min()), cls, len(ys), sx.start, sy.start, sx.stop - sx.start, sy.stop - sy.start))
    assert got.tolist() == [list(r) for r in sorted(want)]
    # the filters: each of the three alone
    for kw in (dict(class_mask=0b10), dict(min_area=5), dict(max_box=9)):
        full = {**dict(class_mask=0xffffffff, min_area=1, max_box=1 << 40), **kw}
        sub = ref.boxes(root, label, K, full["class_mask"], full["min_area"], full["max_box"])
        keep = [r for r in got.tolist() if (full["class_mask"] >> r[2]) & 1 and r[3] >= full["min_area"] and r[6] * r[7] <= full["max_box"]]
        assert sub.tolist() == keep


def test_the_patch_store_holds_the_object_alone():
    """two interlocking combs of one class: each box holds pixels of the other, and alpha leaves them out"""
    label = np.zeros((1, 9, 12), dtype=np.uint8)
    label[0, 0, :11] = 3
    label[0, 0:6, 0:11:4] = 3        # teeth down
    label[0, 8, 1:] = 3
    label[0, 3:9, 2:12:4] = 3        # teeth up
    root = ref.roots_of(label, 9, 4)
    rec = ref.boxes(root, label, 9, 0b1000, 1, 1000)
    assert len(rec) == 2 and rec[0, 4:].tolist() == [0, 0, 11, 6] and rec[1, 4:].tolist() == [1, 3, 11, 6]
    rng = np.random.default_rng(0)
    ir, mask, vis = rng.integers(1, 256, (1, 9, 12), dtype=np.uint8), rng.integers(1, 256, (1, 9, 12), dtype=np.uint8), rng.integers(1, 256, (1, 9, 12, 3), dtype=np.uint8)
    off = ref.offsets_of(rec)
    patches = ref.pack(rec, off, root, ir, vis, mask)
    for m in range(2):
        px = patches[off[m]:off[m + 1]].reshape(6, 11, 8)
        assert int(px[..., 5].sum()) == rec[m, 3]                      # alpha counts the object's area, not the class's pixels in the box
        assert (label[0, rec[m, 5]:rec[m, 5] + 6, rec[m, 4]:rec[m, 4] + 11] == 3).sum() > rec[m, 3]
        assert not px[px[..., 5] == 0].any() and (px[px[..., 5] == 1][:, :5] > 0).all() and not px[..., 6:].any()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_these_symbols_and_its_source_is_built():
    from segmif_amd import build
    assert headers.declared("segmif_paste.h") == ["segmif_copy_paste_f32", "segmif_object_boxes_i32", "segmif_object_boxes_workspace_bytes",
                                                  "segmif_object_pack_u8"]
    assert "copy_paste.hip" in build.SOURCES


def test_the_constants_are_the_headers(tmp_path):
    from segmif_amd import _lib, ops
    names = ["RECORD_WORDS", "MAX_SLOTS", "MAX_SIZE", "MAX_STEP", "MAX_FRAMES", "WORKSPACE_PER_PIXEL"]
    defs = dict(zip(names, headers.c_ints("segmif_paste.h", ["SEGMIF_PASTE_" + n for n in names], tmp_path)))
    assert defs["RECORD_WORDS"] == _lib.PASTE_RECORD_WORDS == ops.PASTE_WORDS == ref.WORDS == 8
    assert defs["MAX_SLOTS"] == _lib.PASTE_MAX_SLOTS == ops.PASTE_MAX_SLOTS == ref.MAX_SLOTS
    assert defs["MAX_SIZE"] == _lib.PASTE_MAX_SIZE == ops.PASTE_MAX_SIZE == ref.MAX_SIZE == 4096
    assert defs["MAX_STEP"] == _lib.PASTE_MAX_STEP == ops.PASTE_MAX_STEP == ref.MAX_STEP == 2 ** 24
    assert defs["MAX_FRAMES"] == _lib.PASTE_MAX_FRAMES and defs["WORKSPACE_PER_PIXEL"] == _lib.PASTE_WORKSPACE_PER_PIXEL


def test_workspace_bytes_is_positive_for_legal_sizes_and_zero_for_refused_ones(lib):
    size = lib.segmif_object_boxes_workspace_bytes
    assert size(1, 1, 1) == 20 and size(3, 65, 129) == 3 * 65 * 129 * 20 and size(32767, 1, 1) > 0
    assert size(1, 46340, 46340) == 46340 * 46340 * 20
    for n, H, W in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (32768, 1, 1), (1, 65536, 32768), (1, 46341, 46341)):
        assert size(n, H, W) == 0, (n, H, W)


# ---- rejections: the cases of the header's EINVAL list, each a row of tests/_abi_contract_table.py that the contract child sent -------

MUTATIONS = {
    "segmif_object_boxes_i32": [("root", None), ("label", None), ("counter", None), ("workspace", None), ("records", None),
                                ("K", 0), ("K", -1), ("K", 33), ("min_area", 0), ("min_area", -3), ("max_box", 0), ("capacity", -1),
                                ("frame0", -1), ("frame0", 2 ** 31 - 2), ("n", 0), ("n", -2), ("n", 32768), ("H", 0), ("W", 0), ("W", -53),
                                ("HW", (65536, 32768)), ("HW", (46341, 46341))],
    "segmif_object_pack_u8": [("records", None), ("offsets", None), ("root", None), ("ir", None), ("vis", None), ("mask", None),
                              ("patches", None), ("M", 0), ("M", -1), ("store_pixels", -1), ("frame0", -1), ("n", 0), ("n", 32768),
                              ("H", 0), ("W", 0), ("HW", (65536, 32768))],
    "segmif_copy_paste_f32": [("ir3", None), ("vis3", None), ("mask3", None), ("label", None), ("records", None), ("offsets", None),
                              ("patches", None), ("table", None), ("ir3_out", None), ("vis3_out", None), ("mask3_out", None),
                              ("label_out", None), ("pasted", None), ("P", 9), ("P", -1), ("w", 10), ("w", 13), ("w", 0), ("h", 0), ("B", 0),
                              ("B", 65536), ("n_class", 0), ("n_class", 256), ("M", 0), ("store_pixels", 0),
                              ("ir3", 0x100004), ("label_out", 0xc00008)],  # a tensor 4 bytes, and 8 bytes, off its 16-byte alignment
}
CASES = [(entry, arg, value) for entry, muts in MUTATIONS.items() for arg, value in muts]


def test_the_cases_cover_the_headers_einval_list():
    boxes, paste = (set(MUTATIONS[k]) for k in ("segmif_object_boxes_i32", "segmif_copy_paste_f32"))
    assert {("K", 0), ("K", 33), ("capacity", -1), ("root", None), ("records", None)} <= boxes   # K outside 1..32, a negative capacity
    assert {("P", 9), ("w", 10), ("table", None), ("pasted", None)} <= paste                       # P > 8, w % 4


@pytest.mark.parametrize("case", CASES, ids=[f"{entry}:{arg}={value}" for entry, arg, value in CASES])
def test_rejected(records, case):
    entry, arg, value = case
    check_rejected(records, table.find(entry, ("H", "W") if arg == "HW" else arg, value))


# ---- the policy ---------------------------------------------------------------------------------------------------------------------------

def fake_bank(boxes=((3, 7), (1, 1), (4096, 4096), (40, 25), (9, 300)), classes=(1, 1, 2, 5, 5)):
    """what CopyPaste reads of an ObjectBank, on the host: records_host, by_class, n_class"""
    rec = np.zeros((len(boxes), 8), dtype=np.int32)
    rec[:, 2], rec[:, 6], rec[:, 7] = classes, [b[0] for b in boxes], [b[1] for b in boxes]
    return types.SimpleNamespace(records_host=rec, by_class={int(c): np.flatnonzero(rec[:, 2] == c) for c in np.unique(rec[:, 2])}, n_class=9)


def test_draw_takes_a_fixed_number_of_draws_per_sample_whatever_the_coins_show():
    from segmif_amd.data import CopyPaste
    for prob, n in ((1.0, 3), (0.01, 3), (0.5, 8), (0.5, 1)):
        cp = CopyPaste(fake_bank(), prob=prob, max_objects=n, seed=5, rank=2)
        assert cp.draws_per_sample() == 2 + 6 * n
        table = cp.draw(7, 64, 96)
        assert table.shape == (7, n, 8) and table.dtype == np.int32
        twin = random.Random("CopyPaste 5 2")
        for _ in range(7 * (2 + 6 * n)):
            twin.random()
        assert cp._py.getstate() == twin.getstate(), (prob, n)
    always, never = CopyPaste(fake_bank(), prob=1.0, seed=1).draw(50, 64, 64), CopyPaste(fake_bank(), prob=1e-9, seed=1).draw(50, 64, 64)
    assert (always[:, 0, 0] >= 0).all() and (never[:, :, 0] == -1).all() and not never[:, :, 1:].any()
    used = (always[:, :, 0] >= 0).sum(axis=1)
    assert set(used.tolist()) == {1, 2, 3}  # 1..max_objects objects, the used slots first
    assert all((row[:k, 0] >= 0).all() and (row[k:, 0] == -1).all() for row, k in zip(always, used))


def test_draw_keeps_centres_in_the_crop_and_slots_in_the_kernels_domain():
    from segmif_amd import ops
    from segmif_amd.data import CopyPaste
    bank = fake_bank()
    for scale, (h, w) in (((0.5, 2.0), (64, 96)), ((0.001, 0.002), (4, 4)), ((50.0, 100.0), (512, 512)), ((1.0, 1.0), (36, 68))):
        cp = CopyPaste(bank, prob=1.0, max_objects=8, scale=scale, seed=3)
        t = cp.draw(40, h, w).reshape(-1, 8)
        t = t[t[:, 0] >= 0]
        assert len(t) > 40 and set(t[:, 0].tolist()) <= set(range(5))
        obj, dx, dy, ow, oh, sx, sy, flip = t.T.astype(np.int64)
        bw, bh = bank.records_host[obj, 6], bank.records_host[obj, 7]
        assert (ow >= 1).all() and (ow <= ops.PASTE_MAX_SIZE).all() and (oh >= 1).all() and (oh <= ops.PASTE_MAX_SIZE).all()
        assert (sx >= 1).all() and (sx <= ops.PASTE_MAX_STEP).all() and (sy >= 1).all() and (sy <= ops.PASTE_MAX_STEP).all()
        assert (sx == np.clip((bw << 16) // ow, 1, ops.PASTE_MAX_STEP)).all() and (sy == np.clip((bh << 16) // oh, 1, ops.PASTE_MAX_STEP)).all()
        assert (0 <= dx + ow // 2).all() and (dx + ow // 2 <= w).all() and (0 <= dy + oh // 2).all() and (dy + oh // 2 <= h).all()
        assert (dx >= -(ow // 2)).all() and (dx <= w - ow + ow // 2).all() and (dy >= -(oh // 2)).all() and (dy <= h - oh + oh // 2).all()
        assert set(flip.tolist()) <= {0, 1}
        if scale == (1.0, 1.0):
            assert (ow == bw).all() and (oh == bh).all() and (sx == 65536).all() and set(flip.tolist()) == {0, 1}
            assert {0, 2}.issubset(set(obj.tolist()))  # boxes of 1 and of 4096 were drawn
        if scale == (50.0, 100.0):
            assert (ow[obj == 2] == 4096).all() and (sx[obj == 1] >= 1).all()  # clamped at 4096; a box of 1 at ow = 50..100: sx = 65536 // ow
        if scale == (0.001, 0.002):
            assert (ow[obj == 1] == 1).all() and (sx[obj == 2] == 2 ** 24).all()  # a box of 4096 at ow = 4..8: (4096 << 16) // ow clamps at 2^24
    assert not CopyPaste(bank, prob=1.0, flip=False, seed=3).draw(40, 64, 64)[:, :, 7].any()


def test_draw_is_reproducible_from_the_seed_and_differs_per_rank():
    from segmif_amd.data import CopyPaste, LabelStats
    a, b = CopyPaste(fake_bank(), prob=0.7, seed=11, rank=0), CopyPaste(fake_bank(), prob=0.7, seed=11, rank=0)
    first = a.draw(6, 64, 64)
    assert np.array_equal(first, b.draw(6, 64, 64)) and np.array_equal(a.draw(6, 64, 64), b.draw(6, 64, 64))
    assert not np.array_equal(first, CopyPaste(fake_bank(), prob=0.7, seed=11, rank=1).draw(6, 64, 64))
    assert not np.array_equal(first, CopyPaste(fake_bank(), prob=0.7, seed=12, rank=0).draw(6, 64, 64))
    state = random.getstate()
    a.draw(3, 64, 64)
    assert random.getstate() == state  # the global generator is not touched
    # the class draw: uniform over the banked classes, or the sampler's rule from the statistics
    assert a.class_prob == {1: 1 / 3, 2: 1 / 3, 5: 1 / 3}
    counts = np.zeros((1, 257), dtype=np.int64)
    counts[0, :9] = [900, 50, 30, 0, 0, 20, 0, 0, 0]
    st = CopyPaste(fake_bank(), stats=LabelStats(counts, ["f"], 9), temperature=0.05)
    z = np.exp((1 - np.array([0.05, 0.03, 0.02])) / 0.05)
    assert np.allclose([st.class_prob[c] for c in (1, 2, 5)], z / z.sum(), rtol=1e-12, atol=0)
    for bad in (dict(prob=0.0), dict(prob=1.5), dict(max_objects=0), dict(max_objects=9), dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)),
                dict(temperature=0.0)):
        with pytest.raises(ValueError, match="CopyPaste"):
            CopyPaste(fake_bank(), **bad)


def test_check_paste_table():
    from segmif_amd import ops
    ok = np.zeros((2, 3, 8), dtype=np.int64)
    ok[0, 0] = (5, -40, 70, 4097, 0, 2 ** 24 + 1, 0, 3)  # values outside the kernel's domain pass: such a slot is empty by the rule
    got = ops.check_paste_table(ok, 2)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, ok)
    assert ops.check_paste_table(np.zeros((2, 0, 8), dtype=np.int32), 2).shape == (2, 0, 8)
    assert ops.check_paste_table(np.zeros((1, 8, 8), dtype=np.int32), 1, P=8).shape == (1, 8, 8)
    for bad, B, P in ((np.zeros((2, 9, 8), np.int32), 2, None), (np.zeros((2, 3, 7), np.int32), 2, None), (np.zeros((3, 3, 8), np.int32), 2, None),
                      (np.zeros((2, 3, 8), np.float32), 2, None), (np.zeros((2, 24), np.int32), 2, None), (np.zeros((2, 3, 8), np.int32), 2, 4),
                      (np.full((2, 3, 8), 2 ** 31, np.int64), 2, None), (np.full((2, 3, 8), -2 ** 31 - 1, np.int64), 2, None)):
        with pytest.raises(ValueError, match="copy_paste"):
            ops.check_paste_table(bad, B, P)


def test_the_wrappers_and_the_iterator_fail_loudly_without_a_device():
    import torch
    from segmif_amd import ops
    z = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.copy_paste(z, z, z, torch.zeros(1, 4, 4, dtype=torch.int64), None, np.zeros((1, 0, 8), np.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.object_boxes(torch.zeros(1, 4, 4, dtype=torch.int32), None, 9, 1, 1, 1, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.object_pack(torch.zeros(1, 8, dtype=torch.int32), None, None, None, None, None, None)


# ---- the parser and the plan ----------------------------------------------------------------------------------------------------------------

BASE = ["--synthetic", "16", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2", "--backbone", "mit_b1", "--crop-size", "64",
        "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", "somewhere"]


def plan_of(argv, capsys=None):
    from segmif_amd import train
    ap = train.build_parser()
    args = ap.parse_args(argv)
    train.check_args(args, ap.error)
    train.resolve_defaults(args)
    return train.make_plan(args)


@pytest.mark.parametrize("flag,values", [("--copy-paste-prob", ["0.3"]), ("--copy-paste-max-objects", ["2"]), ("--copy-paste-classes", ["1", "2"]),
                                         ("--copy-paste-min-area", ["10"]), ("--copy-paste-scale", ["0.5", "1.5"]),
                                         ("--copy-paste-temperature", ["0.1"]), ("--copy-paste-phases", ["both"])])
def test_each_flag_without_the_switch_is_a_parser_error(flag, values, capsys):
    with pytest.raises(SystemExit) as e:
        plan_of(BASE + [flag] + values)
    assert e.value.code == 2 and f"{flag} belongs to --copy-paste, which is not given" in capsys.readouterr().err
    plan_of(BASE + ["--copy-paste", flag] + values)


@pytest.mark.parametrize("flag,values,text", [("--copy-paste-prob", ["0"], "(0, 1]"), ("--copy-paste-prob", ["1.2"], "(0, 1]"),
                                              ("--copy-paste-max-objects", ["0"], "1..8"), ("--copy-paste-max-objects", ["9"], "1..8"),
                                              ("--copy-paste-classes", ["9"], "0..8"), ("--copy-paste-classes", ["-1"], "0..8"),
                                              ("--copy-paste-min-area", ["0"], ">= 1"), ("--copy-paste-scale", ["2", "1"], "LO <= HI"),
                                              ("--copy-paste-scale", ["0", "1"], "LO <= HI"), ("--copy-paste-temperature", ["0"], "> 0"),
                                              ("--copy-paste-phases", ["none"], "invalid choice")])
def test_values_outside_their_ranges_are_parser_errors(flag, values, text, capsys):
    with pytest.raises(SystemExit) as e:
        plan_of(BASE + ["--copy-paste", flag] + values)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_the_plan_with_the_flag_and_the_unchanged_plan_without_it():
    off, on = plan_of(BASE), plan_of(BASE + ["--copy-paste"])
    assert sorted(vars(off)) == sorted(["batch", "guarded", "ema_seg", "ema_fus", "rcs_kw", "rcs_phases", "mix_kw", "mix_phases", "st_kw", "st_mix_kw",
                                        "fusion_opt_kw", "seg_opt_kw", "loader_kw", "fusion_iters", "seg_iters", "say"])
    assert not any("copy-paste" in line for line in off.say)
    assert sorted(set(vars(on)) - set(vars(off))) == ["paste_bank_kw", "paste_kw", "paste_phases"]
    assert {k: v for k, v in vars(on).items() if k not in ("say", "paste_bank_kw", "paste_kw", "paste_phases")} == {k: v for k, v in vars(off).items() if k != "say"}
    assert on.paste_phases == ("seg",) and on.paste_bank_kw == dict(n_class=9, classes=None, min_area=64)
    assert on.paste_kw == dict(prob=0.5, max_objects=3, scale=(0.5, 2.0), temperature=None)
    line = [l for l in on.say if l.startswith("[train] --copy-paste (")]
    assert len(line) == 1 and "NOT the reference's loader" in line[0] and "mIoU" in line[0] and "phases seg)" in line[0]
    assert on.say == off.say + line
    full = plan_of(BASE + ["--copy-paste", "--copy-paste-prob", "1.0", "--copy-paste-max-objects", "8", "--copy-paste-classes", "2", "5",
                           "--copy-paste-min-area", "9", "--copy-paste-scale", "0.25", "4", "--copy-paste-temperature", "0.02",
                           "--copy-paste-phases", "both", "--class-mix"])
    assert full.paste_phases == ("seg", "fusion") and full.paste_bank_kw == dict(n_class=9, classes=[2, 5], min_area=9)
    assert full.paste_kw == dict(prob=1.0, max_objects=8, scale=(0.25, 4.0), temperature=0.02) and full.mix_phases == ("seg",)
    from segmif_amd import train
    helptext = train.build_parser().format_help()
    assert "--copy-paste-phases" in helptext and "this project's choice" in helptext and "NOT the reference's loader" in helptext
