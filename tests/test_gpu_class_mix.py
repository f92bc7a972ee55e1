"""GPU tests of ClassMix: csrc/class_mix.hip (segmif_class_mix_select, segmif_class_mix_apply_f32) through ops.class_mix against
the numpy restatement of the rule (tests/_class_mix_ref.py), the mixed iterator against the restatement applied to an unmixed
twin, and the training command line with the new flags.  Integers and float BITS only: every comparison is equality."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _class_mix_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODD = (255, -1, 256, 2 ** 40 + 3)  # values that are no class, whatever their low byte


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import data
    return data


def _bits(t):
    return t.view(torch.int32).cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def run_labels(rng, B, h, w, n_class):
    """(B, h, w) int64: runs of 1 to 9 equal pixels along the rows, so that groups of 4 pixels come whole and split"""
    flat = np.empty(B * h * w, dtype=np.int64)
    at = 0
    while at < flat.size:
        n = int(rng.integers(1, 10))
        flat[at:at + n] = int(rng.integers(0, n_class))
        at += n
    return flat.reshape(B, h, w)


def bit_planes(rng, B, h, w):
    """three (B, 3, h, w) int32 arrays of random bit patterns (NaNs of every payload among them), with -0.0, a quiet and a
    signalling NaN with payloads and an infinity placed by hand in every sample"""
    planes = [rng.integers(0, 2 ** 32, (B, 3, h, w), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    for p in planes:
        flat = p.reshape(B, -1)
        flat[:, 0], flat[:, 5], flat[:, 10], flat[:, 15] = 0x80000000, 0x7FC12345, 0xFFA00001, 0x7F800000
    return [p.view(np.int32) for p in planes]


def keys_table(rng, donors, n_class, force=None):
    rows = [[d, -1 if force is None else force[b]] + rng.permutation(n_class).tolist() for b, d in enumerate(donors)]
    return np.asarray(rows, dtype=np.int32)


# name: (B, h, w), donors, samples expected to mix, whether a group of every kind is required
APPLY_CASES = {
    "2x4x4_one_group_a_row": ((2, 4, 4), [1, 0], [0, 1], False),
    "3x5x8": ((3, 5, 8), [1, 2, 0], [0, 1, 2], True),
    "2x33x68_rows_across_waves_and_blocks": ((2, 33, 68), [1, 0], [0, 1], True),
    "4x64x256_blocks_a_sample": ((4, 64, 256), [1, 2, 3, 0], [0, 1, 2, 3], True),
    "4x64x256_unmixed_sample_and_empty_donor": ((4, 64, 256), [1, 3, 0, 3], [0, 2], True),
}


def apply_inputs(case):
    (B, h, w), donors, mixing, kinds = APPLY_CASES[case]
    rng = np.random.default_rng(sorted(APPLY_CASES).index(case) + 100)
    label = run_labels(rng, B, h, w, 9)
    if case.startswith("4x64x256_unmixed"):
        label[3] = 255  # sample 1's donor holds no class at all; sample 3 itself is not mixed (donor == b)
    if h * w >= 40:
        for b in range(B):  # values outside the classes, by hand, in every crop
            at = rng.choice(h * w, 8, replace=False)
            label[b].reshape(-1)[at] = ODD + ODD
    else:
        label[1, 3, :] = ODD
    return label, bit_planes(rng, B, h, w), keys_table(rng, donors, 9), mixing, kinds


def expected(label, planes, table, n_class, min_pixels):
    cnt = mr.counts(label, n_class)
    sel, pasted, chosen = mr.select(cnt, table, n_class, min_pixels)
    out, lab, M = mr.apply(planes, label, table[:, 0], sel)
    return cnt, sel, pasted, chosen, out, lab, M


def on_device(label, planes, table, n_class=9, min_pixels=0, tally=None):
    from segmif_amd import ops
    lab_d = torch.from_numpy(label).cuda()
    pl_d = [torch.from_numpy(p).cuda().view(torch.float32) for p in planes]
    keep = [t.clone() for t in pl_d + [lab_d]]
    got = ops.class_mix(*pl_d, lab_d, table, n_class, min_pixels, tally)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(pl_d + [lab_d], keep))  # out of place: the inputs equal their clones
    assert all(o.data_ptr() != i.data_ptr() for o, i in zip(got[:4], pl_d + [lab_d]))
    return got


def same(got, out, lab, sel, pasted):
    ir3, vis3, mask3, label, sel_d, pasted_d = got
    assert sel_d.dtype == torch.int32 and tuple(sel_d.shape) == sel.shape and pasted_d.dtype == torch.int64 and label.dtype == torch.int64
    assert np.array_equal(sel_d.cpu().numpy(), sel)
    assert np.array_equal(pasted_d.cpu().numpy(), pasted)
    assert np.array_equal(label.cpu().numpy(), lab)
    for t, o in zip((ir3, vis3, mask3), out):
        assert t.dtype == torch.float32 and np.array_equal(t.view(torch.int32).cpu().numpy(), o)


@pytest.mark.parametrize("case", sorted(APPLY_CASES))
def test_apply_equals_the_restatement(data, case):
    label, planes, table, mixing, kinds = apply_inputs(case)
    B, h, w = label.shape
    cnt, sel, pasted, chosen, out, lab, M = expected(label, planes, table, 9, 0)
    # the inputs reach every path of the kernel: whole groups from the donor, whole groups from the receiver, split groups
    assert set(int(v) for v in label.reshape(-1)) >= set(ODD)
    assert np.array_equal(M.reshape(B, -1).sum(axis=1), pasted)
    for b in range(B):
        per_group = M[b].reshape(-1, 4).sum(axis=1)
        if b in mixing:
            assert 0 < pasted[b] < h * w, (b, pasted[b])
            if kinds:
                assert (per_group == 0).any() and (per_group == 4).any() and ((per_group > 0) & (per_group < 4)).any(), b
        else:
            assert pasted[b] == 0 and not chosen[b] and np.array_equal(lab[b], label[b])
    got = on_device(label, planes, table)
    same(got, out, lab, sel, pasted)
    again = on_device(label, planes, table)  # a second call returns equal bits
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


def _select(counts, table, n_class, min_pixels, tally=None):
    """segmif_class_mix_select alone, on a count table made by hand"""
    from segmif_amd import _lib
    B = len(table)
    cnt = torch.zeros((B, 257), dtype=torch.int64)
    cnt[:, :counts.shape[1]] = torch.from_numpy(np.asarray(counts, dtype=np.int64))
    cnt, tab = cnt.cuda(), torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
    sel = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
    pasted = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    err = _lib.load().segmif_class_mix_select(cnt.data_ptr(), tab.data_ptr(), B, n_class, min_pixels, sel.data_ptr(), pasted.data_ptr(),
                                              tally.data_ptr() if tally is not None else None,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert err == 0
    return sel.cpu().numpy(), pasted.cpu().numpy()


KEYS = [8, 0, 7, 1, 6, 2, 5, 3, 4]


def test_select_hand_cases_on_the_device(data):
    """The cases of test_class_mix_host, on the device, each also against the restatement; the tally adds up over the calls."""
    five, four, one, none, edge = [10, 20, 30, 40, 50, 0, 0, 0, 0], [5, 0, 6, 0, 7, 0, 8, 0, 0], [0] * 7 + [3, 0], [0] * 9, [0, 0, 7, 8, 0, 100, 0, 0, 0]
    counts = np.asarray([five, four, one, none, edge], dtype=np.int64)
    tally = torch.zeros((9, 2), dtype=torch.int64, device="cuda")
    tally[8, 1] = 5  # (the call adds to the tally, it does not reset it)
    want_tally = np.zeros((9, 2), dtype=np.int64)
    want_tally[8, 1] = 5
    row = lambda d, force=-1: [d, force] + KEYS
    for min_pixels, table, by_hand in (
            (0, [row(1), row(0), row(3), row(2), row(4)], [[4, 6], [1, 3, 4], [], [7], []]),   # 4 -> 2, 5 -> 3, none, 1 -> 1, donor == b
            (7, [row(4), row(4, 5), row(4, 2), row(4, 4), row(0)], [[3], [5], [], [], [1, 3, 4]]),  # n == min_pixels absent; force
            (6, [row(4), row(1), row(2), row(3), row(3)], [[3, 5], [], [], [], []])):
        table = np.asarray(table, dtype=np.int32)
        sel, pasted, chosen = mr.select(counts, table, 9, min_pixels)
        assert chosen == by_hand
        got_sel, got_pasted = _select(counts, table, 9, min_pixels, tally)
        assert np.array_equal(got_sel, sel) and np.array_equal(got_pasted, pasted)
        want_tally += mr.tally(counts, table, chosen, 9)
        assert np.array_equal(tally.cpu().numpy(), want_tally)
    # a donor outside 0..B-1 is treated as donor == b (the wrapper refuses it; the entry point cannot see it)
    got_sel, got_pasted = _select(counts, np.asarray([row(7), row(-3), row(0), row(1), row(2)]), 9, 0)
    assert not got_sel[:2].any() and not got_pasted[:2].any() and got_sel[2:].any(axis=1).all()


def test_select_on_crop_labels_one_class_and_255_classes(data):
    from segmif_amd import ops
    rng = np.random.default_rng(7)
    # B = 5, 9 classes, counts taken from real crop labels through ops.label_stats (inside ops.class_mix)
    src = data.synthetic_pairs(5, 96, 128, seed=31)
    ds = data.DeviceDataset.from_arrays(**src)
    it = data.AugmentedBatches(ds, batch=5, crop_size=64, seed=2)
    _, ir3, vis3, mask3, label = next(it)
    lab = label.cpu().numpy()
    table = keys_table(rng, [1, 2, 3, 4, 0], 9)
    planes = [t.view(torch.int32).cpu().numpy() for t in (ir3, vis3, mask3)]
    for min_pixels in (0, 300):
        cnt, sel, pasted, chosen, out, mixed, M = expected(lab, planes, table, 9, min_pixels)
        assert np.array_equal(ops.label_stats(label).cpu().numpy()[:, :9], cnt)
        tally = torch.zeros((9, 2), dtype=torch.int64, device="cuda")
        got = ops.class_mix(ir3, vis3, mask3, label, table, 9, min_pixels, tally)
        same(got, out, mixed, sel, pasted)
        assert np.array_equal(tally.cpu().numpy(), mr.tally(cnt, table, chosen, 9)) and pasted.sum() > 0
        assert np.array_equal(M.reshape(5, -1).sum(axis=1), pasted)  # pasted is the mask's popcount
    # one class: present iff the donor holds a 0; k = 1
    lab1 = np.where(rng.random((3, 4, 8)) < 0.5, 0, 255).astype(np.int64)
    lab1[2] = 255
    planes1 = bit_planes(rng, 3, 4, 8)
    table1 = np.asarray([[1, -1, 0], [2, -1, 0], [0, 0, 0]], dtype=np.int32)
    cnt, sel, pasted, chosen, out, mixed, M = expected(lab1, planes1, table1, 1, 0)
    assert chosen == [[0], [], [0]]
    same(on_device(lab1, planes1, table1, n_class=1), out, mixed, sel, pasted)
    # 255 classes, labels up to 254: word 7 of sel
    lab255 = rng.integers(0, 255, (2, 16, 64)).astype(np.int64)
    lab255[0, 0, :4] = 254
    lab255[1, 0, :4] = (254, 255, 256, 254 + 256)
    planes255 = bit_planes(rng, 2, 16, 64)
    table255 = keys_table(rng, [1, 0], 255)
    for row in table255:  # class 254 gets the smallest key
        j = int(np.nonzero(row[2:] == 0)[0][0])
        row[2 + j], row[2 + 254] = row[2 + 254], 0
    assert (np.sort(table255[:, 2:], axis=1) == np.arange(255)).all()
    tally = torch.zeros((255, 2), dtype=torch.int64, device="cuda")
    cnt, sel, pasted, chosen, out, mixed, M = expected(lab255, planes255, table255, 255, 0)
    assert all(254 in c for c in chosen) and (sel.view(np.uint32)[:, 7] >> 30 & 1).all() and all(len(c) > 64 for c in chosen)
    same(on_device(lab255, planes255, table255, n_class=255, tally=tally), out, mixed, sel, pasted)
    assert np.array_equal(tally.cpu().numpy(), mr.tally(cnt, table255, chosen, 255))


def test_wrapper_refuses_what_the_kernels_cannot_take(data):
    from segmif_amd import ops
    label, planes, table, _, _ = apply_inputs("3x5x8")
    lab = torch.from_numpy(label).cuda()
    ir3, vis3, mask3 = (torch.from_numpy(p).cuda().view(torch.float32) for p in planes)
    ops.class_mix(ir3, vis3, mask3, lab, table)
    wide = torch.zeros((3, 3, 5, 16), device="cuda")
    with pytest.raises(RuntimeError):
        ops.class_mix(wide[..., ::2], vis3, mask3, lab, table)  # not contiguous
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3[..., :6].contiguous(), vis3[..., :6].contiguous(), mask3[..., :6].contiguous(), lab[..., :6].contiguous(), table)
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3.double(), vis3, mask3, lab, table)
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3.cpu(), vis3, mask3, lab, table)
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3, vis3, mask3, lab.int(), table)
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3, vis3[:2].contiguous(), mask3, lab, table)
    with pytest.raises(ValueError):
        ops.class_mix(ir3, vis3, mask3, lab, table[:, :-1])  # a host table of the wrong width
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3, vis3, mask3, lab, torch.from_numpy(table[:, :-1].copy()).cuda())  # and one on the device
    with pytest.raises(ValueError):
        ops.class_mix(ir3, vis3, mask3, lab, np.asarray([[5, -1] + list(range(9))] * 3))  # a donor outside the batch
    with pytest.raises(RuntimeError):
        ops.class_mix(ir3, vis3, mask3, lab, table, tally=torch.zeros((8, 2), dtype=torch.int64, device="cuda"))


def _frames(data):
    src = data.synthetic_pairs(16, 96, 128, seed=27)
    return src, data.DeviceDataset.from_arrays(**src)


def _check_iterators(data, src, ds, mixed_it, twin_it, forced):
    total = np.zeros((9, 2), dtype=np.int64)
    pasted_any = 0
    for _ in range(3):
        names, ir3, vis3, mask3, label = next(mixed_it)
        t_names, t_ir3, t_vis3, t_mask3, t_label = next(twin_it)
        assert names == t_names
        plain = [{k: v for k, v in p.items() if k != "mix"} for p in mixed_it.last_params]
        assert repr(plain) == repr(twin_it.last_params)  # the crops underneath are the ones the same seed gives without mixing
        table = np.asarray([[p["mix"][0], p["mix"][1]] + list(p["mix"][2]) for p in mixed_it.last_params], dtype=np.int32)
        assert (table[:, 0] != np.arange(4)).all()  # prob = 1
        if forced:
            assert [int(f) for f in table[:, 1]] == [mixed_it.last_params[int(d)]["want"][0] for d in table[:, 0]]
        else:
            assert (table[:, 1] == -1).all()
        lab, planes = t_label.cpu().numpy(), [_bits(t) for t in (t_ir3, t_vis3, t_mask3)]
        cnt, sel, pasted, chosen, out, want_label, M = expected(lab, planes, table, 9, 0)
        assert np.array_equal(label.cpu().numpy(), want_label)
        for t, o in zip((ir3, vis3, mask3), out):
            assert np.array_equal(_bits(t), o)
        total += mr.tally(cnt, table, chosen, 9)
        pasted_any += int(pasted.sum())
        assert np.array_equal(mixed_it.mix_tally(), total)
        if not forced:  # the twin's batches are what dataset.augment gives directly
            idx = [src["names"].index(n) for n in t_names]
            direct = ds.augment(*data.pack_records(idx, twin_it.last_params, 96, 128), 64, 64)[:4]
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(direct, (t_ir3, t_vis3, t_mask3, t_label)))
    assert pasted_any > 0


def test_mixed_iterator_equals_the_restatement_on_its_twin(data):
    src, ds = _frames(data)
    _check_iterators(data, src, ds, data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3, mix=data.ClassMix(prob=1.0, seed=3)),
                     data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3), forced=False)
    stats = ds.label_stats()
    sampler = lambda: data.RareClassSampler(stats, range(16), min_pixels=200, fraction=0.75, seed=5)
    _check_iterators(data, src, ds,
                     data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3, sampler=sampler(), mix=data.ClassMix(prob=1.0, classes="wanted", seed=3)),
                     data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3, sampler=sampler()), forced=True)
    for kw in (dict(batch=1, mix=data.ClassMix()), dict(batch=4, aug=False, mix=data.ClassMix()),
               dict(batch=4, mix=data.ClassMix(classes="wanted")), dict(batch=4, mix=data.ClassMix(rank=1))):
        with pytest.raises(ValueError):
            data.AugmentedBatches(ds, crop_size=64, **kw)
    with pytest.raises(RuntimeError):
        data.AugmentedBatches(ds, batch=4, crop_size=64).mix_tally()


@pytest.mark.parametrize("classes", ["half", "wanted"])
def test_train_command_line_with_class_mix(data, tmp_path, classes):
    """python -m segmif_amd.train in a fresh child process: the arguments of test_gpu_class_balance's command plus ClassMix."""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "16", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path),
           "--rare-class-sampling", "--rcs-min-pixels", "16", "--seg-loss", "weighted", "--seg-class-weights-from", "median",
           "--class-mix", "--class-mix-prob", "1.0"] + (["--class-mix-classes", "wanted"] if classes == "wanted" else [])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = r.stdout
    announced = [ln for ln in out.splitlines() if ln.startswith("[train] --class-mix (")]
    assert len(announced) == 1 and "NOT the reference's loader" in announced[0] and f"classes {classes}" in announced[0]
    seg_lines = [ln for ln in out.splitlines() if "segmentation iter 2/2" in ln]
    assert len(seg_lines) == 1 and " mix sel/px " in seg_lines[0] and " rcs drawn/hit " in seg_lines[0]
    fields = seg_lines[0].split(" mix sel/px ")[1].split()
    if fields != ["none"]:
        pairs = [f.split(":")[1].split("/") for f in fields]
        assert all(int(s) >= 1 and int(px) >= 1 for s, px in pairs)
        assert sum(int(px) for _, px in pairs) < 4 * 64 * 64  # 2 iterations of batch 2
    assert not any(" mix " in ln for ln in out.splitlines() if "fusion iter" in ln)  # --class-mix-phases defaults to seg
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
