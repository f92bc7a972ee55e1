"""GPU tests of the class-balance path: csrc/label_stats.hip against np.bincount, the second pick rule of csrc/augment.hip
(segmif_augment_pick_class_u8) against its numpy restatement (tests/_class_balance_ref.py) and against the crops apply cuts, the
sampled iterator, and the training command line with the new flags.  Everything compared is integers: every comparison is
equality."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ar
import _class_balance_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import data
    return data


def _offset_slice(rng):
    """(2, 33, 65) frames that start one byte into a larger tensor: neither frame begins on a 16-byte line"""
    big = torch.from_numpy(rng.integers(0, 256, 2 * 33 * 65 + 40, dtype=np.uint8)).cuda()
    return big[1:1 + 2 * 33 * 65].view(2, 33, 65)


COUNT_CASES = {
    "u8_3x7x13": lambda rng: torch.from_numpy(rng.integers(0, 256, (3, 7, 13), dtype=np.uint8)).cuda(),
    "u8_1x1x1": lambda rng: torch.full((1, 1, 1), 200, dtype=torch.uint8).cuda(),
    "u8_2x33x65": lambda rng: torch.from_numpy(rng.integers(0, 9, (2, 33, 65), dtype=np.uint8)).cuda(),
    "u8_offset_slice": _offset_slice,
    "u8_constant_64x64": lambda rng: torch.full((1, 64, 64), 3, dtype=torch.uint8).cuda(),
    "u8_blocky_two_blocks_a_frame": lambda rng: torch.from_numpy(np.repeat(rng.integers(0, 9, (3, 300, 11), dtype=np.uint8), 31, axis=2)).cuda(),
    "i64_2x5x9": lambda rng: torch.from_numpy(np.where(rng.random((2, 5, 9)) < 0.3, rng.choice([-1, 256, 1000], (2, 5, 9)),
                                                       rng.integers(0, 256, (2, 5, 9))).astype(np.int64)).cuda(),
    "i64_odd_start": lambda rng: torch.from_numpy(rng.integers(-3, 12, 1 + 3 * 17 * 29).astype(np.int64)).cuda()[1:].view(3, 17, 29),
}


@pytest.mark.parametrize("case", sorted(COUNT_CASES))
def test_counts_equal_bincount(data, case):
    from segmif_amd import ops
    label = COUNT_CASES[case](np.random.default_rng(31))
    assert label.is_contiguous()
    got = ops.label_stats(label)
    assert got.dtype == torch.int64 and tuple(got.shape) == (label.shape[0], 257) and got.is_cuda
    want = cr.counts(label.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want)
    if case.startswith("u8"):
        assert not want[:, 256].any()
    if case == "i64_2x5x9":
        assert want[:, 256].all() and {-1, 256, 1000} <= set(label.cpu().numpy().reshape(-1).tolist())
    again = ops.label_stats(label)  # (the call zeroes its output itself: no carry-over)
    assert torch.equal(again, got)


def test_counts_of_a_frame_longer_than_2_to_the_31(data):
    """Element indices past 2^31 in one frame: the values are placed by hand, so the expected table needs no host pass."""
    from segmif_amd import ops
    n = 2 ** 31 + 21
    label = torch.zeros((1, 1, n), dtype=torch.uint8, device="cuda")
    label[0, 0, -3:] = 5
    label[0, 0, 2 ** 31 - 1] = 7
    label[0, 0, 2 ** 31] = 7
    got = ops.label_stats(label)[0].cpu().numpy()
    want = np.zeros(257, dtype=np.int64)
    want[0], want[5], want[7] = n - 5, 3, 2
    assert np.array_equal(got, want)


def _upload(data, idx, params, h, w):
    rec, tab = data.pack_records(idx, params, h, w)
    return torch.from_numpy(rec).cuda(), torch.from_numpy(tab).cuda()


def test_unwanted_samples_match_the_old_pick(data):
    """want = -1 on the samples of test_gpu_augment.test_small_and_odd_geometry's kind: every word of the record equals what
    segmif_augment_pick_u8 writes on the same records, got is -1, and the tally is not touched."""
    from segmif_amd import ops
    rng = np.random.default_rng(13)
    src = data.synthetic_pairs(3, 37, 53, seed=22)
    label = torch.from_numpy(src["label"]).cuda()
    for crop, ratios in ((20, [0.3, 0.5, 1.0, 3.1]), (100, [0.3, 1.9, 2.7, 1.0])):
        params = [ar.random_params(rng, 37, 53, crop, r) for r in ratios]
        idx = [0, 1, 2, 1]
        rec_a, tab = _upload(data, idx, params, 37, 53)
        rec_b = rec_a.clone()
        tally = torch.zeros((9, 2), dtype=torch.int64, device="cuda")
        ops.augment_pick(label, rec_a, tab, crop, crop)
        got = ops.augment_pick_class(label, rec_b, tab, crop, crop, [[-1, 0]] * 4, tally)
        assert torch.equal(rec_a, rec_b)
        assert got.dtype == torch.int32 and got.cpu().tolist() == [-1] * 4
        assert not tally.any()
        r = rec_b.cpu().numpy()
        for b, (i, p) in enumerate(zip(idx, params)):
            chosen, box, mask, _, _ = cr.pick_class(src["label"][i], p, crop, -1, 0)
            assert (int(r[b, data._CHOSEN]), (int(r[b, data._BOXH]), int(r[b, data._BOXW])), int(r[b, data._ACCEPTED])) == (chosen, box, mask)


def _wanted_batch(data):
    """24 x 40 frames, crop 16, ratios 0.5 (padding), 1.0 and 1.7, with and without flip.  Per geometry: the first accepted
    candidate (t one below the largest count), no candidate accepted with a constructed tie (t the largest count, the best
    window entered twice), a class that is nowhere, a sample without a wanted class, and t = 0."""
    rng = np.random.default_rng(41)
    src = data.synthetic_pairs(3, 24, 40, seed=25)
    lab = src["label"]
    lab[lab == 8] = 1                 # class 8 is nowhere
    lab[0][5:15, 8:26] = 5
    lab[1][2:9, 20:38] = 5
    lab[2][12:22, 3:14] = 5
    lab[2][0:6, 30:36] = 3
    idx, params, wants, kinds = [], [], [], []
    for ratio in (0.5, 1.0, 1.7):
        for flip in (False, True):
            i = len(idx) % 3
            p = ar.random_params(rng, 24, 40, 16, ratio)
            p["flip"] = flip
            n = [int((win == 5).sum()) for win in cr.windows(lab[i], p, 16)]
            assert max(n) > 0
            tie = dict(p, cand=list(p["cand"]))
            k = int(np.argmax(n))
            tie["cand"][9 if k < 9 else 0] = tie["cand"][k]  # the best window a second time, at another index
            for kind, q, want in (("first", p, (5, max(n) - 1)), ("tie", tie, (5, max(n))), ("absent", p, (8, 0)), ("plain", p, (-1, 0)),
                                  ("any", p, (5, 0)), ("three", p, (3, 2))):
                idx.append(i), params.append(q), wants.append(want), kinds.append(kind)
    return src, idx, params, wants, kinds


def test_wanted_samples_match_the_restatement_and_the_crops(data):
    src, idx, params, wants, kinds = _wanted_batch(data)
    ds = data.DeviceDataset.from_arrays(**src)
    rec, tab = data.pack_records(idx, params, 24, 40)
    tally = torch.zeros((9, 2), dtype=torch.int64, device="cuda")
    tally[2, 0] = 11  # (the call adds to the tally, it does not reset it)
    _, _, _, label, rec_d, got = ds.augment(rec, tab, 16, 16, want=np.asarray(wants), tally=tally)
    r, got, label = rec_d.cpu().numpy(), got.cpu().numpy(), label.cpu().numpy()
    assert (r[:, data._TICKET] == 0).all() and (r[:, data._AMASK] == 0).all() and (r[:, 46:48] == 0).all()
    hits, seen = [], set()
    for b, (i, p, (c, t), kind) in enumerate(zip(idx, params, wants, kinds)):
        chosen, box, mask, n, hit = cr.pick_class(src["label"][i], p, 16, c, t)
        have = (int(r[b, data._CHOSEN]), (int(r[b, data._BOXH]), int(r[b, data._BOXW])), int(r[b, data._ACCEPTED]), int(got[b]))
        assert have == (chosen, box, mask, n), (b, kind, p["ratio"], p["flip"])
        hits.append(hit)
        if c >= 0:
            assert int((label[b] == c).sum()) == got[b], (b, kind)  # what apply cut holds what pick counted
        counts = [int((win == c).sum()) for win in cr.windows(src["label"][i], p, 16)]
        if kind == "first":
            assert hit and counts[chosen] == t + 1 and all(v <= t for v in counts[:chosen])  # t rejects a window of t pixels, t - 1 ...
        elif kind == "tie":
            assert not hit and mask == 0 and counts.count(max(counts)) >= 2 and chosen == counts.index(max(counts)) and n == t
        elif kind == "absent":
            assert (chosen, n, mask) == (0, 0, 0)
        elif kind == "plain":
            assert n == -1
        seen.add((kind, hit))
    assert {("first", True), ("tie", False), ("absent", False), ("any", True)} <= seen
    want_tally = cr.tally(wants, hits, 9)
    want_tally[2, 0] += 11
    assert np.array_equal(tally.cpu().numpy(), want_tally)


def test_threshold_is_strict_on_one_window(data):
    """One sample, all ten candidates the SAME window of n pixels: t = n rejects every one (mask 0, candidate 0, got n),
    t = n - 1 accepts every one (mask 1023, candidate 0)."""
    from segmif_amd import ops
    src, idx, params, _, _ = _wanted_batch(data)
    label = torch.from_numpy(src["label"]).cuda()
    p0, i = params[12], idx[12]  # ratio 1.0
    assert p0["ratio"] == 1.0
    k = int(np.argmax([(win == 5).sum() for win in cr.windows(src["label"][i], p0, 16)]))
    p = dict(p0, cand=[p0["cand"][k]] * 10)
    n = int((cr.windows(src["label"][i], p, 16)[0] == 5).sum())
    assert n > 1
    for t, mask in ((n, 0), (n - 1, 1023)):
        rec, tab = _upload(data, [i], [p], 24, 40)
        got = ops.augment_pick_class(label, rec, tab, 16, 16, [[5, t]])
        r = rec.cpu().numpy()[0]
        assert (int(r[data._ACCEPTED]), int(r[data._CHOSEN]), int(got[0])) == (mask, 0, n)


def test_wrapper_refuses_what_the_device_cannot(data):
    from segmif_amd import ops
    src, idx, params, _, _ = _wanted_batch(data)
    label = torch.from_numpy(src["label"]).cuda()
    rec, tab = _upload(data, idx[:2], params[:2], 24, 40)
    for bad in ([[255, 0], [1, 0]], [[1, -1], [1, 0]], [[1, 0]]):
        with pytest.raises(ValueError):
            ops.augment_pick_class(label, rec, tab, 16, 16, bad)
    ds = data.DeviceDataset.from_arrays(**src)
    with pytest.raises(ValueError):
        ds.augment(*data.pack_records(idx[:2], params[:2], 24, 40), 16, 16, want=[[300, 0], [1, 0]])


def _painted_set(data):
    src = data.synthetic_pairs(12, 96, 128, seed=26)
    src["label"][src["label"] == 8] = 1
    src["label"][3][10:50, 20:70] = 8   # class 8 lives in two frames only
    src["label"][7][60:90, 5:45] = 8
    return src


def test_sampled_iterator(data):
    from segmif_amd import ops
    src = _painted_set(data)
    ds = data.DeviceDataset.from_arrays(**src)
    stats = ds.label_stats()
    assert np.array_equal(stats.counts, cr.counts(src["label"])[:, :9]) and stats.frames[8] == 2
    table = ds._label_counts
    assert np.array_equal(ds.label_stats().counts, stats.counts) and ds._label_counts is table  # one readback, kept
    make = lambda: data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3,
                                         sampler=data.RareClassSampler(stats, range(12), min_pixels=200, fraction=0.75, seed=5))
    it, again = make(), make()
    assert it.sampler.candidates[8] == [3, 7]
    drawn, classes = 0, set()
    for _ in range(8):
        names, ir3, vis3, mask3, label = next(it)
        assert tuple(vis3.shape) == (4, 3, 64, 64) and label.dtype == torch.int64 and tuple(label.shape) == (4, 64, 64)
        batch_counts = ops.label_stats(label)  # the int64 entry on a produced batch
        assert np.array_equal(batch_counts.cpu().numpy(), cr.counts(label.cpu().numpy()))
        for name, p in zip(names, it.last_params):
            frame, (c, t) = src["names"].index(name), p["want"]
            if c >= 0:
                assert frame in it.sampler.candidates[c]
                assert t == math.floor(200 * 0.5 * (p["nw"] * p["nh"]) / (128 * 96))
                drawn += 1
                classes.add(c)
            else:
                assert (c, t) == (-1, 0)
        other = next(again)
        assert other[0] == names and all(torch.equal(a, b) for a, b in zip((ir3, vis3, mask3, label), other[1:]))
    tally = it.rcs_tally()
    assert tally.dtype == np.int64 and tally.shape == (9, 2)
    assert tally[:, 0].sum() == drawn and 0 < drawn < 32 and (tally[:, 1] <= tally[:, 0]).all()
    assert set(np.nonzero(tally[:, 0])[0].tolist()) == classes
    with pytest.raises(ValueError):
        data.AugmentedBatches(ds, batch=4, crop_size=64, sampler=data.RareClassSampler(stats, range(8), min_pixels=200))
    bad = _painted_set(data)
    bad["label"][5][0, 0] = 9
    with pytest.raises(ValueError, match=r"frame 5 .* value 9"):
        data.DeviceDataset.from_arrays(**bad).label_stats()


def test_train_command_line_with_class_balance(data, tmp_path):
    """python -m segmif_amd.train in a fresh child process: the arguments of test_gpu_augment.test_train_command_line plus
    rare-class sampling and weights computed from the labels."""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "16", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path),
           "--rare-class-sampling", "--rcs-min-pixels", "16", "--seg-loss", "weighted", "--seg-class-weights-from", "median"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = r.stdout
    assert "--rare-class-sampling" in out and "NOT the reference's loader" in out
    assert "classes of the synthetic labels" in out and "labelled pixels" in out and "--seg-class-weights-from median:" in out and "candidate frames per class:" in out
    seg_lines = [ln for ln in out.splitlines() if "segmentation iter 2/2" in ln]
    assert len(seg_lines) == 1 and " rcs drawn/hit " in seg_lines[0]
    pairs = [f.split(":")[1].split("/") for f in seg_lines[0].split(" rcs drawn/hit ")[1].split()]
    assert sum(int(d) for d, _ in pairs) == 4 and all(int(h) <= int(d) for d, h in pairs)  # 2 iterations of batch 2, all sampled
    assert not any(" rcs " in ln for ln in out.splitlines() if "fusion iter" in ln)  # --rcs-phases defaults to seg
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
