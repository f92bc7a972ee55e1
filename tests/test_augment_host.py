"""Host-side checks of the device data path (segmif_amd/data.py): Pillow's resize tables against Pillow itself, the numpy model
of the whole transform (tests/_augment_ref.py) against what the reference's loader produced (tests/golden/augment.npz), the
parameter sampling, the iterator's order and the refusals.  No kernel is launched here."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import _augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [0.5, 0.51, 0.6180339, 0.73, 0.75, 0.9, 0.999, 1.0, 1.001, 1.1, 1.2345, 1.3333333, 1.5, 1.61803, 1.75, 1.9, 1.99, 2.0]


@pytest.fixture(scope="module")
def data():
    from segmif_amd import data
    return data


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def apply_table(img, table, axis):
    """one pass with a table of the package: rows of (first index, tap count, weights)"""
    return ar._pass(img, [(int(r[0]), [int(k) for k in r[2:2 + r[1]]]) for r in table], axis)


def package_resize(data, img, nw, nh):
    a = img[:, :, None] if img.ndim == 2 else img
    h, w = a.shape[:2]
    a = apply_table(a, data.bilinear_table(w, nw)[1], 1)  # (the identity table of an unchanged axis goes through the same code)
    a = apply_table(a, data.bilinear_table(h, nh)[1], 0)
    return a[:, :, 0] if img.ndim == 2 else a


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_bilinear_tables_against_pillow(data, mode):
    """segmif_amd.data.bilinear_table applied in integers equals Image.resize(BILINEAR) on every pixel, over a sweep of ratios."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    h, w = 96, 128
    img = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
    for ratio in RATIOS:
        nw, nh = int(ratio * w), int(ratio * h)
        want = np.asarray(Image.fromarray(img).resize((nw, nh), resample=Image.BILINEAR))
        assert np.array_equal(package_resize(data, img, nw, nh), want), ratio
        assert np.array_equal(ar.resize_bilinear(img, nw, nh), want), ratio


def test_nearest_tables_against_pillow(data):
    """nearest_table equals Image.resize(NEAREST) at 480 x 640 over 45 ratios, 0.73 among them (where (x + 0.5) a is wrong)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    h, w = 480, 640
    lab = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for ratio in sorted(set(np.round(np.linspace(0.5, 2.0, 44), 4).tolist() + [0.73])):
        nw, nh = int(ratio * w), int(ratio * h)
        want = np.asarray(Image.fromarray(lab).resize((nw, nh), resample=Image.NEAREST))
        got = lab[data.nearest_table(h, nh)][:, data.nearest_table(w, nw)]
        assert np.array_equal(got, want), ratio
        assert np.array_equal(ar.resize_nearest(lab, nw, nh), want), ratio


def test_package_tables_equal_the_loop_model(data):
    """The vectorised builders and the line-by-line model give the same integers (this one needs no Pillow)."""
    for n_in in (60, 80, 480, 641):
        for ratio in RATIOS + [0.2501, 3.9]:
            n_out = int(ratio * n_in)
            taps, t = data.bilinear_table(n_in, n_out)
            assert t.dtype == np.int32 and t.shape == (n_out, 2 + taps)
            if n_out != n_in:
                ref = ar.coeffs(n_in, n_out)
                assert [int(r[0]) for r in t] == [lo for lo, _ in ref]
                assert [[int(k) for k in r[2:2 + r[1]]] for r in t] == [ks for _, ks in ref]
                assert all((r[2 + r[1]:] == 0).all() for r in t) and (t[:, 0] + t[:, 1] <= n_in).all() and (t[:, 1] >= 1).all()
            assert np.array_equal(data.nearest_table(n_in, n_out), ar.nearest_index(n_in, n_out))
            assert data.nearest_table(n_in, n_out).max() < n_in


def golden_params(g, i):
    return {k: g[k][i] for k in ar.PARAM_KEYS}


def test_numpy_model_against_the_reference_loader(golden):
    """tests/_augment_ref.transform on the stored frames and draws equals, bit for bit, the four arrays the reference's own
    __getitem__ returned, and picks the box it picked."""
    n = len(golden["frame"])
    assert n >= 8
    for i in range(n):
        f = int(golden["frame"][i])
        ir3, vis3, mask3, label, box, chosen = ar.transform(golden["frames_ir"][f], golden["frames_vis"][f], golden["frames_mask"][f],
                                                            golden["frames_label"][f], golden_params(golden, i), 64)
        assert box == tuple(golden["box"][i]) and chosen == int(golden["drawn"][i]) - 1, i
        for got, key in ((ir3, "ir3"), (vis3, "vis3"), (mask3, "mask3")):
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), golden[key][i].view(np.int32)), (i, key)
        assert np.array_equal(label, golden["label"][i].astype(np.int64)), i


def test_the_fixture_covers_what_it_should(golden):
    g = golden
    ratio = g["ratio"]
    assert 0.5 in ratio and 2.0 in ratio and ((ratio > 0.5) & (ratio < 1)).any() and ((ratio > 1) & (ratio < 2)).any()
    pad_h, pad_w = g["nh"] < 64, g["nw"] < 64
    assert (pad_h & pad_w).any() and (pad_h ^ pad_w).any() and (~pad_h & ~pad_w).any()
    for coin in ("flip", "bright_on", "contrast_on"):
        assert g[coin].any() and not g[coin].all(), coin
    assert (g["beta"] > 25).any() and (g["beta"] < -25).any()
    assert ((g["drawn"] > 1) & (g["drawn"] < 10)).any() and (g["drawn"] == 10).sum() >= 2
    assert any((g["frames_label"][int(f)] == 255).all() for f in g["frame"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "augment.npz")) < 2 ** 20


def test_record_layout_matches_c(data):
    """The word offsets segmif_amd.data packs records with are those of the C struct's ctypes mirror (which
    tests/test_abi_and_host.py::test_struct_layouts_match_c holds to the header, field by field)."""
    from segmif_amd._lib import SegmifAugmentRec as R
    fields = {"src": data._SRC, "h": data._H, "w": data._W, "nw": data._NW, "nh": data._NH, "flip": data._FLIP, "bright_on": data._BON,
              "beta": data._BETA, "contrast_on": data._CON, "alpha": data._ALPHA, "pad_h": data._PADH, "pad_w": data._PADW,
              "H": data._CH, "W": data._CW, "cand": data._CAND, "box_h": data._BOXH, "box_w": data._BOXW, "chosen": data._CHOSEN,
              "ticket": data._TICKET, "accept_mask": data._AMASK, "accepted": data._ACCEPTED, "tab_x": data._TABX, "tab_y": data._TABY,
              "near_x": data._NEARX, "near_y": data._NEARY, "taps_x": data._TAPSX, "taps_y": data._TAPSY}
    assert ctypes.sizeof(R) == 4 * data.REC_WORDS
    for name, word in fields.items():
        assert getattr(R, name).offset == 4 * word, name


def test_pack_records(data):
    p = data.sample_params(random.Random(3), np.random.RandomState(3), 60, 80, 64, 64)
    q = data.sample_params(random.Random(4), np.random.RandomState(4), 60, 80, 64, 64)
    rec, tab = data.pack_records([5, 2], [p, q], 60, 80)
    assert rec.shape == (2, data.REC_WORDS) and rec.dtype == np.int32 and tab.dtype == np.int32 and tab.ndim == 1
    for r, (src, s) in zip(rec, ((5, p), (2, q))):
        assert r[data._SRC] == src and (r[data._NW], r[data._NH]) == (s["nw"], s["nh"]) and r[data._TICKET] == 0 and r[data._AMASK] == 0
        assert r[data._BETA:data._BETA + 1].view(np.float32)[0] == np.float32(s["beta"])
        tx, bx = data.bilinear_table(80, s["nw"])
        assert r[data._TAPSX] == tx and np.array_equal(tab[r[data._TABX]:r[data._TABX] + bx.size], bx.reshape(-1))
        assert np.array_equal(tab[r[data._NEARY]:r[data._NEARY] + s["nh"]], data.nearest_table(60, s["nh"]))
        assert np.array_equal(r[data._CAND:data._CAND + 20].reshape(10, 2), np.asarray(s["cand"]))
    with pytest.raises(RuntimeError, match="in / out"):
        data.pack_records([0], [dict(p, nw=10, nh=10)], 60, 80)


def test_parameter_ranges_and_determinism(data):
    h, w, crop = 480, 640, 512
    draws = [data.sample_params(random.Random(s), np.random.RandomState(s), h, w, crop, crop) for s in range(300)]
    again = [data.sample_params(random.Random(s), np.random.RandomState(s), h, w, crop, crop) for s in range(300)]
    assert draws == again
    assert draws[0] != draws[1]
    for p in draws:
        assert 0.5 <= p["ratio"] <= 2.0 and (p["nw"], p["nh"]) == (int(p["ratio"] * w), int(p["ratio"] * h))
        assert (p["H"], p["W"]) == (max(crop, p["nh"]), max(crop, p["nw"]))
        assert 0 <= p["pad_h"] <= p["H"] - p["nh"] and 0 <= p["pad_w"] <= p["W"] - p["nw"]
        assert len(p["cand"]) == 10 and all(0 <= a <= p["H"] - crop and 0 <= b <= p["W"] - crop for a, b in p["cand"])
        assert -32 <= p["beta"] <= 32 and 0.5 <= p["alpha"] <= 1.5
        assert p["bright_on"] or p["beta"] == 0.0
        assert p["contrast_on"] or p["alpha"] == 1.0
    for coin in ("flip", "bright_on", "contrast_on"):
        share = np.mean([p[coin] for p in draws])
        assert 0.35 < share < 0.65, (coin, share)  # 300 fair tosses: 0.5 +- 5 sigma (sigma = 0.029) lies inside
    off = data.sample_params(random.Random(0), np.random.RandomState(0), h, w, crop, crop, rescale_range=None, fliplr=False, photometric=())
    assert off["ratio"] == 1.0 and not off["flip"] and not off["bright_on"] and not off["contrast_on"]


class StubSet:
    """what AugmentedBatches asks of a data set, without a device"""

    def __init__(self, n, shape=(60, 80)):
        self.names, self.shape = [f"n{i}" for i in range(n)], shape

    def __len__(self):
        return len(self.names)


def stub_batches(data, n, **kw):
    it = data.AugmentedBatches(StubSet(n), **kw)
    it._device_step = lambda idx, params: (list(idx), [p["ratio"] for p in params], None, None)
    return it


def test_batches_order_drop_last_restart_and_ranks(data):
    it = stub_batches(data, 11, batch=4, crop_size=64, seed=7)
    assert len(it) == 2
    out = [next(it) for _ in range(5)]
    assert [o[1] for o in out] == [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3]]  # no shuffle, 8..10 dropped
    assert out[0][0] == ("n0", "n1", "n2", "n3") and len(out[0]) == 5
    assert out[0][2] != out[2][2]  # the second pass draws new parameters
    from segmif_amd.dist import shard
    seen = []
    for rank in range(3):
        r = stub_batches(data, 11, batch=2, crop_size=64, seed=7, rank=rank, world=3)
        assert r.indices == list(shard(11, rank, 3))
        seen += r.indices
        first = next(r)
        assert first[1] == r.indices[:2]
    assert sorted(seen) == list(range(11))
    a, b = stub_batches(data, 11, batch=2, crop_size=64, seed=7, rank=0, world=3), stub_batches(data, 11, batch=2, crop_size=64, seed=7, rank=1, world=3)
    assert next(a)[2] != next(b)[2]  # ranks draw from different streams
    with pytest.raises(RuntimeError, match="fewer than one batch"):
        stub_batches(data, 3, batch=4, crop_size=64)


def test_batches_are_deterministic_and_leave_the_global_generators_alone(data):
    random.seed(123)
    np.random.seed(123)
    torch.manual_seed(123)
    before = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    runs = []
    for _ in range(2):
        it = stub_batches(data, 8, batch=4, crop_size=64, seed=5)
        runs.append([next(it)[2] for _ in range(4)])
        params = it.last_params
    assert runs[0] == runs[1] and len(params) == 4
    assert runs[0][0] != next(stub_batches(data, 8, batch=4, crop_size=64, seed=6))[2]  # first batch of seed 5 against seed 6's
    assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
    assert torch.equal(torch.get_rng_state(), before[2])
    plain = stub_batches(data, 8, batch=4, crop_size=64, aug=False)
    next(plain)
    assert all(p["ratio"] == 1.0 and (p["nw"], p["nh"]) == (80, 60) and p["box"] == (0, 0) for p in plain.last_params)


def test_unknown_photometric_names_are_refused(data):
    for bad in (("saturation",), ("brightness", "hue")):
        with pytest.raises(ValueError, match="saturation and hue"):
            data.AugmentedBatches(StubSet(4), batch=2, photometric=bad)
    data.AugmentedBatches(StubSet(4), batch=2, photometric=("contrast",))
    with pytest.raises(ValueError):
        data.AugmentedBatches(StubSet(4), batch=2, crop_size=30)


def test_cpu_tensors_are_refused(data):
    from segmif_amd import ops
    u = lambda *s: torch.zeros(s, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="on the MI355X device"):
        data.DeviceDataset(["a", "b"], u(2, 8, 8), u(2, 8, 8, 3), u(2, 8, 8), u(2, 8, 8))
    rec, tab = torch.zeros((1, ops.AUGMENT_REC_WORDS), dtype=torch.int32), torch.zeros(64, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="on the MI355X device"):
        ops.augment_pick(u(2, 8, 8), rec, tab, 8, 8)
    with pytest.raises(RuntimeError, match="on the MI355X device"):
        ops.augment_apply(u(2, 8, 8), u(2, 8, 8, 3), u(2, 8, 8), u(2, 8, 8), rec, tab, 8, 8)
    assert ops.AUGMENT_REC_WORDS == data.REC_WORDS


def write_folder(root, names, size=(12, 16), odd=None):
    rng = np.random.default_rng(0)
    frames = {}
    for sub in ("Infrared", "Visible", "Mask2", "Label"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for n in names:
        h, w = odd[1] if odd and n == odd[0] else size
        frames[n] = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
                     rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 9, (h, w), dtype=np.uint8))
        for sub, a in zip(("Infrared", "Visible", "Mask2", "Label"), frames[n]):
            np.save(os.path.join(root, sub, n + ".npy"), a)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    return frames


def test_pair_folder(data, tmp_path):
    names = ["00003D", "00001N", "00002D"]
    frames = write_folder(str(tmp_path), names)
    pf = data.PairFolder(str(tmp_path), str(tmp_path), "train")
    assert len(pf) == 3 and pf.names == names  # the list's order, not the directory's
    for i, n in enumerate(names):
        item = pf[i]
        assert item[0] == n and all(a.dtype == np.uint8 for a in item[1:])
        assert all(np.array_equal(a, b) for a, b in zip(item[1:], frames[n]))
    data.stack_same_size([pf[i] for i in range(3)])
    with pytest.raises(FileNotFoundError):
        data.PairFolder(str(tmp_path), str(tmp_path), "val")
    os.remove(tmp_path / "Mask2" / "00001N.npy")
    with pytest.raises(FileNotFoundError, match="Mask2"):
        pf[1]


def test_pair_folder_reads_png(data, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    frames = write_folder(str(tmp_path), ["a"])
    for sub, a in zip(("Infrared", "Visible", "Mask2", "Label"), frames["a"]):
        os.remove(tmp_path / sub / "a.npy")
        Image.fromarray(a).save(tmp_path / sub / "a.png")
    item = data.PairFolder(str(tmp_path), str(tmp_path))[0]
    assert all(np.array_equal(a, b) for a, b in zip(item[1:], frames["a"]))


def test_frames_of_different_sizes_are_refused(data, tmp_path):
    write_folder(str(tmp_path), ["a", "b", "c"], odd=("c", (12, 20)))
    pf = data.PairFolder(str(tmp_path), str(tmp_path))
    with pytest.raises(RuntimeError, match="ONE size: c has a 12 x 20"):
        data.stack_same_size([pf[i] for i in range(3)])


def test_synthetic_pairs(data):
    a, b, c = data.synthetic_pairs(3, 48, 64, seed=1), data.synthetic_pairs(3, 48, 64, seed=1), data.synthetic_pairs(3, 48, 64, seed=2)
    assert a["ir"].shape == (3, 48, 64) and a["vis"].shape == (3, 48, 64, 3) and a["mask"].shape == a["label"].shape == (3, 48, 64)
    assert all(a[k].dtype == np.uint8 for k in ("ir", "vis", "mask", "label")) and len(a["names"]) == 3
    assert all(np.array_equal(a[k], b[k]) for k in ("ir", "vis", "mask", "label")) and not np.array_equal(a["vis"], c["vis"])
    assert a["label"].max() <= 8 and len(np.unique(a["label"])) >= 2
    # blocky labels: most horizontal neighbours are equal; image-like: neighbouring pixels correlate
    assert (a["label"][:, :, 1:] == a["label"][:, :, :-1]).mean() > 0.9
    v = a["vis"].astype(np.float64)
    assert np.corrcoef(v[:, :, 1:].ravel(), v[:, :, :-1].ravel())[0, 1] > 0.8


def test_plain_hand_over_refuses_a_width_that_is_not_a_multiple_of_4(data):
    """aug=False writes whole rows with 16-byte stores: refused when the iterator is built, not at the first batch"""
    with pytest.raises(ValueError, match="multiple of 4"):
        data.AugmentedBatches(StubSet(4, shape=(60, 82)), batch=2, aug=False)
    data.AugmentedBatches(StubSet(4, shape=(60, 82)), batch=2, crop_size=64)  # (the augmented path crops: any width)
