"""GPU tests of the device data path: csrc/augment.hip against what the reference's loader produced (tests/golden/augment.npz)
and against the integer numpy model (tests/_augment_ref.py), the iterator's output contract, one training step of each kind
on an augmented batch, and the training command line.  Everything the kernels compute is integers or one correctly rounded
division, so every comparison here is bit equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import data
    return data


def run_kernels(data, ds, indices, params, crop):
    """-> host arrays ir3, vis3, mask3, label and the (B, 3) chosen (box_h, box_w, index) the pick kernel wrote; the record's
    per-candidate `accepted` bits are compared with the numpy model's here"""
    h, w = ds.shape
    rec, tab = data.pack_records(indices, params, h, w)
    ir3, vis3, mask3, label, rec_d = ds.augment(rec, tab, crop, crop)
    torch.cuda.synchronize()
    assert ir3.dtype == vis3.dtype == mask3.dtype == torch.float32 and label.dtype == torch.int64
    r = rec_d.cpu().numpy()
    assert (r[:, data._TICKET] == 0).all() and (r[:, data._AMASK] == 0).all()
    src_label = ds.label.cpu().numpy()
    assert [int(v) for v in r[:, data._ACCEPTED]] == [ar.accepted_mask(src_label[i], p, crop) for i, p in zip(indices, params)]
    return ir3.cpu().numpy(), vis3.cpu().numpy(), mask3.cpu().numpy(), label.cpu().numpy(), r[:, [data._BOXH, data._BOXW, data._CHOSEN]]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_kernels_against_the_reference_loader(data, golden_dir):
    """All samples of the fixture as ONE batch: the four outputs equal the arrays the reference's __getitem__ returned, bit for
    bit (torch.equal), and the pick kernel kept the box the reference kept."""
    g = np.load(os.path.join(golden_dir, "augment.npz"))
    ds = data.DeviceDataset.from_arrays([f"f{i}" for i in range(len(g["frames_ir"]))], g["frames_ir"], g["frames_vis"], g["frames_mask"],
                                        g["frames_label"])
    n = len(g["frame"])
    params = []
    for i in range(n):
        p = {k: g[k][i] for k in ar.PARAM_KEYS}
        p.update(nw=int(p["nw"]), nh=int(p["nh"]), H=max(64, int(p["nh"])), W=max(64, int(p["nw"])), pad_h=int(p["pad_h"]), pad_w=int(p["pad_w"]),
                 cand=[tuple(int(v) for v in c) for c in p["cand"]], beta=float(p["beta"]), alpha=float(p["alpha"]))
        params.append(p)
    h, w = ds.shape
    rec, tab = data.pack_records([int(f) for f in g["frame"]], params, h, w)
    ir3, vis3, mask3, label, rec_d = ds.augment(rec, tab, 64, 64)
    for got, key in ((ir3, "ir3"), (vis3, "vis3"), (mask3, "mask3")):
        assert torch.equal(got.cpu(), torch.from_numpy(g[key])), key
        assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(g[key]).view(torch.int32)), key
    assert torch.equal(label.cpu(), torch.from_numpy(g["label"].astype(np.int64)))
    r = rec_d.cpu().numpy()
    assert np.array_equal(r[:, [data._BOXH, data._BOXW]], g["box"])
    assert np.array_equal(r[:, data._CHOSEN], g["drawn"] - 1)
    assert [int(v) for v in r[:, data._ACCEPTED]] == [ar.accepted_mask(g["frames_label"][int(f)], p, 64) for f, p in zip(g["frame"], params)]


RATIO_SETS = {"fixed": [0.5, 0.73, 1.0, 1.2345, 2.0, 0.5, 2.0, 1.0], "seeded": None}


@pytest.mark.parametrize("which", sorted(RATIO_SETS))
def test_kernels_against_the_numpy_model_at_full_size(data, which):
    """480 x 640 -> 512, batch 8: the given ratios and seeded random ones; outputs and boxes equal the numpy model exactly."""
    rng = np.random.default_rng(11 if which == "fixed" else 12)
    src = data.synthetic_pairs(4, 480, 640, seed=21)
    src["label"][1][:] = 4          # a uniform map: all ten candidates rejected
    src["label"][2][:, :600] = 255  # mostly unlabelled
    ds = data.DeviceDataset.from_arrays(**src)
    ratios = RATIO_SETS[which] or [float(r) for r in rng.uniform(0.5, 2.0, 8)]
    idx = [int(i) for i in rng.integers(0, 4, 8)]
    idx[:3] = [0, 1, 2]
    params = [ar.random_params(rng, 480, 640, 512, r) for r in ratios]
    ir3, vis3, mask3, label, boxes = run_kernels(data, ds, idx, params, 512)
    picked = set()
    for b, (i, p) in enumerate(zip(idx, params)):
        want = ar.transform(src["ir"][i], src["vis"][i], src["mask"][i], src["label"][i], p, 512)
        assert tuple(boxes[b]) == want[4] + (want[5],), (b, p["ratio"])
        assert same_bits(ir3[b], want[0]) and same_bits(vis3[b], want[1]) and same_bits(mask3[b], want[2]), (b, p["ratio"])
        assert np.array_equal(label[b], want[3]), (b, p["ratio"])
        picked.add(want[5])
    assert 9 in picked  # (the uniform map)


def test_small_and_odd_geometry(data):
    """Frames whose sides are not multiples of the tile, a crop that is not a multiple of it either, shrink by almost 4."""
    rng = np.random.default_rng(13)
    src = data.synthetic_pairs(3, 37, 53, seed=22)
    ds = data.DeviceDataset.from_arrays(**src)
    for crop, ratios in ((20, [0.3, 0.5, 1.0, 3.1]), (100, [0.3, 1.9, 2.7, 1.0])):
        params = [ar.random_params(rng, 37, 53, crop, r) for r in ratios]
        idx = [0, 1, 2, 1]
        ir3, vis3, mask3, label, boxes = run_kernels(data, ds, idx, params, crop)
        for b, (i, p) in enumerate(zip(idx, params)):
            want = ar.transform(src["ir"][i], src["vis"][i], src["mask"][i], src["label"][i], p, crop)
            assert tuple(boxes[b]) == want[4] + (want[5],)
            assert same_bits(ir3[b], want[0]) and same_bits(vis3[b], want[1]) and same_bits(mask3[b], want[2]), (crop, b)
            assert np.array_equal(label[b], want[3])


def test_iterator_contract(data):
    """(names, ir3, vis3, mask3, label): layout, dtypes, shapes, value ranges, determinism per seed; aug=False hands the frames over."""
    src = data.synthetic_pairs(6, 96, 128, seed=23)
    ds = data.DeviceDataset.from_arrays(**src)
    it = data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3)
    names, ir3, vis3, mask3, label = next(it)
    assert names == tuple(src["names"][:4])
    for t in (ir3, vis3, mask3):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (4, 3, 64, 64) and t.is_contiguous()
        assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    assert label.is_cuda and label.dtype == torch.int64 and tuple(label.shape) == (4, 64, 64)
    assert set(np.unique(label.cpu().numpy())) <= set(range(9)) | {255}
    again = next(data.AugmentedBatches(ds, batch=4, crop_size=64, seed=3))
    assert all(torch.equal(a, b) for a, b in zip((ir3, vis3, mask3, label), again[1:]))
    other = next(data.AugmentedBatches(ds, batch=4, crop_size=64, seed=4))
    assert not torch.equal(other[2], vis3)
    assert next(it)[0] == tuple(src["names"][:4])  # 6 frames, batch 4: the partial batch is dropped and the pass starts again
    plain = next(data.AugmentedBatches(ds, batch=2, aug=False))
    assert tuple(plain[2].shape) == (2, 3, 96, 128) and tuple(plain[4].shape) == (2, 96, 128)
    f32 = lambda a: torch.from_numpy(a.astype(np.float32) / np.float32(255.0))
    assert torch.equal(plain[2].cpu(), f32(src["vis"][:2]).permute(0, 3, 1, 2))
    assert torch.equal(plain[1].cpu(), f32(src["ir"][:2])[:, None].expand(-1, 3, -1, -1))
    assert torch.equal(plain[3].cpu(), f32(src["mask"][:2])[:, None].expand(-1, 3, -1, -1))
    assert torch.equal(plain[4].cpu(), torch.from_numpy(src["label"][:2].astype(np.int64)))


def test_training_steps_on_an_augmented_batch(data):
    """One seg_train_step and one FusionTrainer.step (mit_b1, the smallest backbone whose 64/128-channel features
    the fusion net takes; crop 64) on a batch of the iterator: finite losses."""
    import detweights as dw
    import segmif_amd.core as core
    from segmif_amd import train
    from segmif_amd.train import FusionTrainer, seg_train_step
    torch.manual_seed(0)
    seg, fus = core.Network3("mit_b1", 9, pretrained=None), core.Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0), dw.load_det_weights(fus, seed=0)
    seg, fus = seg.cuda().train(), fus.cuda().train()
    ds = data.DeviceDataset.from_arrays(**data.synthetic_pairs(4, 96, 128, seed=24))
    it = data.AugmentedBatches(ds, batch=2, crop_size=64, seed=1)
    opt_seg, opt_fus = train.make_seg_optimizer(seg, max_iter=10), train.make_fusion_optimizer(fus, iter_=2, max_iter=10)
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    _, ir3, vis3, mask3, label = next(it)
    loss_f = FusionTrainer(seg, fus, opt_fus, crit, iter_=2).step(ir3, vis3, mask3, label)
    _, ir3, vis3, mask3, label = next(it)
    loss_s = seg_train_step(seg, opt_seg, vis3, label, crit)
    assert torch.isfinite(loss_f).item() and torch.isfinite(loss_s).item(), (loss_f, loss_s)


def test_train_command_line(data, tmp_path, golden_dir):
    """python -m segmif_amd.train in a fresh child process on synthetic frames: it says so, finishes, and leaves both
    checkpoints with the reference's state_dict keys."""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "16", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "SYNTHETIC" in r.stdout
    keys = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    seg_sd = torch.load(tmp_path / "model-fusion_add_final2.pth", map_location="cpu")
    fus_sd = torch.load(tmp_path / "modelfusion-final2.pth", map_location="cpu")
    for sd, table in ((fus_sd, keys["Fusion_Network3_ac"]), (seg_sd, keys["Network3:mit_b1"])):
        assert sorted(sd) == sorted(table)
        assert all(list(sd[k].shape) == list(table[k]) for k in table)
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
