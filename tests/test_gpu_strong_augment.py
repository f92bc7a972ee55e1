"""GPU tests of the strong augmentation (csrc/strong_augment.hip through ops.strong_augment) against the numpy restatement of the
rule, tests/_strong_aug_ref.py, and of SelfTrainingStep(strong=).

Gate: max |y - ref64| <= 4 * max(e32, 2^-23), where ref64 is the restatement in float64 and e32 = max |ref32 - ref64| is what the
same code loses in float32 on the same case; 4x is this project's standing margin over torch-class float32 error.  `mean` is
held to the same bound against the float64 mean.  Equalities are through bits."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _strong_aug_ref as sr
import detweights as dw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.array([123.675, 116.28, 103.53], dtype=np.float32) / np.float32(255)  # augment_apply's mean-colour padding
VALUE_GATE = 1e-5  # (tests/test_gpu_self_training.py's)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import ops as o
    return o


def make_input(shape, quantised, seed):
    """random or 1/255-quantised values with a grey, a black, a primary-colour and a mean-colour-padding region"""
    B, _, h, w = shape
    rng = np.random.RandomState(seed)
    x = rng.rand(*shape).astype(np.float32)
    if quantised:
        x = (np.round(x * 255) / np.float32(255)).astype(np.float32)
    q = max(1, h // 4)
    x[:, :, :q, : w // 2] = x[:, :1, :q, : w // 2]          # grey
    x[:, :, :q, w // 2:] = 0.0                               # black
    for c in range(3):                                       # red, green, blue stripes
        x[:, :, q:2 * q, c * (w // 3):(c + 1) * (w // 3)] = 0.0
        x[:, c, q:2 * q, c * (w // 3):(c + 1) * (w // 3)] = 1.0
    x[:, :, -q:, :] = PAD[None, :, None, None]               # the padding, bottom rows
    x[:, :, :, -2:] = PAD[None, :, None, None]               # and right columns
    return x


def taps_of(ops, sigma):
    return dict(zip(("radius", "taps"), ops.strong_taps(sigma)))


def run(ops, x, records, table=None):
    table = sr.to_table(records, ops.strong_rec_dtype()) if table is None else table
    y, mean = ops.strong_augment(torch.from_numpy(x).cuda(), table, return_mean=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), mean.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(ops, name, x, records):
    """the gate of the module's docstring; copy samples are compared through bits -> (y, mean)"""
    y, mean = run(ops, x, records)
    h, w = x.shape[2:]
    live = [b for b, r in enumerate(records) if r["jitter"] is not None or sr.effective_radius(r["radius"], h, w)]
    for b in range(len(records)):
        if b not in live:
            assert np.array_equal(bits(y[b]), bits(x[b])) and mean[b] == 0
    if live:
        y64, m64 = sr.strong_augment(x[live], [records[b] for b in live], np.float64)
        y32, m32 = sr.strong_augment(x[live], [records[b] for b in live], np.float32)
        e32 = float(np.abs(y32 - y64).max())
        tol = 4 * max(e32, 2.0 ** -23)
        err, merr = float(np.abs(y[live] - y64).max()), float(np.abs(mean[live] - m64).max())
        print(f"strong_augment {name} {x.shape}: e32 {e32:.3e} tol {tol:.3e} | y err {err:.3e} ratio {err / tol:.3f} | mean err {merr:.3e} "
              f"ratio {merr / tol:.3f} | differs from ref32 in {int((y[live] != y32).sum())} of {y32.size}")
        assert err <= tol and merr <= tol
        for b in live:
            assert (mean[b] == 0) == (records[b]["jitter"] is None)
    return y, mean


FULL = (1.8, 0.7, 1.4, -0.2)  # fb = 1.8: the clamp bites


@pytest.mark.parametrize("quantised", [False, True])
def test_pointwise_only_4x4(ops, quantised):
    x = make_input((1, 3, 4, 4), quantised, 1)
    check(ops, "pointwise", x, [sr.record(jitter=FULL)])


@pytest.mark.parametrize("quantised", [False, True])
def test_radius_8_on_9x12_where_both_borders_reflect_into_the_same_pixels(ops, quantised):
    x = make_input((2, 3, 9, 12), quantised, 2)
    wide = taps_of(ops, 2.0)
    assert wide["radius"] == 8
    check(ops, "radius8", x, [sr.record(jitter=FULL, **wide), sr.record(**wide)])


@pytest.mark.parametrize("quantised", [False, True])
def test_copy_jitter_only_and_blur_only_samples_33x68(ops, quantised):
    x = make_input((3, 3, 33, 68), quantised, 3)
    planted = np.array([0x7FC12345, -0x3FFFFF, 0x7F800001, -0x80000000, 0x7F800000, -0x800000], dtype=np.int64).astype(np.int32)
    x.view(np.int32)[0, 1, 5, 7:13] = planted  # NaN payloads (quiet, negative, signalling), -0.0, +inf, -inf in the copy sample
    records = [sr.record(), sr.record(jitter=(1.1, 1.3, 0.6, 0.35)), sr.record(**taps_of(ops, 1.15))]
    y, mean = check(ops, "copy|jitter|blur", x, records)
    assert np.array_equal(bits(y[0]), bits(x[0])) and np.array_equal(bits(y[0])[1, 5, 7:13], planted)
    assert mean[0] == 0 and mean[1] > 0 and mean[2] == 0
    assert not np.array_equal(y[1], x[1]) and not np.array_equal(y[2], x[2])


@pytest.mark.parametrize("quantised", [False, True])
def test_two_tiles_plus_one_row_by_two_tiles_plus_four_columns_both_operations(ops, quantised):
    th, tw = ops.STRONG_TILE
    x = make_input((2, 3, 2 * th + 1, 2 * tw + 4), quantised, 4)
    records = [sr.record(jitter=FULL, **taps_of(ops, 2.0)), sr.record(jitter=(0.9, 1.2, 1.1, 0.5), **taps_of(ops, 0.7))]
    check(ops, "tiles+1", x, records)


@pytest.mark.parametrize("factor", ["brightness", "contrast", "saturation", "hue", "hue_half", "identity"])
def test_each_factor_alone(ops, factor):
    jit = dict(brightness=(1.8, 1, 1, 0), contrast=(1, 1.7, 1, 0), saturation=(1, 1, 1.9, 0), hue=(1, 1, 1, -0.2), hue_half=(1, 1, 1, 0.5),
               identity=(1, 1, 1, 0))[factor]
    x = make_input((2, 3, 33, 68), factor in ("hue", "identity"), 5)
    y, _ = check(ops, factor, x, [sr.record(jitter=jit), sr.record(jitter=(jit[0] ** -1, 2 - jit[1], 2 - jit[2], -jit[3]))])
    if factor == "identity":  # one rule, no special case: the conversion there and back is not a copy, it is close to one.  The hue
        # is rounded where h / 6 + 1 lies in [1, 2), half an ulp of 2^-23 per step, and 6 h magnifies that six times: 16 ulps of room
        assert np.abs(y - x).max() <= 16 * 2.0 ** -23


def test_two_runs_and_a_sample_alone_give_equal_bits(ops):
    th, tw = ops.STRONG_TILE
    x = make_input((3, 3, th + 5, tw + 8), False, 6)
    records = [sr.record(jitter=FULL, **taps_of(ops, 1.0)), sr.record(jitter=(0.8, 1.2, 0.9, 0.1)), sr.record(**taps_of(ops, 0.4))]
    y1, m1 = run(ops, x, records)
    y2, m2 = run(ops, x, records)
    assert np.array_equal(bits(y1), bits(y2)) and np.array_equal(bits(m1), bits(m2))
    for b in range(3):  # neither the mean nor a pixel depends on the other samples of the batch
        yb, mb = run(ops, np.ascontiguousarray(x[b:b + 1]), records[b:b + 1])
        assert np.array_equal(bits(yb[0]), bits(y1[b])) and np.array_equal(bits(mb), bits(m1[b:b + 1]))
    back = [records[2], records[0], records[1]]
    y3, m3 = run(ops, np.ascontiguousarray(x[[2, 0, 1]]), back)
    assert np.array_equal(bits(y3), bits(y1[[2, 0, 1]])) and np.array_equal(bits(m3), bits(m1[[2, 0, 1]]))


def test_a_device_record_with_a_radius_out_of_range_behaves_as_radius_0(ops):
    x = make_input((3, 3, 4, 16), False, 7)
    wide = ops.strong_taps(2.0)[1]
    records = [sr.record(jitter=FULL, radius=8, taps=wide), sr.record(radius=4, taps=wide), sr.record(radius=3, taps=wide)]
    table = sr.to_table(records, ops.strong_rec_dtype())
    table["radius"][0] = 9  # what check_strong_table refuses, so it goes up as a device tensor
    dev = torch.from_numpy(table.view(np.int32).reshape(3, 16)).cuda()
    y, mean = run(ops, x, None, table=dev)
    zero = [sr.record(jitter=FULL), sr.record(), records[2]]
    y0, mean0 = run(ops, x, zero)
    assert np.array_equal(bits(y), bits(y0)) and np.array_equal(bits(mean), bits(mean0))
    assert np.array_equal(bits(y[1]), bits(x[1]))  # radius 4 >= h = 4: a copy
    assert not np.array_equal(y[2], x[2])          # radius 3 = h - 1 is a blur
    table["radius"][0], table["radius"][1] = -1, 2 ** 30
    y, _ = run(ops, x, None, table=torch.from_numpy(table.view(np.int32).reshape(3, 16)).cuda())
    assert np.array_equal(bits(y), bits(y0))
    check(ops, "radius3 of 4 rows", x, zero)


def test_wrapper_refusals(ops):
    x = torch.rand(2, 3, 8, 8, device="cuda")
    table = sr.to_table([sr.record(), sr.record()], ops.strong_rec_dtype())
    with pytest.raises(RuntimeError, match="gradient"):
        ops.strong_augment(x.clone().requires_grad_(True), table)
    with pytest.raises(RuntimeError):
        ops.strong_augment(x.cpu(), table)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.strong_augment(torch.rand(2, 3, 8, 6, device="cuda"), table)
    with pytest.raises(RuntimeError):
        ops.strong_augment(x[:, :, :, ::2], table)
    with pytest.raises(ValueError):
        ops.strong_augment(x, table[:1])
    bad = table.copy()
    bad["fh"][1] = 0.7
    with pytest.raises(ValueError):
        ops.strong_augment(x, bad)
    with pytest.raises(RuntimeError):
        ops.strong_augment(x, torch.zeros(2, 15, dtype=torch.int32, device="cuda"))
    y = ops.strong_augment(x, table)
    assert y.data_ptr() != x.data_ptr() and torch.equal(y, x)


# ------------------------------------------------------------------------------------------------ the self-training step

B, H, W = 2, 64, 64


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core as c
    return c


def make_net(core):
    net = core.Network3("mit_b1", 9, pretrained=None)
    dw.load_det_weights(net, seed=0)
    return net.cuda().eval()


def batch(tag):
    x = dw.det_input(f"st_x{tag}", (B, 3, H, W)).cuda()
    y = dw.det_labels(f"st_y{tag}", (B, H, W), 9)
    y[:, 3:9, 10:30] = 255
    return x, y.cuda()


def tbits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("mix", [False, True])
def test_step_with_a_policy_equals_its_hand_composition(core, ops, mix):
    from segmif_amd import losses
    from segmif_amd.data import ClassMix, StrongAugment
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep, cross_mix
    from segmif_amd.train import make_seg_optimizer
    net = make_net(core)
    twin = copy.deepcopy(net)
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)
    (xL, yL), (xU, _) = batch("L"), batch("U")
    xL, xU = xL.clamp(0, 1), xU.clamp(0, 1)
    keep = xU.clone()
    with torch.no_grad():
        t_logits = twin._segment_nhwc(xU)  # before any step the teacher is the student, and it sees the clean xU
    tau = float(ops.pseudo_label(t_logits, H, W, return_conf=True)[2].median())
    policy = StrongAugment(jitter_prob=1.0, blur_prob=1.0, seed=2)
    step = SelfTrainingStep(net, EmaTeacher(opt, net), opt, torch.nn.CrossEntropyLoss(ignore_index=255), tau=tau,
                            mix=ClassMix(prob=1.0, seed=1) if mix else None, strong=policy)
    assert step.last_strong is None
    _, l_unsup = step.step(xL, yL, xU)
    table = step.last_strong
    assert table.dtype == ops.strong_rec_dtype() and table.shape == (B,) and table["jitter_on"].all() and (table["radius"] > 0).all()
    assert table.tobytes() == StrongAugment(jitter_prob=1.0, blur_prob=1.0, seed=2).draw(B).tobytes()
    assert torch.equal(tbits(xU), tbits(keep))  # out of place
    labels, count = ops.pseudo_label(t_logits, H, W, tau=tau)
    q = ops.pseudo_weight(count, H, W)
    unsup = losses.SegObjective(reduction="mean_all")
    if mix:
        xM, yM, uM, pasted = cross_mix(xL, yL, xU, labels, q, step.last_table)
        assert int(pasted.sum()) > 0
        kw = dict(pixel_weight=uM)
    else:
        xM, yM, kw = xU, labels, dict(sample_weight=q)
    xS = ops.strong_augment(xM, table)  # after the mix; labels and weights as they were
    want = float(twin._loss(xS, yM, unsup, **kw).detach())
    plain = float(twin._loss(xM, yM, unsup, **kw).detach())
    print(f"unlabelled term: step {float(l_unsup):.6f}, by hand {want:.6f}, without the augmentation {plain:.6f}")
    assert want > 0 and abs(float(l_unsup) - want) <= VALUE_GATE * abs(want)
    assert abs(plain - want) > 10 * VALUE_GATE * abs(want)  # (the augmentation is seen by the loss)


def test_two_steps_without_a_policy_give_the_bits_of_a_step_that_was_never_given_one(core, ops):
    from segmif_amd.data import ClassMix
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
    from segmif_amd.train import make_seg_optimizer
    (xL, yL), (xU, _) = batch("L"), batch("U")
    seen = []
    for kw in ({}, dict(strong=None)):
        net = make_net(core)
        opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)
        step = SelfTrainingStep(net, EmaTeacher(opt, net), opt, torch.nn.CrossEntropyLoss(ignore_index=255), tau=0.3,
                                mix=ClassMix(prob=1.0, seed=1), **kw)
        out = [step.step(xL, yL, xU) for _ in range(2)]
        assert step.last_strong is None
        seen.append(([tbits(v).clone() for pair in out for v in pair], [tbits(p).clone() for p in net.parameters()]))
    (la, pa), (lb, pb) = seen
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_train_command_line_with_strong_augmentation(core, tmp_path):
    """python -m segmif_amd.train --self-training --st-strong in a fresh child process: it names the settings, trains and leaves
    both checkpoints with finite weights"""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "8", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "3",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path),
           "--ema-decay", "0.9", "--self-training", "--st-threshold", "0.12", "--st-mix", "--st-strong", "--st-jitter-prob", "1.0",
           "--st-blur-prob", "1.0", "--st-blur-sigma", "0.5", "2.0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = r.stdout
    announced = [ln for ln in out.splitlines() if ln.startswith("[train] --self-training (")]
    assert len(announced) == 1 and "NOT the reference's training" in announced[0]
    assert "--st-strong jitter_prob 1.0, strength 0.2, hue 0.2, blur_prob 1.0, sigma (0.5, 2.0)" in announced[0]
    seg_lines = [ln for ln in out.splitlines() if "segmentation iter 3/3" in ln]
    assert len(seg_lines) == 1 and " unlabelled " in seg_lines[0]
    unl = float(seg_lines[0].split(" unlabelled ")[1].split()[0])
    assert np.isfinite(unl) and unl >= 0.0
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
