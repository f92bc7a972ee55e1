"""GPU tests of ops.pseudo_label / ops.pseudo_weight (csrc/pseudo_label.hip) against the float64 restatement of
tests/_self_training_ref.py.  Inputs: x = float32(8 * RandomState(seed).standard_normal((B, h, w, C))).

Gates.  Labels: equal to the float64 argmax wherever the float64 top-2 gap is at least 1e-4, and equal to ops.bilinear_argmax on
EVERY pixel (the same expression, the same comparison).  Decisions: pixels whose float64 p_max lies within 1e-5 of tau are left out
of the comparison - at most 0.1 % of a case's pixels may be (on these inputs at most 12 of 86 400 are) - and every other decision
equals the reference's; |count - reference| is at most the sample's left-out pixels; count equals the number of conf > tau in the
kernel's own conf exactly.  conf: 4 x the largest error of torch's own float32 evaluation of the formula on the same inputs,
softmax(ops.bilinear(x)).max, measured in the same test (the rule of the TTA and EMA tests)."""
import functools

import numpy as np
import pytest
import torch

import _self_training_ref as ref

pytestmark = pytest.mark.gpu

CASES = {  # name: (B, h, w, OH, OW, C, seed)
    "odd": (3, 5, 7, 19, 27, 9, 0),         # odd sizes, a scale that is no integer, three per-sample counts
    "x4": (2, 16, 16, 64, 64, 9, 1),        # the training case
    "c32": (2, 3, 4, 12, 16, 32, 2),        # the most classes a row holds
    "wide": (2, 9, 300, 36, 1200, 9, 3),    # more than one 256-wide block per output row
}
TAUS = (0.968, 0.5)
GAP_MARGIN, TAU_MARGIN, LEFT_OUT_CAP = 1e-4, 1e-5, 1e-3


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def host_input(name):
    B, h, w, OH, OW, C, seed = CASES[name]
    return np.float32(8 * np.random.RandomState(seed).standard_normal((B, h, w, C)))


@functools.lru_cache(maxsize=None)
def reference(name, tau):
    """computed once per (case, tau), shared, never modified"""
    _, _, _, OH, OW, _, _ = CASES[name]
    return ref.pseudo_label(host_input(name), OH, OW, tau)


def check_case(ops, x_dev, x_host_name, tau):
    _, _, _, OH, OW, _, _ = CASES[x_host_name]
    r = reference(x_host_name, tau)
    labels, count, conf = ops.pseudo_label(x_dev, OH, OW, tau=tau, return_conf=True)
    lab_ign, count_ign = ops.pseudo_label(x_dev, OH, OW, tau=tau, below="ignore", ignore_index=255)
    ba = ops.bilinear_argmax(x_dev, OH, OW)
    assert labels.dtype == torch.int64 and count.dtype == torch.int64 and conf.dtype == torch.float32
    labels_h, conf_h, count_h = labels.cpu().numpy(), conf.cpu().numpy(), count.cpu().numpy()
    # labels
    sure = r["gap"] >= GAP_MARGIN
    assert (labels_h[sure] == r["argmax"][sure]).all()
    assert torch.equal(labels, ba.long()), "pseudo_label and bilinear_argmax disagree: the interpolation was contracted differently"
    # decisions and counts
    near = np.abs(r["p_max"] - tau) <= TAU_MARGIN
    share = near.mean()
    print(f"{x_host_name} tau {tau}: left out {int(near.sum())} of {near.size} ({share:.5%}); confident share {r['confident'].mean():.4f}")
    assert share <= LEFT_OUT_CAP
    decided = conf_h > tau
    assert (decided[~near] == r["confident"][~near]).all()
    per_sample_near = near.reshape(len(near), -1).sum(1)
    assert (np.abs(count_h - r["count"]) <= per_sample_near).all()
    assert (count_h == decided.reshape(len(decided), -1).sum(1)).all()
    assert torch.equal(count_ign, count)
    assert torch.equal(lab_ign, torch.where(conf > tau, labels, torch.full_like(labels, 255)))
    assert 0.05 < r["confident"].mean() < 0.99  # both branches are exercised
    return conf_h, r


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", list(CASES))
def test_labels_decisions_and_counts(ops, name, tau):
    check_case(ops, torch.from_numpy(host_input(name)).cuda(), name, tau)


def test_channel_slice_of_a_wider_tensor(ops):
    """ldx > C: the logits are a channel slice, read in place"""
    x = host_input("odd")
    wide = torch.full(x.shape[:3] + (13,), float("nan"), dtype=torch.float32)
    wide[..., 2:11] = torch.from_numpy(x)
    view = wide.cuda()[..., 2:11]
    assert not view.is_contiguous()
    conf_h, r = check_case(ops, view, "odd", 0.968)
    assert np.isfinite(conf_h).all()


@pytest.mark.parametrize("name", list(CASES))
def test_confidence_against_float64(ops, name):
    _, _, _, OH, OW, _, _ = CASES[name]
    x = torch.from_numpy(host_input(name)).cuda()
    r = reference(name, 0.968)
    _, _, conf = ops.pseudo_label(x, OH, OW, return_conf=True)
    torch_f32 = torch.softmax(ops.bilinear(x, OH, OW), dim=-1).max(-1).values
    err = float(np.abs(conf.cpu().numpy().astype(np.float64) - r["p_max"]).max())
    torch_err = float(np.abs(torch_f32.cpu().numpy().astype(np.float64) - r["p_max"]).max())
    print(f"{name}: conf max abs error {err:.3e}; torch float32 softmax(bilinear).max {torch_err:.3e}")
    assert err <= 4 * torch_err


def test_pseudo_weight_is_the_confident_share(ops):
    _, _, _, OH, OW, _, _ = CASES["odd"]
    _, count = ops.pseudo_label(torch.from_numpy(host_input("odd")).cuda(), OH, OW)
    q = ops.pseudo_weight(count, OH, OW)
    assert q.dtype == torch.float32 and q.shape == count.shape and q.is_cuda
    assert np.array_equal(q.cpu().numpy(), (count.cpu().numpy() / (OH * OW)).astype(np.float32))


def test_edges(ops):
    B, h, w, OH, OW, C, _ = CASES["odd"]
    x = torch.from_numpy(host_input("odd")).cuda()
    _, count = ops.pseudo_label(x, OH, OW, tau=0.0)
    assert count.tolist() == [OH * OW] * B
    lab1, count1, conf1 = ops.pseudo_label(x, OH, OW, tau=1.0, below="ignore", return_conf=True)
    assert count1.tolist() == [0] * B and bool((lab1 == 255).all()) and bool((conf1 <= 1).all())
    # C = 1: label 0, confidence 1, every pixel confident
    lab, count, conf = ops.pseudo_label(x[..., :1], OH, OW, tau=0.968, return_conf=True)
    assert bool((lab == 0).all()) and bool((conf == 1).all()) and count.tolist() == [OH * OW] * B
    # one NaN logit: the output pixels that read it are not confident, all others are untouched
    clean = ops.pseudo_label(x, OH, OW, tau=0.5, return_conf=True)
    bad = x.clone()
    bad[1, 2, 3, 4] = float("nan")
    lab_n, count_n, conf_n = ops.pseudo_label(bad, OH, OW, tau=0.5, return_conf=True)
    touched = torch.isnan(conf_n)
    probe = torch.zeros(B, h, w, 1, device="cuda")
    probe[1, 2, 3, 0] = 1.0
    reads = ops.bilinear(probe, OH, OW)[..., 0] != 0  # the output pixels with a non-zero weight on that source pixel
    # every pixel that weighs the NaN is hit; a tap of weight 0 passes a NaN on too, so the hit set may be a little larger, but it
    # stays inside the source pixel's neighbourhood: at most (2 ceil(19 / 5) + 1) x (2 ceil(27 / 7) + 1) output pixels of sample 1
    assert bool((reads & ~touched).sum() == 0) and 0 < int(touched.sum()) <= 81 and not bool(touched[0].any()) and not bool(touched[2].any())
    assert torch.equal(lab_n[~touched], clean[0][~touched]) and torch.equal(conf_n[~touched], clean[2][~touched])
    assert count_n.tolist() == (torch.nan_to_num(conf_n, nan=0.0) > 0.5).flatten(1).sum(1).tolist()
    lab_i, _ = ops.pseudo_label(bad, OH, OW, tau=0.5, below="ignore", ignore_index=250)
    assert bool((lab_i[touched] == 250).all())


def test_count_is_zeroed_by_every_call(ops):
    """the same count buffer, two calls: the second does not add to the first"""
    import ctypes

    from segmif_amd import _lib
    B, h, w, OH, OW, C, _ = CASES["odd"]
    x = torch.from_numpy(host_input("odd")).cuda()
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device="cuda")
    count = torch.full((B,), 12345, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = []
    for _ in range(2):
        assert _lib.load().segmif_pseudo_label_f32(x.data_ptr(), labels.data_ptr(), None, count.data_ptr(), B, h, w, OH, OW, C, C, 0.5, 0,
                                                    255, stream) == 0
        seen.append(count.tolist())
    assert seen[0] == seen[1] == ops.pseudo_label(x, OH, OW, tau=0.5)[1].tolist()


def test_refusals_come_before_any_launch(ops):
    import ctypes

    from segmif_amd import _lib
    lib = _lib.load()
    B, h, w, OH, OW, C = 1, 2, 2, 4, 4, 3
    x = torch.zeros(B, h, w, C, device="cuda")
    labels = torch.full((B, OH, OW), -7, dtype=torch.int64, device="cuda")
    count = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B=B, h=h, w=w, OH=OH, OW=OW, C=C, ldx=C, tau=0.5):
        return lib.segmif_pseudo_label_f32(x.data_ptr(), labels.data_ptr(), None, count.data_ptr(), B, h, w, OH, OW, C, ldx, tau, 0, 255, stream)

    einval = -22  # SEGMIF_EINVAL
    for kw in (dict(B=0), dict(h=0), dict(w=0), dict(OH=0), dict(OW=0), dict(C=0), dict(C=33, ldx=33), dict(ldx=2),
               dict(tau=float("nan")), dict(tau=-0.01), dict(tau=1.01)):
        assert call(**kw) == einval, kw
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((count == -7).all())  # nothing ran: not even the memset of count
    with pytest.raises(ValueError):
        ops.pseudo_label(x, OH, OW, tau=float("nan"))
    with pytest.raises(ValueError):
        ops.pseudo_label(x, OH, OW, tau=1.5)
    with pytest.raises(ValueError):
        ops.pseudo_label(x, OH, OW, below="drop")
    with pytest.raises((ValueError, RuntimeError)):
        ops.pseudo_label(torch.zeros(1, 2, 2, 33, device="cuda"), OH, OW)
    with pytest.raises(RuntimeError):
        ops.pseudo_label(x.cpu(), OH, OW)
