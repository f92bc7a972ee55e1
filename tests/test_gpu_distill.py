"""GPU tests of the distillation objectives (csrc/distill_objective.hip behind losses.DistillObjective), of segmif_amd.distill and of
the train command's --distill-from.

The gate, for value and gradient alike: the error against the float64 restatement tests/_distill_ref.py is at most 4 times the error
of torch's own float32 evaluation of the same formula (softmax, log-softmax, multiply, sum; _distill_ref.torch_ops) on the device, on
the same inputs - 4 x torch's float32 error is this project's convention for float32 kernels - with a floor of 4 * 2^-23 where
torch's error is smaller.  The error is relative to |loss|, and for the gradient to its largest element; torch's is measured inside
the test.  Where the float64 value is exactly 0 (one class in pixel mode, one position in channel mode: a softmax over one element)
there is nothing to be relative to, and the kernel must give exactly 0 - which it does by construction: p = exp(0) / 1, and
(z - max) - log(1) = 0 on both sides.

The shapes are the smallest at which the kernels can go wrong; the block constants come from include/segmif_distill.h."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _distill_ref as ref
import detweights as dw
from _observed import observed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 4 * 2.0 ** -23
UPSTREAM = 0.37
KINDS = ("pixel", "channel")
TEMPERATURES = (0.5, 1.0, 4.0)


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "segmif_distill.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


BLOCK_ROWS, MAX_BLOCKS = header_constant("SEGMIF_DISTILL_BLOCK_ROWS"), header_constant("SEGMIF_DISTILL_MAX_BLOCKS_PER_SAMPLE")
assert 2 * BLOCK_ROWS + 1 == 19 * 27 and (MAX_BLOCKS + 1) * BLOCK_ROWS + 1 == 129 * 129  # the two shapes below are built on them
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 9), (2, 3, 5, 9), (3, 17, 23, 9), (2, 5, 7, 32),
          (2, 19, 27, 9),    # P = 2 blocks of rows + 1: three blocks per sample, the last with one row
          (3, 16, 20, 9),    # P * C a multiple of 4 and two blocks per sample: channel mode's 16-byte path on every sample
          (1, 129, 129, 9)]  # P = (the cap + 1) blocks of rows + 1: blocks 0 and 1 of the sample walk two tiles


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core  # noqa: F401
    return torch.device("cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def inputs(shape, extreme=False):
    """student and teacher logits (B, h, w, C) float32 on the CPU; extreme: a tenth of the entries of each set to +-80"""
    g = torch.Generator().manual_seed(1000 + sum(shape) + 7 * shape[-1])
    s, t = (3.0 * torch.randn(shape, generator=g, dtype=torch.float32) for _ in range(2))
    if extreme:
        for x in (s, t):
            where = torch.rand(shape, generator=g) < 0.1
            sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
            x[where] = 80.0 * sign[where]
    return s, t


@functools.lru_cache(maxsize=None)
def reference(kind, shape, T, extreme=False):
    """float64 value and gradient of the restatement: computed once, shared, never changed"""
    s, t = inputs(shape, extreme)
    return float(ref.loss(kind, s.double(), t.double(), T)), ref.grad(kind, s.double(), t.double(), T)


def torch_float32(kind, s, t, T):
    """torch's own float32 evaluation on the device: value and gradient for upstream 1"""
    s = s.detach().clone().requires_grad_(True)
    v = ref.torch_ops(kind, s, t, T)
    v.backward()
    return float(v.detach()), s.grad.double().cpu()


def ours(kind, s, t, T, upstream=UPSTREAM):
    from segmif_amd import losses
    v = losses.DistillObjective(kind, T).forward_nhwc(s, t)
    (v * upstream).backward()
    return v.detach(), s.grad


def leaf(x, layout, dev):
    """x on the device as a leaf in `layout`: dense | pitched (a channel slice of a wider buffer) | offset (base one float off)"""
    shape = x.shape
    if layout == "dense":
        out = x.to(dev)
    elif layout == "pitched":
        wide = torch.full(shape[:-1] + (shape[-1] + 3,), float("nan"), device=dev)
        wide[..., :shape[-1]] = x.to(dev)
        out = wide[..., :shape[-1]]
    else:
        flat = torch.full((x.numel() + 1,), float("nan"), device=dev)
        flat[1:] = x.to(dev).reshape(-1)
        out = flat[1:].view(shape)
        assert out.data_ptr() % 16 == 4
    return out.detach()


def gate(name, kind, shape, T, v, g, s_dev, t_dev, extreme=False):
    """the docstring's gate for value v and gradient g (of upstream UPSTREAM) on inputs(shape, extreme)"""
    want_v, want_g = reference(kind, shape, T, extreme)
    v, g = float(v), g.double().cpu() / float(np.float32(UPSTREAM))  # (the upstream the backward read: 0.37 as a float32)
    assert np.isfinite(v) and bool(torch.isfinite(g).all())
    tv, tg = torch_float32(kind, s_dev.detach(), t_dev, T)
    gmax = float(want_g.abs().max())
    if want_v == 0.0 and gmax == 0.0:
        print(f"{name}: exact zero expected; value {v!r}, largest gradient element {float(g.abs().max())!r}")
        assert v == 0.0 and float(g.abs().max()) == 0.0
        return
    ev, tev = abs(v - want_v) / abs(want_v), abs(tv - want_v) / abs(want_v)
    eg, teg = float((g - want_g).abs().max()) / gmax, float((tg - want_g).abs().max()) / gmax
    print(f"{name}: value error {ev:.3e} (torch float32 {tev:.3e}), gradient error {eg:.3e} (torch float32 {teg:.3e})")
    observed(f"distill_{name}", {"value": ev, "torch_value": tev, "grad": eg, "torch_grad": teg})
    assert ev <= max(4 * tev, FLOOR), (ev, tev)
    assert eg <= max(4 * teg, FLOOR), (eg, teg)


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_value_and_gradient_against_float64(dev, kind, shape, T):
    s, t = inputs(shape)
    s_dev, t_dev = leaf(s, "dense", dev).requires_grad_(True), leaf(t, "dense", dev)
    v, g = ours(kind, s_dev, t_dev, T)
    gate(f"{kind}_{'x'.join(map(str, shape))}_T{T}", kind, shape, T, v, g, s_dev, t_dev)
    v2, g2 = ours(kind, s_dev.detach().clone().requires_grad_(True), t_dev.clone(), T)
    assert torch.equal(bits(v), bits(v2)) and torch.equal(bits(g), bits(g2))  # two runs: equal bits


@pytest.mark.parametrize("layouts", [("pitched", "dense"), ("dense", "pitched"), ("offset", "dense"), ("dense", "offset"), ("offset", "pitched")])
@pytest.mark.parametrize("shape", [(3, 17, 23, 9), (3, 16, 20, 9)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_layouts_give_the_dense_bits(dev, kind, shape, layouts):
    """pitched views (ld > C) for the student and the teacher separately, and a base offset by one float: the scalar path computes
    what the 16-byte path does, and the gate holds"""
    s, t = inputs(shape)
    T = 4.0
    s_dev, t_dev = leaf(s, layouts[0], dev).requires_grad_(True), leaf(t, layouts[1], dev)
    v, g = ours(kind, s_dev, t_dev, T)
    gate(f"{kind}_{'x'.join(map(str, shape))}_{layouts[0]}_{layouts[1]}", kind, shape, T, v, g, s_dev, t_dev)
    dense = leaf(s, "dense", dev).requires_grad_(True)
    v0, g0 = ours(kind, dense, leaf(t, "dense", dev), T)
    assert torch.equal(bits(v), bits(v0)) and torch.equal(bits(g), bits(g0))


@pytest.mark.parametrize("shape", [(2, 3, 5, 9), (3, 17, 23, 9), (2, 19, 27, 9), (2, 5, 7, 32)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_logits_of_80_at_half_temperature_stay_finite(dev, kind, shape):
    """z = +-160: exp overflows without the max subtraction, and log(p) of an underflowed teacher probability gives 0 * inf"""
    s, t = inputs(shape, True)
    assert float(s.abs().max()) == 80.0 and float(t.abs().max()) == 80.0
    s_dev, t_dev = leaf(s, "dense", dev).requires_grad_(True), leaf(t, "dense", dev)
    v, g = ours(kind, s_dev, t_dev, 0.5)
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(g).all())
    gate(f"{kind}_{'x'.join(map(str, shape))}_pm80", kind, shape, 0.5, v, g, s_dev, t_dev, extreme=True)


def test_channel_mode_sample_zero_alone_has_its_bits_in_a_batch(dev):
    """a sample's k_bc and its gradient's direction depend on that sample only: sample 0 alone (B = 1, upstream 1.0) against its rows
    in a batch of 2 with upstream 2.0 - the scale T / (B C) halves, the upstream doubles, both exactly"""
    for shape in ((2, 19, 27, 9), (2, 16, 20, 9)):
        s, t = inputs(shape)
        s2, t2 = leaf(s, "dense", dev).requires_grad_(True), leaf(t, "dense", dev)
        _, g2 = ours("channel", s2, t2, 4.0, upstream=2.0)
        s1, t1 = leaf(s[:1], "dense", dev).requires_grad_(True), leaf(t[:1], "dense", dev)
        _, g1 = ours("channel", s1, t1, 4.0, upstream=1.0)
        assert torch.equal(bits(g1[0]), bits(g2[0])) and float(g1.abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_teacher_gets_no_gradient_and_one_that_wants_it_is_refused(dev, kind):
    from segmif_amd import autograd as ag, losses
    s, t = inputs((2, 3, 5, 9))
    s_dev, t_dev = leaf(s, "dense", dev).requires_grad_(True), leaf(t, "dense", dev)
    desc = ag.distill_descriptor(kind, 2.0)
    v = ag.DistillObjectiveFn.apply(s_dev, t_dev.requires_grad_(True), desc, 15)  # the node itself: no gradient for the teacher
    v.backward()
    assert t_dev.grad is None and s_dev.grad is not None
    with pytest.raises(RuntimeError, match="teacher logits require grad"):
        losses.DistillObjective(kind).forward_nhwc(s_dev, t_dev)
    nchw = losses.DistillObjective(kind, 2.0)(s_dev.detach().permute(0, 3, 1, 2), t_dev.detach().permute(0, 3, 1, 2))
    assert torch.equal(bits(nchw), bits(v))  # the NCHW front end on a channels-last view: the same rows


def make_net(backbone, seed):
    import segmif_amd.core as core
    net = core.Network3(backbone, 9, pretrained=None)
    dw.load_det_weights(net, seed=seed)
    return net.cuda().eval()


@pytest.mark.parametrize("kind", KINDS)
def test_distill_step_equals_its_composition_by_hand(dev, kind):
    """student Network3('mit_b1'), teacher mit_b2, 9 classes, 2 frames of 64 x 96, seeded weights, in the eval-mode regime of the
    other step tests (no stochastic depth: two evaluations of one step agree): both loss terms and every parameter after one step,
    bit for bit"""
    import copy
    from segmif_amd import losses
    from segmif_amd.core.model_fusion import seg_criterion_loss
    from segmif_amd.distill import DistillStep, FrozenTeacher
    from segmif_amd.train import make_seg_optimizer
    student, teacher_net = make_net("mit_b1", 0), make_net("mit_b2", 1)
    twin = copy.deepcopy(student)
    x = dw.det_input("distill_x", (2, 3, 64, 96)).cuda()
    y = dw.det_labels("distill_y", (2, 64, 96), 9)
    y[:, 3:9, 10:30] = 255
    y = y.cuda()
    crit, obj = torch.nn.CrossEntropyLoss(ignore_index=255), losses.DistillObjective(kind)
    teacher = FrozenTeacher(teacher_net)
    assert not any(p.requires_grad for p in teacher_net.parameters())
    step = DistillStep(student, teacher, make_seg_optimizer(student), crit, obj)
    sup, kd = step.step(x, y)
    assert float(sup) > 0 and float(kd) > 0 and not sup.requires_grad and not kd.requires_grad

    opt = make_seg_optimizer(twin)
    opt.zero_grad(set_to_none=True)
    seg = twin._segment_nhwc(x)
    want_sup = seg_criterion_loss(seg, y, crit)
    with torch.no_grad():
        t_logits = teacher_net._segment_nhwc(x)
    assert t_logits.shape == seg.shape and torch.equal(bits(t_logits), bits(teacher.logits(x)))
    want_kd = obj.forward_nhwc(seg, t_logits)
    (want_sup + 3.0 * want_kd).backward()
    opt.step()
    assert torch.equal(bits(sup), bits(want_sup)) and torch.equal(bits(kd), bits(want_kd))
    for (n, a), b in zip(student.named_parameters(), twin.parameters()):
        assert torch.equal(bits(a), bits(b)), n
    before = make_net("mit_b1", 0)
    assert any(not torch.equal(a, b) for a, b in zip(student.parameters(), before.parameters()))  # the step moved the weights
    assert all(p.grad is None for p in teacher_net.parameters())


def test_train_command_line_with_distillation(dev, tmp_path):
    """two iterations of python -m segmif_amd.train --synthetic with --distill-from a checkpoint this test writes, in a fresh child
    process: the files are the usual two, the log has the announcement and the distillation term"""
    import segmif_amd.core as core
    ckpt, out_dir = tmp_path / "teacher.pth", tmp_path / "out"
    torch.manual_seed(11)
    torch.save(core.Network3("mit_b2", 9, pretrained=None).state_dict(), ckpt)
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "8", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(out_dir),
           "--distill-from", str(ckpt), "--distill-backbone", "mit_b2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    announced = [ln for ln in lines if ln.startswith("[train] --distill-from ")]
    assert len(announced) == 1 and "NOT the reference's training" in announced[0] and "mIoU" in announced[0]
    assert "kind channel, temperature 4.0, weight 3.0" in announced[0]
    seg_lines = [ln for ln in lines if "segmentation iter 2/2" in ln]
    assert len(seg_lines) == 1 and " distill " in seg_lines[0]
    term = float(seg_lines[0].split(" distill ")[1].split()[0])
    assert np.isfinite(term) and term >= 0.0
    assert not any(" distill " in ln for ln in lines if "fusion iter" in ln)  # the segmentation phase only
    assert sorted(os.listdir(out_dir)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(out_dir):
        sd = torch.load(out_dir / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
