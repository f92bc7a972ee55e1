"""GPU tests of segmif_amd.selftrain: the EMA teacher that shares the average's storage, the cross-set ClassMix and the
self-training step, on Network3('mit_b1', 9) - the smallest backbone the training tests use - at batch 2, 64 x 64, in the eval-mode
regime of the other step tests (no stochastic depth: two evaluations of one step agree).  Gates: value 1e-5 relative, gradient 5e-5
of the largest element of the reference gradient (tests/test_gpu_seg_objectives.py's); equalities through bits where stated."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _class_mix_ref as mix_ref
import _self_training_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

VALUE_GATE, GRAD_GATE = 1e-5, 5e-5
B, H, W = 2, 64, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_teacher_shares_the_average_and_needs_its_refresh(core):
    from segmif_amd.selftrain import EmaTeacher
    from segmif_amd.utils.optimizer import FusedAdamW, ema_state_dict
    net = make_net(core)
    opt = FusedAdamW(net.parameters(), lr=1e-3, ema_decay=0.9)
    teacher = EmaTeacher(opt, net)
    x, _ = batch("t")
    with torch.no_grad():
        assert torch.equal(bits(teacher.logits(x)), bits(net._segment_nhwc(x)))  # no step yet: the teacher is the student
    g = torch.Generator(device="cuda").manual_seed(5)
    for i in range(3):
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=g, device="cuda")
        opt.step()
        if i < 2:
            teacher.refresh()
            teacher.logits(x)  # (fills the teacher's packed-weight caches with this step's weights)
    avg = opt.ema_tensors()
    shared = [t.data_ptr() == avg[s][0].data_ptr() for t, s in zip(teacher.module.parameters(), net.parameters())]
    assert all(shared) and len(shared) == len(avg)
    fresh = copy.deepcopy(net)
    fresh.load_state_dict(ema_state_dict(opt, net))
    with torch.no_grad():
        want = fresh.eval()._segment_nhwc(x)
        stale = teacher.logits(x).clone()
        assert not torch.equal(stale, want)  # the kernel wrote through raw pointers: the caches still hold step 2's packed weights
        teacher.refresh()
        assert torch.equal(bits(teacher.logits(x)), bits(want))
        assert not torch.equal(want, net._segment_nhwc(x))  # (and the average is not the student)


@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_cross_mix_equals_the_restatement(core, prob):
    from segmif_amd.data import ClassMix
    from segmif_amd.selftrain import cross_mix, cross_mix_table
    n, h, w, n_class, min_pixels = 3, 12, 16, 9, 2
    rng = np.random.RandomState(7)
    xL, xU = (torch.from_numpy(rng.standard_normal((n, 3, h, w)).astype(np.float32)) for _ in range(2))
    yL = torch.from_numpy(np.repeat(np.repeat(rng.randint(0, n_class, (n, h // 4, w // 4)), 4, 1), 4, 2).astype(np.int64))
    yL[:, 0, :5] = 255
    yU = torch.from_numpy(rng.randint(0, n_class, (n, h, w)).astype(np.int64))
    q = torch.tensor([0.25, 0.0, 0.8125], dtype=torch.float32)
    table = cross_mix_table(n, ClassMix(prob=prob, min_pixels=min_pixels, seed=3))
    assert (table[:n, 0] == np.arange(n)).all() and set(table[n:, 0] - np.arange(n)) <= {0, n}
    xM, yM, uM, pasted = cross_mix(xL.cuda(), yL.cuda(), xU.cuda(), yU.cuda(), q.cuda(), table, n_class, min_pixels)
    x, y = torch.cat([xL, xU]).numpy(), torch.cat([yL, yU]).numpy()
    wplane = np.concatenate([np.ones(n, np.float32), q.numpy()])[:, None, None, None] * np.ones((1, 1, h, w), np.float32)
    sel, want_pasted, _ = mix_ref.select(mix_ref.counts(y, n_class), table, n_class, min_pixels)
    (want_x, want_w), want_y, M = mix_ref.apply([x.view(np.int32), wplane.view(np.int32)], y, table[:, 0], sel)
    assert np.array_equal(xM.cpu().numpy().view(np.int32), want_x[n:]) and np.array_equal(yM.cpu().numpy(), want_y[n:])
    assert np.array_equal(uM.cpu().numpy().view(np.int32), want_w[n:, 0]) and np.array_equal(pasted.cpu().numpy(), want_pasted[n:])
    u = uM.cpu().numpy()
    for b in range(n):  # 1.0 exactly where a labelled pixel was pasted, q_b elsewhere
        assert (u[b][M[n + b]] == 1.0).all() and (u[b][~M[n + b]] == q[b].item()).all()
    if prob == 1.0:
        assert M[n:].any() and not M[n:].all()


def hand_composition(net, xL, yL, xU, crit, teacher_logits, tau, unsup_weight):
    """the step's two losses and gradients from the public pieces, without segmif_amd.selftrain"""
    from segmif_amd import losses, ops
    labels, count = ops.pseudo_label(teacher_logits, H, W, tau=tau)
    q = ops.pseudo_weight(count, H, W)
    net.zero_grad(set_to_none=True)
    l_sup = net._loss(xL, yL, crit)
    l_unsup = net._loss(xU, labels, losses.SegObjective(reduction="mean_all"), sample_weight=q)
    (l_sup + unsup_weight * l_unsup).backward()
    return l_sup.detach(), l_unsup.detach(), labels, q


def test_step_equals_its_hand_composition(core):
    from segmif_amd import ops
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
    from segmif_amd.train import make_seg_optimizer
    net = make_net(core)
    twin = copy.deepcopy(net)
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)
    teacher = EmaTeacher(opt, net)
    (xL, yL), (xU, _) = batch("L"), batch("U")
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with torch.no_grad():
        t_logits = twin._segment_nhwc(xU)  # before any step the teacher is the student
        before_teacher = teacher.logits(xU).clone()
    assert torch.equal(bits(before_teacher), bits(t_logits))
    conf = ops.pseudo_label(t_logits, H, W, return_conf=True)[2]
    tau = float(conf.median())  # about half of the pixels confident, whatever these weights make of the input
    step = SelfTrainingStep(net, teacher, opt, crit, tau=tau, unsup_weight=0.75)
    before = [p.detach().clone() for p in net.parameters()]
    l_sup, l_unsup = step.step(xL, yL, xU)
    want_sup, want_unsup, _, q = hand_composition(twin, xL, yL, xU, crit, t_logits, tau, 0.75)
    share = step.confident_share()
    print(f"tau {tau:.6f}: confident share {share:.4f}, q {q.tolist()}, sup {float(l_sup):.6f}, unsup {float(l_unsup):.6f}")
    assert 0.2 < share < 0.8 and abs(share - float(q.double().mean())) < 1e-6
    assert abs(float(l_sup) - float(want_sup)) <= VALUE_GATE * abs(float(want_sup))
    assert float(want_unsup) > 0 and abs(float(l_unsup) - float(want_unsup)) <= VALUE_GATE * abs(float(want_unsup))
    worst, compared = 0.0, 0
    for (name, p), pt in zip(net.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (pt.grad is None), name
        if pt.grad is not None:
            compared += 1
            worst = max(worst, float((p.grad - pt.grad).abs().max() / pt.grad.abs().max().clamp_min(1e-30)))
    print(f"worst parameter gradient, relative to its largest element: {worst:.3e}")
    assert compared > 100 and worst <= GRAD_GATE
    # the step changed the weights and moved the teacher
    assert any(not torch.equal(a, p) for a, p in zip(before, net.parameters()))
    with torch.no_grad():
        assert not torch.equal(teacher.logits(xU), before_teacher)


def test_unlabelled_term_at_tau_zero_is_mean_all_ce_on_the_argmax(core):
    from segmif_amd import ops
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep
    from segmif_amd.train import make_seg_optimizer
    net = make_net(core)
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)
    (xL, yL), (xU, _) = batch("L"), batch("U")
    with torch.no_grad():
        low = net._segment_nhwc(xU)
        arg = ops.bilinear_argmax(low, H, W).long().cpu()
        up = ops.bilinear(low, H, W).double().cpu()
    want = ref.weighted_objective(up, arg, reduction="mean_all")
    step = SelfTrainingStep(net, EmaTeacher(opt, net), opt, torch.nn.CrossEntropyLoss(ignore_index=255), tau=0.0)
    _, l_unsup = step.step(xL, yL, xU)
    assert step.confident_share() == 1.0
    assert abs(float(l_unsup) - float(want)) <= VALUE_GATE * abs(float(want))


def test_step_with_the_cross_set_mix(core):
    """with mix: the unlabelled term is the weighted objective on cross_mix's outputs (recomputed here from the step's table)"""
    from segmif_amd import losses, ops
    from segmif_amd.data import ClassMix
    from segmif_amd.selftrain import EmaTeacher, SelfTrainingStep, cross_mix
    from segmif_amd.train import make_seg_optimizer
    net = make_net(core)
    twin = copy.deepcopy(net)
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)
    (xL, yL), (xU, _) = batch("L"), batch("U")
    with torch.no_grad():
        t_logits = twin._segment_nhwc(xU)
    tau = float(ops.pseudo_label(t_logits, H, W, return_conf=True)[2].median())
    step = SelfTrainingStep(net, EmaTeacher(opt, net), opt, torch.nn.CrossEntropyLoss(ignore_index=255), tau=tau, mix=ClassMix(prob=1.0, seed=1))
    _, l_unsup = step.step(xL, yL, xU)
    labels, count = ops.pseudo_label(t_logits, H, W, tau=tau)
    xM, yM, uM, pasted = cross_mix(xL, yL, xU, labels, ops.pseudo_weight(count, H, W), step.last_table)
    assert int(pasted.sum()) > 0
    want = twin._loss(xM, yM, losses.SegObjective(reduction="mean_all"), pixel_weight=uM)
    want = float(want.detach())
    assert want > 0 and abs(float(l_unsup) - want) <= VALUE_GATE * abs(want)


@pytest.mark.parametrize("mix", [False, True])
def test_train_command_line_with_self_training(core, tmp_path, mix):
    """python -m segmif_amd.train --self-training in a fresh child process, the arguments of the ClassMix command test: it says
    what it is, logs the unlabelled loss and the confident share per line, and leaves both checkpoints with finite weights."""
    cmd = [sys.executable, "-m", "segmif_amd.train", "--synthetic", "8", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2",
           "--backbone", "mit_b1", "--crop-size", "64", "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", str(tmp_path),
           "--ema-decay", "0.9", "--self-training", "--st-threshold", "0.12"] + (["--st-mix", "--st-below", "ignore"] if mix else [])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = r.stdout
    announced = [ln for ln in out.splitlines() if ln.startswith("[train] --self-training (")]
    assert len(announced) == 1 and "NOT the reference's training" in announced[0] and "mIoU" in announced[0]
    assert ("--st-mix" in announced[0]) == mix
    seg_lines = [ln for ln in out.splitlines() if "segmentation iter 2/2" in ln]
    assert len(seg_lines) == 1 and " unlabelled " in seg_lines[0] and " confident " in seg_lines[0]
    share = float(seg_lines[0].split(" confident ")[1].split()[0])
    unl = float(seg_lines[0].split(" unlabelled ")[1].split()[0])
    assert 0.0 <= share <= 1.0 and np.isfinite(unl) and unl >= 0.0
    assert not any(" confident " in ln for ln in out.splitlines() if "fusion iter" in ln)  # the segmentation phase only
    assert sorted(os.listdir(tmp_path)) == ["model-fusion_add_final2.pth", "modelfusion-final2.pth"]
    for f in os.listdir(tmp_path):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
