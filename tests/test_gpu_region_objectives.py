"""GPU tests of the region objectives (csrc/region_objective.hip behind losses.RegionObjective and losses.SegLossSum).  The two
gates of tests/test_gpu_seg_objectives.py throughout:
    value      1e-5 relative
    gradient   5e-5 of the reference gradient's largest magnitude
against the float64 restatement of tests/_region_objective_ref.py (stable descending sort: ties by ascending row index), evaluated
at the float32 logits the kernels get.  Lovasz's gradient depends on the order of the errors, and float32 rounding may legitimately
swap two nearly equal ones, so the inputs come from a seed search on the CPU in float64: a seed is kept only if the float64
gradient changes by at most 1e-5 of its largest magnitude (0.2 of the gate) when the rows are ordered by the float32-rounded
errors, with either tie direction, or with the errors moved by +-2 float32 ulps in alternating row parity
(_region_objective_ref.order_sensitivity).  The value does not depend on the order."""
import functools

import numpy as np
import pytest
import torch

import _region_objective_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

VALUE_GATE, GRAD_GATE = 1e-5, 5e-5
ORDER_MARGIN = 1e-5
SHAPES = {"8x8_c2": ((1, 8, 8), 2), "2x24x40_c9": ((2, 24, 40), 9), "16x16_c32": ((1, 16, 16), 32),
          "3x150x203_c9": ((3, 150, 203), 9)}  # the last: 91 350 rows - no multiple of a block, beyond 2^16, 45 sort tiles
LARGE = "3x150x203_c9"
MODES = [(k, c) for k in ("lovasz", "dice") for c in ("present", "all")]


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core as c
    return c


def search(make, classes="present", tie_directions=True):
    """the first of 200 seeds whose inputs keep the Lovasz gradient's order margin -> (logits, labels, seed, sensitivity)"""
    for seed in range(200):
        x, y = make(seed)
        if x is None:
            continue
        s = ref.order_sensitivity(x.reshape(-1, x.shape[-1]), y.reshape(-1), classes=classes, tie_directions=tie_directions)
        if s <= ORDER_MARGIN:
            return x, y, seed, s
    raise RuntimeError("no seed keeps the order margin")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """logits (B, H, W, C) float32 and labels: imbalanced (a dominant class, a rare one of 5 pixels - 32 at the large shape - about
    10 % ignored), every class present"""
    shape, C = SHAPES[name]

    def make(seed):
        x, y = ref.make_inputs(seed, shape, C, rare=32 if name == LARGE else 5)
        return (x, y) if len(set(y.reshape(-1).tolist()) - {255}) == C else (None, None)

    return search(make)


@functools.lru_cache(maxsize=None)
def reference(name, kind, classes):
    """float64 value and gradient on inputs(name): computed once, shared"""
    x, y, _, _ = inputs(name)
    return ref.value_and_grad(x, y, kind, classes=classes)


def errors(v, g, ref_v, ref_g):
    v, g = float(v.detach() if torch.is_tensor(v) else v), g.detach().double().cpu()
    assert np.isfinite(v) and bool(torch.isfinite(g).all())
    return abs(v - float(ref_v)) / abs(float(ref_v)), float((g - ref_g).abs().max() / ref_g.abs().max())


def run_nhwc(module, x_dev, y_dev):
    x = x_dev.detach().requires_grad_(True)
    v = module.forward_nhwc(x, y_dev)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def check(tag, module, x, y, ref_v, ref_g, grad=True):
    v, g = run_nhwc(module, x.cuda(), y.cuda())
    ev, eg = errors(v, g, ref_v, ref_g)
    print(f"{tag}: value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and (eg <= GRAD_GATE or not grad), (tag, ev, eg)
    return v, g


# ---- 1. both objectives, both class sets, every shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,classes", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernels_against_float64(core, name, kind, classes):
    from segmif_amd.losses import RegionObjective
    x, y, seed, s = inputs(name)
    check(f"{name} {kind} {classes} (seed {seed}, order sensitivity {s:.1e})", RegionObjective(kind, classes), x, y,
          *reference(name, kind, classes))


# ---- 2. layouts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lovasz", "dice"])
@pytest.mark.parametrize("layout", ["slice_ld12", "channels_last_nchw", "contiguous_nchw"])
def test_layouts(core, layout, kind):
    from segmif_amd import ops
    from segmif_amd.losses import RegionObjective
    name = "2x24x40_c9"
    (shape, C), (x, y, _, _) = SHAPES[name], inputs(name)
    ref_v, ref_g = reference(name, kind, "present")
    module, y_dev = RegionObjective(kind), y.cuda()
    if layout == "slice_ld12":  # a channel slice of a wider buffer: pixel pitch 12, scalar accesses
        wide = torch.zeros(shape + (12,), device="cuda")
        wide[..., :C] = x.cuda()
        wide.requires_grad_(True)
        v = module.forward_nhwc(wide[..., :C], y_dev)
        (gw,) = torch.autograd.grad(v, wide)
        assert float(gw[..., C:].abs().max()) == 0.0
        g = gw[..., :C]
    elif layout == "channels_last_nchw":  # what ops.as_nchw returns: forward() takes the rows as they are - the same bits
        xv = x.cuda().requires_grad_(True)
        v = module(ops.as_nchw(xv), y_dev)
        (g,) = torch.autograd.grad(v, xv)
        v1, g1 = run_nhwc(module, x.cuda(), y_dev)
        assert torch.equal(v, v1) and torch.equal(g, g1)
    else:  # contiguous NCHW through forward(): the gradient comes back contiguous NCHW
        xn = x.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
        v = module(xn, y_dev)
        (gn,) = torch.autograd.grad(v, xn)
        assert gn.is_contiguous() and gn.shape == xn.shape
        g = gn.permute(0, 2, 3, 1)
    ev, eg = errors(v, g, ref_v, ref_g)
    print(f"{layout} {kind}: value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and eg <= GRAD_GATE, (layout, kind, ev, eg)


# ---- 3. added to cross entropy -----------------------------------------------------------------------------------------------------------
def test_sum_with_cross_entropy(core):
    from segmif_amd import autograd as ag
    from segmif_amd.losses import RegionObjective, SegLossSum
    name = "2x24x40_c9"
    x, y, _, _ = inputs(name)
    xd = x.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(xd.reshape(-1, 9), y.reshape(-1), ignore_index=255)
    want = ce + 0.5 * ref.objective(xd, y, "lovasz")
    (want_g,) = torch.autograd.grad(want, xd)
    module = SegLossSum(torch.nn.CrossEntropyLoss(ignore_index=255), RegionObjective("lovasz"), 0.5)
    check("CE + 0.5 lovasz", module, x, y, want.detach(), want_g)
    xb = x.cuda().requires_grad_(True)
    v_ce = module.base_nhwc(xb, y.cuda())
    (g_ce,) = torch.autograd.grad(v_ce, xb)
    xo = x.cuda().requires_grad_(True)
    vo = ag.softmax_ce(xo, y.cuda(), 255)
    (go,) = torch.autograd.grad(vo, xo)
    assert torch.equal(v_ce.detach(), vo.detach()) and torch.equal(g_ce, go)  # the CE term is the existing node's, bit for bit


# ---- 4. the tie rule ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tied_inputs():
    """the second image a copy of the first: every error has a bit-equal twin 960 rows on, in float32 and in float64.  (The search
    leaves the tie direction out of its orders - that is what the test is about - and the +-2 ulp moves keep twins together: 960
    is even.)"""
    def make(seed):
        x, y = ref.make_inputs(seed, (2, 24, 40), 9)
        x[1], y[1] = x[0], y[0]
        return x, y

    return search(make, tie_directions=False)


def test_ties_go_by_ascending_row_index(core):
    from segmif_amd.losses import RegionObjective
    x, y, seed, s = tied_inputs()
    ref_v, ref_g = ref.value_and_grad(x, y, "lovasz")
    _, other_g = ref.value_and_grad(x, y, "lovasz", order=ref._ties_descending)
    other = float((other_g - ref_g).abs().max() / ref_g.abs().max())
    assert other > 4 * GRAD_GATE, other  # the opposite tie order is a different gradient, several gates away
    check(f"ties (seed {seed}, order sensitivity {s:.1e}, descending ties differ by {other:.1e})", RegionObjective("lovasz"), x, y,
          ref_v, ref_g)


# ---- 5. saturation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lovasz", "dice"])
def test_saturated_rows(core, kind):
    """rows 100..163: the labelled logit at +30 (q ~ 1e-13), rows 200..263: a wrong logit at +30, rows 300..331 / 332..363: the same
    at +200, where float32 gives errors of exactly 0 and exactly 1.  float32 ties there that float64 does not have: the gradient
    is checked to be finite, the value against the gate."""
    from segmif_amd.losses import RegionObjective
    x, y, _, _ = inputs("2x24x40_c9")
    x, y = x.clone(), y.clone()
    X, Y = x.view(-1, 9), y.view(-1)
    for rows, right, height in ((range(100, 164), True, 30.0), (range(200, 264), False, 30.0), (range(300, 332), True, 200.0),
                                (range(332, 364), False, 200.0)):
        for r in rows:
            if Y[r] != 255:
                X[r, int(Y[r]) if right else (int(Y[r]) + 1) % 9] = height
    ref_v, ref_g = ref.value_and_grad(x, y, kind)
    check(f"saturated {kind}", RegionObjective(kind), x, y, ref_v, ref_g, grad=kind == "dice")


# ---- 6. absent classes, a single class, nothing valid ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def absent_inputs(only=None):
    """class 3 relabelled as class 4 (and class 8 out of range, which is ignored), or every valid pixel labelled `only`"""
    def make(seed):
        x, y = ref.make_inputs(seed, (2, 24, 40), 9)
        if only is None:
            y[y == 3] = 4
            y[y == 8] = 9
        else:
            y[y != 255] = only
        return x, y

    return search(make, classes="all")


@pytest.mark.parametrize("kind,classes", MODES)
@pytest.mark.parametrize("only", [None, 2])
def test_absent_classes(core, only, kind, classes):
    from segmif_amd.losses import RegionObjective
    x, y, seed, s = absent_inputs(only)
    ref_v, ref_g = ref.value_and_grad(x, y, kind, classes=classes)
    v, _ = check(f"{'classes 3, 8 absent' if only is None else 'class 2 alone'} {kind} {classes} (seed {seed})",
                 RegionObjective(kind, classes), x, y, ref_v, ref_g)
    if kind == "lovasz" and classes == "all" and only is None:  # an absent class's term is max_i p_ic
        p = torch.softmax(x.double().view(-1, 9)[y.view(-1) < 9], 1)
        terms = ref.value_and_grad(x, y, kind, classes="present")[0] * 7 + p[:, 3].max() + p[:, 8].max()
        assert abs(float(v) - float(terms) / 9) <= VALUE_GATE * float(terms) / 9


@pytest.mark.parametrize("kind,classes", MODES)
def test_all_pixels_ignored(core, kind, classes):
    from segmif_amd.losses import RegionObjective
    x = torch.randn(2, 19, 23, 9, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((2, 19, 23), 255, dtype=torch.int64).cuda()
    y[0, 0, :5] = 9  # outside [0, C): ignored as well
    v, g = run_nhwc(RegionObjective(kind, classes), x, y)
    assert float(v) == 0.0 and bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lovasz", "dice"])
def test_runs_are_bit_identical(core, kind):
    from segmif_amd.losses import RegionObjective
    x, y, _, _ = inputs(LARGE)
    module, xd, yd = RegionObjective(kind), x.cuda(), y.cuda()
    v1, g1 = run_nhwc(module, xd, yd)
    v2, g2 = run_nhwc(module, xd, yd)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    with torch.no_grad():
        v3 = module.forward_nhwc(xd, yd)
    assert torch.equal(v1, v3) and not v3.requires_grad


# ---- 8. through the segmentation net, eager and captured --------------------------------------------------------------------------------
def test_network_loss_and_graphed_step_with_lovasz(core):
    """Network3._loss with SegLossSum(CE, lovasz) is the restatement applied to the HIP bilinear output, and GraphedSegTrainStep with
    that criterion takes the eager step's two steps bitwise: the path has no host synchronisation, is capture-safe and
    deterministic (built as test_network_loss_and_graphed_step_with_ohem builds it)."""
    from segmif_amd import ops
    from segmif_amd.losses import RegionObjective, SegLossSum
    from segmif_amd.train import GraphedSegTrainStep, seg_train_step
    from segmif_amd.utils.optimizer import PolyWarmupAdamW_seg
    B, H, W = 2, 64, 96

    def make():
        net = core.Network3("mit_b1", 9, pretrained=None)
        dw.load_det_weights(net, seed=0)
        net = net.cuda().eval()
        g = net.denoise_net.get_param_groups()
        opt = PolyWarmupAdamW_seg([{"params": g[0], "lr": 8e-5, "weight_decay": 0.01}, {"params": g[1], "lr": 8e-5, "weight_decay": 0.0},
                                   {"params": g[2], "lr": 8e-4, "weight_decay": 0.01}], lr=8e-5, weight_decay=0.01, betas=(0.9, 0.999),
                                  iter_curr=10000, warmup_iter=3000, max_iter=160000, warmup_ratio=1e-6, power=1.0)
        return net, opt

    xs = [dw.det_input(f"ro_x{i}", (B, 3, H, W)).cuda() for i in range(2)]
    ys = []
    for i in range(2):
        y = dw.det_labels(f"ro_y{i}", (B, H, W), 9)
        y[:, 5:20, 7:40] = 255
        ys.append(y.cuda())
    crit = SegLossSum(torch.nn.CrossEntropyLoss(ignore_index=255), RegionObjective("lovasz")).cuda()
    net_e, opt_e = make()
    loss = net_e._loss(xs[0], ys[0], crit).detach()
    up = ops.bilinear(net_e._segment_nhwc(xs[0]).detach(), H, W).double().cpu()
    want = torch.nn.functional.cross_entropy(up.reshape(-1, 9), ys[0].cpu().reshape(-1), ignore_index=255) \
        + ref.objective(up, ys[0].cpu(), "lovasz")
    ev = abs(float(loss) - float(want)) / abs(float(want))
    print(f"Network3._loss with CE + lovasz: {float(loss):.8f} vs {float(want):.8f}, rel {ev:.3e}")
    assert ev <= VALUE_GATE
    losses_e = [float(seg_train_step(net_e, opt_e, x, y, crit)) for x, y in zip(xs, ys)]
    net_g, opt_g = make()
    step = GraphedSegTrainStep(net_g, opt_g, crit, xs[0], ys[0], warmup=1)
    losses_g = [float(step(x, y)) for x, y in zip(xs, ys)]
    assert losses_g == losses_e, (losses_g, losses_e)
    for (n, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), n
