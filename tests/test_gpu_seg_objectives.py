"""GPU tests of the segmentation objectives (csrc/seg_objective.hip behind losses.SegObjective, core.OhemCELoss,
core.SoftmaxFocalLoss, core.NormalLoss).  Two gates throughout, the existing CE kernel's (tests/test_gpu_backward.py):
    value      1e-5 relative
    gradient   5e-5 of the reference gradient's largest magnitude
The references are the real reference classes' records (tests/golden/seg_objectives.npz) and the float64 restatement of
tests/_seg_objective_ref.py, which the host tests pin to those records at 1e-6.  OHEM selects pixels, so its inputs come from a
seed search (on the CPU, float64) that keeps every loss at least a margin away from the threshold and the k-th sorted loss a margin
above the (k+1)-th: 1e-4 for the small shapes, 1e-5 for the large one - float32 rounding of a loss of a few units is below 1e-6 - so
the kernels select the pixels the reference does and every gradient element is compared."""
import functools

import numpy as np
import pytest
import torch

import _seg_objective_ref as ref
import detweights as dw

pytestmark = pytest.mark.gpu

VALUE_GATE, GRAD_GATE = 1e-5, 5e-5
PUSHED = slice(100, 164)  # rows whose label's logit is set to +30: p_y -> 1, q -> 0


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core as c
    return c


def ohem_plan(logits, labels):
    """(thresh, n_min) of the four OHEM configurations for these inputs (classes last).  The top-k case uses thresh 0.05 (t = 3.0):
    at 32 classes every ordinary pixel's loss is above -log(0.7), which would leave no k between n_gt and the valid count; its k
    is half way between n_gt and the number of pixels with a loss to speak of (the pushed block's are ~1e-12)."""
    l, _, _ = ref.pixel_losses(logits.double().reshape(-1, logits.shape[-1]), labels.reshape(-1))
    n_hi, n_lo, n_real, rows = int((l > ref.ohem_t(0.7)).sum()), int((l > ref.ohem_t(0.05)).sum()), int((l > 1e-3).sum()), l.numel()
    assert n_lo < (n_lo + n_real) // 2 <= n_real
    return {"ohem_thresh": (0.7, max(1, n_hi // 4)), "ohem_topk": (0.05, (n_lo + n_real) // 2),
            "ohem_top1": (1e-30, 1), "ohem_all": (0.7, rows)}  # thresh 1e-30: no loss is above 69, so n_min = 1 is the top-k branch


@functools.lru_cache(maxsize=None)
def inputs(shape, C, margin, plan_names=("ohem_thresh", "ohem_topk", "ohem_top1", "ohem_all")):
    """logits (B, H, W, C) float32 and labels of the recorder's recipe, a block of pixels pushed to p_y -> 1, reseeded until every
    OHEM configuration keeps the selection margin in float64"""
    for seed in range(200):
        x, y = ref.make_inputs(seed, shape, C)
        x = x.permute(0, 2, 3, 1).contiguous()
        idx = torch.arange(PUSHED.start, PUSHED.stop)
        ok = y.view(-1)[idx] != 255
        x.view(-1, C)[idx[ok], y.view(-1)[idx[ok]]] = 30.0
        plan = ohem_plan(x, y)
        worst = min(min(ref.selection_margin(x, y, thresh=plan[n][0], n_min=plan[n][1])) for n in plan_names)
        if worst >= margin:
            return x, y, plan, seed, worst
    raise RuntimeError(f"no seed keeps a selection margin of {margin} at {shape} x {C}")


def class_weights(C):
    return torch.linspace(0.25, 2.0, C) if C > 1 else torch.ones(1)


def settings(name, C, plan):
    """config name -> (SegObjective keyword arguments, restatement keyword arguments)"""
    w = class_weights(C)
    table = {"ce": ({}, {}), "weights": (dict(weight=w), dict(weight=w)),
             "smooth_weights": (dict(label_smoothing=0.1, weight=w), dict(eps=0.1, weight=w)),
             "focal_g2": (dict(gamma=2.0), dict(gamma=2.0)), "focal_g05": (dict(gamma=0.5), dict(gamma=0.5)),
             "mean_all": (dict(reduction="mean_all"), dict(reduction="mean_all"))}
    if name in table:
        return table[name]
    thresh, n_min = plan[name]
    return dict(reduction="ohem", ohem_thresh=thresh, ohem_n_min=n_min), dict(reduction="ohem", thresh=thresh, n_min=n_min)


CONFIGS = ("ce", "weights", "smooth_weights", "focal_g2", "focal_g05", "mean_all", "ohem_thresh", "ohem_topk", "ohem_top1", "ohem_all")


@functools.lru_cache(maxsize=None)
def reference(shape, C, margin, name):
    """float64 value and gradient (classes last) of configuration `name` on inputs(shape, C, margin): computed once, shared"""
    x, y, plan, _, _ = inputs(shape, C, margin)
    return ref.value_and_grad(x, y, **settings(name, C, plan)[1])


def errors(v, g, ref_v, ref_g):
    v, g = float(v.detach() if torch.is_tensor(v) else v), g.detach().double().cpu()
    assert np.isfinite(v) and bool(torch.isfinite(g).all())
    return abs(v - float(ref_v)) / abs(float(ref_v)), float((g - ref_g).abs().max() / ref_g.abs().max())


def run_nhwc(module, x_dev, y_dev):
    x = x_dev.detach().requires_grad_(True)
    v = module.forward_nhwc(x, y_dev)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


# ---- 1. the classes of core/loss.py against the real reference's records ----------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    import os
    return {k: v for k, v in np.load(os.path.join(golden_dir, "seg_objectives.npz")).items()}


@pytest.mark.parametrize("name", ["normal", "focal_g2", "focal_g05", "ohem_thresh", "ohem_thresh_low", "ohem_topk_valid", "ohem_topk_ignored"])
def test_core_classes_reproduce_the_reference(core, golden, name):
    if name == "normal":
        fn = core.NormalLoss()
    elif name.startswith("focal"):
        fn = core.SoftmaxFocalLoss({"focal_g2": 2.0, "focal_g05": 0.5}[name])
    else:
        fn = core.OhemCELoss(float(golden["thresh:" + name]), int(golden["n_min:" + name]))
    x = torch.from_numpy(golden["logits"]).cuda().requires_grad_(True)  # contiguous NCHW, as the reference took it
    v = fn(x, torch.from_numpy(golden["labels"]).cuda())
    (g,) = torch.autograd.grad(v, x)
    assert g.shape == x.shape and g.is_contiguous()
    ev, eg = errors(v, g, golden["value:" + name], torch.from_numpy(golden["grad:" + name]).double())
    print(f"{name}: value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and eg <= GRAD_GATE, (name, ev, eg)


# ---- 2, 3. the kernel pair against the float64 restatement: shapes, layouts, configurations --------------------------------------------
SMALL = (2, 19, 23)      # 874 rows: four blocks, the last one ragged
RAGGED = (3, 37, 53)     # 5 883 rows, 36-byte rows at C = 9
LAYOUTS = {"nhwc_c9": (RAGGED, 9), "nhwc_c2": (SMALL, 2), "nhwc_c32": (SMALL, 32), "slice_ld12_c9": (RAGGED, 9), "nchw_c9": (RAGGED, 9)}


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_kernels_against_float64(core, layout, config):
    from segmif_amd.losses import SegObjective
    shape, C = LAYOUTS[layout]
    x, y, plan, seed, worst = inputs(shape, C, 1e-4)
    ref_v, ref_g = reference(shape, C, 1e-4, config)
    module = SegObjective(**settings(config, C, plan)[0]).cuda()
    y_dev = y.cuda()
    if layout == "slice_ld12_c9":  # a channel slice of a wider buffer: pixel pitch 12, rows not 16-byte aligned
        wide = torch.zeros(shape + (12,), device="cuda")
        wide[..., :C] = x.cuda()
        wide.requires_grad_(True)
        v = module.forward_nhwc(wide[..., :C], y_dev)
        (gw,) = torch.autograd.grad(v, wide)
        assert float(gw[..., C:].abs().max()) == 0.0
        g = gw[..., :C]
    elif layout == "nchw_c9":      # contiguous NCHW through forward(): the gradient comes back contiguous NCHW
        xn = x.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
        v = module(xn, y_dev)
        (gn,) = torch.autograd.grad(v, xn)
        assert gn.is_contiguous() and gn.shape == xn.shape
        g = gn.permute(0, 2, 3, 1)
    else:
        v, g = run_nhwc(module, x.cuda(), y_dev)
    ev, eg = errors(v, g, ref_v, ref_g)
    print(f"{layout} {config} (seed {seed}, margin {worst:.2e}): value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and eg <= GRAD_GATE, (layout, config, ev, eg)
    if config.startswith("focal"):
        # the pushed block on its own scale: q ~ 1e-12 there, the gradient ~ q^gamma.  float32 carries q through exp (argument
        # magnitude <= 40, so a relative 40 * 2^-24 = 2.4e-6 from the argument's rounding), a sum, a division and pow: 1e-4 of the
        # block's largest reference element bounds that with room; a 1 - p_y formulation gives 0 or inf here instead
        gb, rb = g.detach().double().cpu().reshape(-1, C)[PUSHED], ref_g.reshape(-1, C)[PUSHED]
        assert float(rb.abs().max()) > 0 and float((gb - rb).abs().max()) <= 1e-4 * float(rb.abs().max())


def test_channels_last_view_through_forward(core):
    """forward() on what ops.as_nchw returns is forward_nhwc on the rows: no copy, the same bits"""
    from segmif_amd import ops
    from segmif_amd.losses import SegObjective
    x, y, plan, _, _ = inputs(RAGGED, 9, 1e-4)
    module = SegObjective(gamma=2.0).cuda()
    v1, g1 = run_nhwc(module, x.cuda(), y.cuda())
    xv = x.cuda().requires_grad_(True)
    v2 = module(ops.as_nchw(xv), y.cuda())
    (g2,) = torch.autograd.grad(v2, xv)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


# ---- 4. more row blocks than a finalising block has threads -----------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["ohem_thresh", "ohem_topk"])
def test_large_ohem(core, config):
    from segmif_amd.losses import SegObjective
    shape, C = (2, 384, 384), 9   # 294 912 rows = 1 152 blocks: multi-round partial sums, histograms from many blocks
    x, y, plan, seed, worst = inputs(shape, C, 1e-5, ("ohem_thresh", "ohem_topk"))
    ref_v, ref_g = reference(shape, C, 1e-5, config)
    v, g = run_nhwc(SegObjective(**settings(config, C, plan)[0]).cuda(), x.cuda(), y.cuda())
    ev, eg = errors(v, g, ref_v, ref_g)
    print(f"large {config} (seed {seed}, margin {worst:.2e}, n_min {plan[config][1]}): value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and eg <= GRAD_GATE, (config, ev, eg)
    assert int((g.abs().sum(-1) > 0).sum()) == int((ref_g.abs().sum(-1) > 0).sum())  # the same number of selected pixels


# ---- 5. the plain-CE configuration against the node the default criterion runs on -------------------------------------------------------
def test_plain_ce_equals_the_existing_node(core):
    from segmif_amd import autograd as ag
    from segmif_amd.losses import SegObjective
    x, y, _, _, _ = inputs(RAGGED, 9, 1e-4)
    v, g = run_nhwc(SegObjective().cuda(), x.cuda(), y.cuda())
    xo = x.cuda().requires_grad_(True)
    vo = ag.softmax_ce(xo, y.cuda(), 255)
    (go,) = torch.autograd.grad(vo, xo)
    ev, eg = errors(v, g, vo.detach().double().cpu(), go.detach().double().cpu())
    print(f"new pair vs softmax_ce node: value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= VALUE_GATE and eg <= GRAD_GATE


# ---- 6. determinism, no_grad, batch decomposition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["smooth_weights", "focal_g05", "ohem_thresh", "ohem_topk"])
def test_runs_are_bit_identical(core, config):
    from segmif_amd.losses import SegObjective
    x, y, plan, _, _ = inputs(RAGGED, 9, 1e-4)
    module = SegObjective(**settings(config, 9, plan)[0]).cuda()
    xd, yd = x.cuda(), y.cuda()
    v1, g1 = run_nhwc(module, xd, yd)
    v2, g2 = run_nhwc(module, xd, yd)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    with torch.no_grad():
        v3 = module.forward_nhwc(xd, yd)
    assert torch.equal(v1, v3) and not v3.requires_grad


def test_mean_all_of_a_batch_is_the_mean_of_its_images(core):
    from segmif_amd.losses import SegObjective
    x, y, _, _, _ = inputs(RAGGED, 9, 1e-4)
    module = SegObjective(reduction="mean_all").cuda()
    xd, yd = x.cuda(), y.cuda()
    with torch.no_grad():
        whole = float(module.forward_nhwc(xd, yd))
        parts = [float(module.forward_nhwc(xd[b:b + 1], yd[b:b + 1])) for b in range(x.shape[0])]
    want = sum(parts) / len(parts)  # equal row counts: the row-weighted mean is the plain one
    assert abs(whole - want) <= VALUE_GATE * abs(want), (whole, parts)


# ---- 7. nothing valid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,want_nan", [(dict(), True), (dict(gamma=2.0), True), (dict(reduction="mean_all"), False),
                                         (dict(reduction="ohem", ohem_thresh=0.7, ohem_n_min=50), False)])
def test_all_pixels_ignored(core, kw, want_nan):
    from segmif_amd.losses import SegObjective
    x = torch.randn(2, 19, 23, 9, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.full((2, 19, 23), 255, dtype=torch.int64).cuda()
    y[0, 0, :5] = 9  # outside [0, C): ignored as well
    v, g = run_nhwc(SegObjective(**kw).cuda(), x, y)
    assert bool(torch.isnan(v)) if want_nan else float(v) == 0.0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
    if want_nan:  # as torch's
        assert bool(torch.isnan(torch.nn.functional.cross_entropy(x.permute(0, 3, 1, 2).cpu(), torch.full((2, 19, 23), 255), ignore_index=255)))


# ---- 8. through the segmentation net, eager and captured --------------------------------------------------------------------------------
def test_network_loss_and_graphed_step_with_ohem(core):
    """Network3._loss with OhemCELoss is the restatement applied to the HIP bilinear output, and GraphedSegTrainStep with that
    criterion takes the eager step's three steps bitwise: the path has no host synchronisation, is capture-safe and deterministic
    (eval-mode regime as in test_graphed_seg_train_step_equals_eager)."""
    from segmif_amd import ops
    from segmif_amd.train import GraphedSegTrainStep, seg_train_step
    from segmif_amd.utils.optimizer import PolyWarmupAdamW_seg
    B, H, W = 2, 64, 96
    n_min = B * H * W // 16

    def make():
        net = core.Network3("mit_b1", 9, pretrained=None)
        dw.load_det_weights(net, seed=0)
        net = net.cuda().eval()
        g = net.denoise_net.get_param_groups()
        opt = PolyWarmupAdamW_seg([{"params": g[0], "lr": 8e-5, "weight_decay": 0.01}, {"params": g[1], "lr": 8e-5, "weight_decay": 0.0},
                                   {"params": g[2], "lr": 8e-4, "weight_decay": 0.01}], lr=8e-5, weight_decay=0.01, betas=(0.9, 0.999),
                                  iter_curr=10000, warmup_iter=3000, max_iter=160000, warmup_ratio=1e-6, power=1.0)
        return net, opt

    xs = [dw.det_input(f"so_x{i}", (B, 3, H, W)).cuda() for i in range(3)]
    ys = []
    for i in range(3):
        y = dw.det_labels(f"so_y{i}", (B, H, W), 9)
        y[:, 5:20, 7:40] = 255
        ys.append(y.cuda())
    crit = core.OhemCELoss(0.7, n_min).cuda()
    net_e, opt_e = make()
    loss = net_e._loss(xs[0], ys[0], crit)
    up = ops.bilinear(net_e._segment_nhwc(xs[0]).detach(), H, W)
    want = ref.objective(up.double().cpu(), ys[0].cpu(), reduction="ohem", thresh=0.7, n_min=n_min)
    at_t, at_k = ref.selection_margin(up.cpu(), ys[0].cpu(), thresh=0.7, n_min=n_min)
    ev = abs(float(loss) - float(want)) / abs(float(want))
    print(f"Network3._loss with OHEM: {float(loss):.8f} vs {float(want):.8f}, rel {ev:.3e} (selection margins {at_t:.2e}, {at_k:.2e})")
    assert ev <= VALUE_GATE
    losses_e = [float(seg_train_step(net_e, opt_e, x, y, crit)) for x, y in zip(xs, ys)]
    net_g, opt_g = make()
    step = GraphedSegTrainStep(net_g, opt_g, crit, xs[0], ys[0], warmup=1)
    losses_g = [float(step(x, y)) for x, y in zip(xs, ys)]
    assert losses_g == losses_e, (losses_g, losses_e)
    for (n, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), n
