"""GPU tests of the pixel- and sample-weighted segmentation objective (segmif_seg_objective_weighted_f32 / _bwd_f32 in
csrc/seg_objective.hip, behind ag.seg_objective(pixel_weight=, sample_weight=)) against the float64 restatement of
tests/_self_training_ref.py.  Gates: the project's existing ones (tests/test_gpu_seg_objectives.py) - value 1e-5 relative, gradient
5e-5 of the reference gradient's largest element.  Where the weighted entries must equal the unweighted path - both weights absent, or
all ones - loss and dlogits are compared through their bits."""
import functools

import pytest
import torch

import _self_training_ref as ref

pytestmark = pytest.mark.gpu

VALUE_GATE, GRAD_GATE = 1e-5, 5e-5
SHAPES = {"ragged": ((2, 19, 27), 9), "c32": ((2, 12, 16), 32)}  # 1026 rows: four blocks of 256 and two rows; the most classes
CONFIGS = {  # name: (SegObjective keyword arguments, restatement keyword arguments)
    "ce": (dict(), dict()),
    "ce_mean_all": (dict(reduction="mean_all"), dict(reduction="mean_all")),
    "weights_smooth": (dict(label_smoothing=0.1, weight="w"), dict(eps=0.1, weight="w")),
    "weights_smooth_mean_all": (dict(label_smoothing=0.1, weight="w", reduction="mean_all"), dict(eps=0.1, weight="w", reduction="mean_all")),
    "focal_g2": (dict(gamma=2.0), dict(gamma=2.0)),
    "focal_g2_mean_all": (dict(gamma=2.0, reduction="mean_all"), dict(gamma=2.0, reduction="mean_all")),
}
WEIGHTINGS = ("pixel", "sample", "both")


@pytest.fixture(scope="module")
def losses():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import losses as l
    return l


@functools.lru_cache(maxsize=None)
def inputs(shape_name):
    """logits (B, H, W, C) = 2 randn, labels with 255s and values outside [0, C), u in [0, 2] with exact zeros, sample weights
    in [0, 1]: host tensors, made once"""
    (B, H, W), C = SHAPES[shape_name]
    g = torch.Generator().manual_seed(11 + C)
    x = torch.randn(B, H, W, C, generator=g) * 2.0
    y = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64)
    r = torch.rand(B, H, W, generator=g)
    y[r < 0.12] = 255
    y[(r >= 0.12) & (r < 0.15)] = C + 3
    y[(r >= 0.15) & (r < 0.17)] = -1
    u = torch.rand(B, H, W, generator=g) * 2.0
    u[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    sw = torch.rand(B, generator=g)
    return x, y, u, sw


def class_weights(C):
    return torch.linspace(0.25, 2.0, C)


def kw_of(cfg, C, which):
    kw = dict(CONFIGS[cfg][which])
    if kw.get("weight") == "w":
        kw["weight"] = class_weights(C)
    return kw


def weights_of(shape_name, weighting):
    _, _, u, sw = inputs(shape_name)
    return (u if weighting in ("pixel", "both") else None), (sw if weighting in ("sample", "both") else None)


@functools.lru_cache(maxsize=None)
def reference(shape_name, cfg, weighting):
    x, y, _, _ = inputs(shape_name)
    pw, sw = weights_of(shape_name, weighting)
    return ref.weighted_value_and_grad(x, y, pixel_weight=pw, sample_weight=sw, **kw_of(cfg, x.shape[-1], 1))


def run(module, x, y, pw=None, sw=None):
    x = x.detach().requires_grad_(True)
    v = module.forward_nhwc(x, y, pixel_weight=pw, sample_weight=sw)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def dev(t):
    return None if t is None else t.cuda()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_value_and_gradient_against_float64(losses, shape_name, cfg, weighting):
    x, y, u, _ = inputs(shape_name)
    pw, sw = weights_of(shape_name, weighting)
    module = losses.SegObjective(**kw_of(cfg, x.shape[-1], 0)).cuda()
    v, g = run(module, x.cuda(), y.cuda(), dev(pw), dev(sw))
    ref_v, ref_g = reference(shape_name, cfg, weighting)
    ev = abs(float(v) - float(ref_v)) / abs(float(ref_v))
    eg = float((g.double().cpu() - ref_g).abs().max() / ref_g.abs().max())
    print(f"{shape_name} {cfg} {weighting}: value rel {ev:.3e}, gradient rel-to-max {eg:.3e}")
    assert bool(torch.isfinite(g).all()) and ev <= VALUE_GATE and eg <= GRAD_GATE
    if pw is not None:  # a row of weight 0 has an all-zero gradient, as an ignored one has
        dead = (u == 0) | (y == 255) | (y < 0) | (y >= x.shape[-1])
        assert int((u == 0).sum()) > 0 and bool((bits(g.cpu())[dead] == 0).all())


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_no_weights_and_unit_weights_give_the_unweighted_bits(losses, shape_name, cfg):
    import ctypes

    from segmif_amd import _lib, autograd as ag
    x, y, _, _ = inputs(shape_name)
    x, y = x.cuda(), y.cuda()
    B, C = x.shape[0], x.shape[-1]
    module = losses.SegObjective(**kw_of(cfg, C, 0)).cuda()
    v0, g0 = run(module, x, y)
    ones_p, ones_s = torch.ones(y.shape, device="cuda"), torch.ones(B, device="cuda")
    for pw, sw in ((ones_p, ones_s), (ones_p, None), (None, ones_s)):
        v1, g1 = run(module, x, y, pw, sw)
        assert torch.equal(bits(v1), bits(v0)) and torch.equal(bits(g1), bits(g0))
    # the weighted ENTRY POINTS with both weights NULL, called directly
    lib, rows = _lib.load(), y.numel()
    desc = ag.seg_objective_descriptor(module.gamma, module.label_smoothing, module.ignore_index, module.reduction)
    ws = torch.empty(lib.segmif_seg_objective_workspace_bytes(rows, desc.reduction), dtype=torch.uint8, device="cuda")
    rec, up, dlog = torch.empty(4, device="cuda"), torch.ones(1, device="cuda"), torch.empty_like(x)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = module.weight.data_ptr() if module.weight is not None else None
    assert lib.segmif_seg_objective_weighted_f32(ctypes.byref(desc), x.data_ptr(), y.data_ptr(), w, None, None, 0, ws.data_ptr(),
                                                 rec.data_ptr(), rows, C, C, stream) == 0
    assert lib.segmif_seg_objective_weighted_bwd_f32(ctypes.byref(desc), x.data_ptr(), y.data_ptr(), w, None, None, 0, None, rec.data_ptr(),
                                                     up.data_ptr(), dlog.data_ptr(), rows, C, C, C, stream) == 0
    assert torch.equal(bits(rec[0]), bits(v0)) and torch.equal(bits(dlog), bits(g0))


@pytest.mark.parametrize("cfg", ["ce", "ce_mean_all", "focal_g2_mean_all"])
def test_a_uniform_sample_weight_scales_and_does_not_cancel(losses, cfg):
    x, y, _, _ = inputs("ragged")
    x, y = x.cuda(), y.cuda()
    module = losses.SegObjective(**kw_of(cfg, x.shape[-1], 0)).cuda()
    v0, g0 = run(module, x, y)
    q = 0.37
    v, g = run(module, x, y, None, torch.full((x.shape[0],), q, device="cuda"))
    assert abs(float(v) - q * float(v0)) <= VALUE_GATE * q * abs(float(v0))
    assert float((g - q * g0).abs().max()) <= GRAD_GATE * q * float(g0.abs().max())


def test_what_is_not_built_raises(losses):
    import ctypes

    from segmif_amd import _lib, autograd as ag
    from segmif_amd.core.model_fusion import seg_criterion_loss
    x, y, u, sw = inputs("ragged")
    x, y, u, sw = x.cuda(), y.cuda(), u.cuda(), sw.cuda()
    B, H, W, C = x.shape
    ohem = losses.SegObjective(reduction="ohem", ohem_thresh=0.7, ohem_n_min=16).cuda()
    with pytest.raises(TypeError):
        ohem.forward_nhwc(x, y, pixel_weight=u)
    with pytest.raises(ValueError):
        ag.seg_objective(x, y, reduction="ohem", ohem_t=0.3, ohem_n_min=16, sample_weight=sw)
    # the entry points themselves: SEGMIF_EINVAL
    lib, rows = _lib.load(), y.numel()
    ws = torch.empty(lib.segmif_seg_objective_workspace_bytes(rows, 2), dtype=torch.uint8, device="cuda")
    rec = torch.empty(4, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(desc, pw, sw_, rps):
        return lib.segmif_seg_objective_weighted_f32(ctypes.byref(desc), x.data_ptr(), y.data_ptr(), None, pw, sw_, rps, ws.data_ptr(),
                                                     rec.data_ptr(), rows, C, C, stream)

    assert fwd(ag.seg_objective_descriptor(reduction="ohem", ohem_t=0.3, ohem_n_min=16), u.data_ptr(), None, 0) == -22
    mean = ag.seg_objective_descriptor()
    assert fwd(mean, None, sw.data_ptr(), 0) == -22 and fwd(mean, None, sw.data_ptr(), 7) == -22  # rows % 7 != 0
    assert fwd(mean, None, sw.data_ptr(), H * W) == 0
    # SegLossSum, RegionObjective and a criterion of the caller's take no weights
    low = torch.randn(B, 5, 7, C, device="cuda")
    region = losses.RegionObjective("dice")
    for crit in (losses.SegLossSum(torch.nn.CrossEntropyLoss(ignore_index=255), region), region, torch.nn.NLLLoss()):
        with pytest.raises(TypeError, match="not"):
            seg_criterion_loss(low, y, crit, sample_weight=sw)
    # a plain CrossEntropyLoss is routed through SegObjective.from_criterion
    v = seg_criterion_loss(low, y, torch.nn.CrossEntropyLoss(ignore_index=255), sample_weight=sw)
    up = torch.nn.functional.interpolate(low.permute(0, 3, 1, 2).double().cpu(), size=(H, W), mode="bilinear", align_corners=False)
    ref_v = ref.weighted_objective(up.permute(0, 2, 3, 1), y.cpu(), sample_weight=sw)
    assert abs(float(v) - float(ref_v)) <= 2 * VALUE_GATE * abs(float(ref_v))  # (the bilinear resize in float32 before it)
    # weights are data
    module = losses.SegObjective().cuda()
    with pytest.raises(RuntimeError, match="requires grad"):
        module.forward_nhwc(x, y, pixel_weight=u.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="requires grad"):
        module.forward_nhwc(x, y, sample_weight=sw.clone().requires_grad_(True))
