"""GPU tests of the table-driven fusion objectives (csrc/fusion_objective.hip through autograd.FusionObjectiveFn):
  * every class of core/loss.py on the device against the real reference's record (tests/golden/fusion_objectives.npz): value
    within 1e-5 relative, gradient within 1e-4 of max |grad| - the bounds of losses.npz / laploss.npz;
  * the kernel pair against the CPU formulation (losses.objective_means) in float64, same bounds, on an 8-term table that uses
    every op / target / weight / rho, at sizes below the halo, at exact tile multiples (the tile is 16 x 64), one pixel past a
    tile in both directions, odd sizes, mask_channels 1 and 3;
  * a 3-image batch equals its three images evaluated alone (the halo at a plane's edge is zero, never the neighbouring image);
  * the Fusionloss3 table on the new kernel equals losses.fusion_loss3 on the same device tensors;
  * no_grad and grad forwards agree bit for bit, two runs give bit-identical sums and gradients;
  * FusionTrainer's fusion_loss hook.
L1 and max have discontinuous gradients.  No element is excluded anywhere: every input set is seeded so that each argument of a
sign and each difference inside a max - gen - t, S gen - target, S ir - S vis, ir - vis, gx(gen), gy(gen), in float64 - is at least
1e-5 from zero, which each test asserts on the CPU first; float32 rounding of an 8-tap sum of values <= 1.4 is below 1e-6.  (An
argument that is EXACTLY zero in float64 is a sum of padding zeros only - the gradients of a 1-pixel-wide image - and is zero in
every precision; sign(0) = 0 in the kernel and in torch.)"""
import os

import numpy as np
import pytest
import torch

import detweights as dw
from _observed import observed

pytestmark = pytest.mark.gpu

VALUE_TOL, GRAD_TOL, MARGIN = 1e-5, 1e-4, 1e-5
THREE_ARG = ("Fusionloss", "Fusionloss_add")
FOUR_ARG = ("Fusionloss2", "Fusionloss4", "Fusionloss6", "Fusionloss_grad", "Fusionloss_grad2")
MASK_THIRD = ("Total_fusion_loss", "Total_fusion_loss2", "Total_fusion_loss3", "new_loss_sobel")


@pytest.fixture(scope="module")
def losses():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import losses as L
    return L


@pytest.fixture(scope="module")
def golden(golden_dir):
    return {k: v for k, v in np.load(os.path.join(golden_dir, "fusion_objectives.npz")).items()}


def all_terms(L):
    """eight terms: every op, target, weight and rho at least once, |.| and (.)^2 under both kinds of weight"""
    T = L.ObjTerm
    return (T("identity", "max"), T("sobel", "max"), T("identity", "linear", a_mask=1.0), T("sobel", "linear", a_ir=0.5, a_vis=0.5),
            T("identity", "linear", "mask", "square", a_ir=1.0), T("identity", "linear", "inv_mask", "square", a_vis=1.0),
            T("sobel", "linear", "one", "square", a_mask=1.0), T("identity", "linear", "mask", "abs", a_ir=0.6, a_vis=0.4))


WEIGHTS = (1.0, 8.0, 0.5, 4.0, 0.85, 1.0, 0.25, 1.5)


def combine_all(m):
    """a weighted sum plus a product of means (new_loss_sobel's kind): the coefficients of the backward depend on the sums"""
    w = torch.tensor(WEIGHTS, dtype=m.dtype, device=m.device)
    return (w * m).sum() + m[4] * m[4] * m[6] + m[5] * m[1]


def combine_linear(m):
    return (torch.tensor(WEIGHTS[:m.numel()], dtype=m.dtype, device=m.device) * m).sum()


def make_inputs(shape, mask_channels, seed, binary_mask=False):
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.rand(B, c, H, W, generator=g, dtype=torch.float32)
    ir, vis, mask, gen = r(1), r(1), r(mask_channels), r(1) * 1.4 - 0.2
    return gen, ir, vis, (mask > 0.5).float() if binary_mask else mask


def tie_margin(L, terms, gen, ir, vis, mask):
    """the smallest non-zero magnitude among the arguments of the signs and the differences inside the maxima, in float64"""
    gen, ir, vis, mask = (t.double() for t in (gen, ir, vis, mask))

    def parts(x):
        p = torch.nn.functional.pad(x, (1, 1, 1, 1))
        top, mid, bot = p[:, :, :-2], p[:, :, 1:-1], p[:, :, 2:]
        return ((top[..., 2:] + 2 * mid[..., 2:] + bot[..., 2:]) - (top[..., :-2] + 2 * mid[..., :-2] + bot[..., :-2]),
                (top[..., :-2] + 2 * top[..., 1:-1] + top[..., 2:]) - (bot[..., :-2] + 2 * bot[..., 1:-1] + bot[..., 2:]))

    args = []
    for t in terms:
        S = L.sobel_xy if t.op == "sobel" else (lambda z: z)
        if t.op == "sobel":
            args += list(parts(gen))
        if t.target == "max":
            args.append(S(ir) - S(vis))
            tgt = torch.maximum(S(ir), S(vis))
        else:
            tgt = S(t.a_ir * ir + t.a_vis * vis + t.a_mask * mask[:, :1])
        args.append(S(gen) - tgt)
    flat = torch.cat([a.reshape(-1) for a in args]).abs()
    flat = flat[flat > 0]
    return float(flat.min()) if flat.numel() else float("inf")


def reference64(L, terms, combine, gen, ir, vis, mask):
    x = gen.double().clone().requires_grad_(True)
    v = combine(L.objective_means(terms, x, ir.double(), vis.double(), mask.double()))
    (g,) = torch.autograd.grad(v, x)
    return float(v.detach()), g


def on_device(L, terms, combine, gen, ir, vis, mask):
    x = gen.cuda().requires_grad_(True)
    v = L.fusion_objective(terms, combine, x, ir.cuda(), vis.cuda(), mask.cuda())
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def errors(v, g, ref_v, ref_g):
    assert bool(torch.isfinite(g).all())
    return abs(float(v) - ref_v) / abs(ref_v), float((g.double().cpu() - ref_g.double()).abs().max() / ref_g.double().abs().max())


# ---- 1. the classes against the reference's record --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE_ARG + FOUR_ARG + MASK_THIRD)
def test_class_reproduces_reference_on_device(losses, golden, name):
    import segmif_amd.core as core
    assert float(golden["margin"]) >= MARGIN
    t = {k: torch.from_numpy(golden[k]).cuda() for k in ("ir", "vis", "mask_soft", "mask_bin")}
    gen = torch.from_numpy(golden["gen"]).cuda().requires_grad_(True)
    fn = getattr(core, name)()
    if name in THREE_ARG:
        v = fn(t["ir"], t["vis"], gen)
    elif name in FOUR_ARG:
        v = fn(t["ir"], t["vis"], gen, t["mask_soft"])
    else:
        v = fn(t["ir"], t["vis"][:, :1] if name == "new_loss_sobel" else t["vis"], t["mask_bin"], gen)
    (g,) = torch.autograd.grad(v, gen)
    ev, eg = errors(v.detach(), g, float(golden["value:" + name]), torch.from_numpy(golden["grad:" + name]))
    print(f"{name}: value rel {ev:.3e}, grad rel {eg:.3e}")
    observed(f"fusion_objective_class_vs_reference[{name}]", {"value_rel": ev, "grad_rel": eg})
    assert ev <= VALUE_TOL and eg <= GRAD_TOL, (name, ev, eg)


# ---- 2. the kernel pair against the float64 CPU formulation ------------------------------------------------------------------------
# (shape, mask_channels, seed): (3,1,37,53) odd, several tiles per row group; (2,1,5,3) and (1,1,1,1) smaller than the halo;
# (1,1,32,128) exact tile multiples (16-byte rows); (2,1,33,65) one pixel past a tile both ways; (1,1,16,68) 16-byte rows that end
# inside a tile
CASES = [((3, 1, 37, 53), 1, 0), ((3, 1, 37, 53), 3, 1), ((2, 1, 5, 3), 3, 0), ((1, 1, 1, 1), 1, 0), ((1, 1, 32, 128), 3, 0),
         ((2, 1, 33, 65), 1, 3), ((2, 1, 33, 65), 3, 2), ((1, 1, 16, 68), 4, 0)]


@pytest.mark.parametrize("shape,mc,seed", CASES)
def test_kernel_vs_float64_formulation(losses, shape, mc, seed):
    terms = all_terms(losses)
    gen, ir, vis, mask = make_inputs(shape, mc, seed)
    margin = tie_margin(losses, terms, gen, ir, vis, mask)
    assert margin >= MARGIN, margin
    ref_v, ref_g = reference64(losses, terms, combine_all, gen, ir, vis, mask)
    v, g = on_device(losses, terms, combine_all, gen, ir, vis, mask)
    ev, eg = errors(v, g, ref_v, ref_g)
    tag = "x".join(map(str, shape)) + f",mc{mc}"
    print(f"{tag}: margin {margin:.3e}, value rel {ev:.3e}, grad rel {eg:.3e}")
    observed(f"fusion_objective_kernel_vs_fp64[{tag}]", {"value_rel": ev, "grad_rel": eg, "margin": margin})
    assert ev <= VALUE_TOL and eg <= GRAD_TOL, (tag, ev, eg)


def test_batch_equals_its_images_alone(losses):
    """the halo at a plane's edge is zero, never the neighbouring image (or the neighbouring mask channel)"""
    terms = all_terms(losses)
    gen, ir, vis, mask = make_inputs((3, 1, 37, 53), 3, 1)
    assert tie_margin(losses, terms, gen, ir, vis, mask) >= MARGIN
    v, g = on_device(losses, terms, combine_linear, gen, ir, vis, mask)
    singles = [on_device(losses, terms, combine_linear, *(t[b:b + 1] for t in (gen, ir, vis, mask))) for b in range(3)]
    mean = sum(float(s[0]) for s in singles) / 3
    ev = abs(float(v) - mean) / abs(mean)
    g1 = torch.cat([s[1] for s in singles]) / 3          # (a mean over 3 x the pixels)
    eg = float((g - g1).abs().max() / g1.abs().max())
    observed("fusion_objective_batch_vs_single_images", {"value_rel": ev, "grad_rel": eg})
    assert ev <= VALUE_TOL and eg <= GRAD_TOL, (ev, eg)


def test_fusionloss3_table_equals_the_dedicated_kernels(losses):
    T = losses.ObjTerm
    terms = (T("identity", "linear", a_mask=1.0), T("sobel", "linear", a_mask=1.0))
    gen, ir, vis, mask = make_inputs((3, 1, 37, 53), 3, 1)
    assert tie_margin(losses, terms, gen, ir, vis, mask) >= MARGIN
    x = gen.cuda().requires_grad_(True)
    want = losses.fusion_loss3(x, mask.cuda())
    (gw,) = torch.autograd.grad(want, x)
    v = losses.fusion_objective(terms, lambda m: m[0] + m[1], x, None, None, mask.cuda()[:, :1])
    (g,) = torch.autograd.grad(v, x)
    ev, eg = errors(v.detach(), g, float(want.detach()), gw.cpu())
    observed("fusion_objective_fusionloss3_table_vs_sobel_l1", {"value_rel": ev, "grad_rel": eg})
    assert ev <= VALUE_TOL and eg <= GRAD_TOL, (ev, eg)


def test_no_grad_forward_and_repeat_runs_are_bit_identical(losses):
    terms = all_terms(losses)
    gen, ir, vis, mask = (t.cuda() for t in make_inputs((2, 1, 33, 65), 3, 0))
    with torch.no_grad():
        v0 = losses.fusion_objective(terms, combine_all, gen, ir, vis, mask)
    runs = [on_device(losses, terms, combine_all, gen.cpu(), ir.cpu(), vis.cpu(), mask.cpu()) for _ in range(2)]
    assert torch.equal(v0, runs[0][0]) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the sums themselves, straight from the library
    import ctypes
    from segmif_amd import _lib, autograd as ag
    lib = _lib.load()
    d = ag.objective_descriptor(terms, 3)
    nblk = lib.segmif_fusion_objective_blocks(2, 33, 65)
    out = []
    for _ in range(2):
        part = torch.empty(8 * nblk, device="cuda", dtype=torch.float64)
        sums = torch.full((8,), float("nan"), device="cuda", dtype=torch.float64)
        _lib.check(lib.segmif_fusion_objective_f32(ctypes.byref(d), gen.data_ptr(), ir.data_ptr(), vis.data_ptr(), mask.data_ptr(), 3,
                                                   part.data_ptr(), sums.data_ptr(), 2, 33, 65, None), "segmif_fusion_objective_f32")
        torch.cuda.synchronize()
        out.append(sums)
    assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out[0]).all()) and bool((out[0] > 0).all())


def test_device_tensors_the_kernel_does_not_cover_are_refused(losses):
    import segmif_amd.core as core
    x = torch.rand(1, 1, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="no torch fallback"):
        core.Fusionloss()(x.double(), x.double(), x.double())
    with pytest.raises(RuntimeError, match="no torch fallback"):
        core.Fusionloss2()(x, x, x, torch.rand(1, 1, 8, 8))            # the mask left on the host
    with pytest.raises(RuntimeError, match="no torch fallback"):
        core.new_loss_sobel()(x, x, torch.rand(1, 5, 8, 8, device="cuda"), x)   # five mask channels


# ---- 3. FusionTrainer's hook -------------------------------------------------------------------------------------------------------
# 32 x 48, the size of the other FusionTrainer tests: the smallest at which a step runs at all.  (At 24 x 40, the size of the
# fusion net's own gradient fixture, the segmentation encoder's stage-1 attention would reduce a 6 x 10 map by 8 - no output
# row, which the convolution refuses; that fixture feeds the fusion net recorded features instead of running the encoder.)
TRAIN_HW = (32, 48)


@pytest.fixture(scope="module")
def nets(losses):
    from segmif_amd.core import Fusion_Network3_ac, Network3
    seg = Network3("mit_b1", 9, pretrained=None)
    fus = Fusion_Network3_ac()
    dw.load_det_weights(seg, seed=0)
    dw.load_det_weights(fus, seed=0)
    seg, fus = seg.cuda().eval(), fus.cuda().train()
    return seg, fus, {k: v.clone() for k, v in fus.state_dict().items()}


def one_step(nets, iter_, fusion_loss):
    from segmif_amd.train import FusionTrainer
    seg, fus, state = nets
    fus.load_state_dict(state)
    for p in fus.parameters():
        p.grad = None
    B, (H, W) = 2, TRAIN_HW
    ir3 = dw.det_input("fo_ir", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
    vis3 = dw.det_input("fo_vis", (B, 3, H, W)).cuda()
    mask3 = dw.det_input("fo_mask", (B, 1, H, W)).repeat(1, 3, 1, 1).cuda()
    labels = dw.det_labels("fo_y", (B, H, W), 9).cuda()
    opt = torch.optim.AdamW(fus.parameters(), lr=1e-4, weight_decay=0.0)
    tr = FusionTrainer(seg, fus, opt, torch.nn.CrossEntropyLoss(ignore_index=255), iter_=iter_, fusion_loss=fusion_loss)
    loss = tr.step(ir3, vis3, mask3, labels)
    return loss, {n: p.detach().clone() for n, p in fus.named_parameters()}, (ir3, vis3)


@pytest.mark.parametrize("iter_,name", [(2, "Fusionloss_grad3"), (1, "Fusionloss3")])
def test_trainer_hook_with_the_default_objective_changes_nothing(nets, iter_, name):
    import segmif_amd.core as core
    loss0, p0, _ = one_step(nets, iter_, None)
    loss1, p1, _ = one_step(nets, iter_, getattr(core, name)())
    assert torch.equal(loss0, loss1) and bool(torch.isfinite(loss0))
    assert all(torch.equal(p0[n], p1[n]) for n in p0)


def test_trainer_step_on_fusionloss(nets, losses):
    """iter_ = 1: the step's loss IS the objective - equal to the CPU formulation on the step's own fused output within 1e-5 relative; every
    fusion-net parameter that takes part in the forward receives a finite gradient and moves"""
    import segmif_amd.core as core
    from segmif_amd.core.model_fusion import RGB2YCrCb
    seen = {}
    fl = core.Fusionloss()

    def hook(ir, vis, fused, mask3):
        seen["fused"], seen["ir"], seen["vis"] = fused.detach().clone(), ir, vis
        return fl(ir, vis, fused, mask3)

    seg, fus, state = nets
    loss, after, (ir3, vis3) = one_step(nets, 1, hook)
    fused, ir, y = seen["fused"].double().cpu(), seen["ir"][:, :1].double().cpu(), seen["vis"][:, :1].double().cpu()
    assert torch.equal(seen["vis"], RGB2YCrCb(vis3)) and fused.shape == (2, 1) + TRAIN_HW
    want = float(fl(ir, y, fused))
    e = abs(float(loss) - want) / abs(want)
    observed("fusion_objective_trainer_fusionloss_vs_cpu", e)
    assert e <= VALUE_TOL, (float(loss), want)
    n = 0
    for pn, p in fus.named_parameters():
        if pn.startswith("ffm2."):  # (no forward of Fusion_Network3_ac reads ffm2, in the reference either: train_fusion_b1.npz)
            assert p.grad is None, pn
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and not torch.equal(after[pn], state[pn]), pn
        n += 1
    assert n > 20
