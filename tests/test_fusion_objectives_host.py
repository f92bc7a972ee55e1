"""CPU-only checks of the table-driven fusion objectives (segmif_amd/core/loss.py over losses.fusion_objective):
  * every class, on CPU tensors, reproduces what the real reference's class gave (tests/golden/fusion_objectives.npz, recorded by
    tools/make_golden_fusion_objectives.py) - value within 1e-5 relative, gradient within 1e-4 of max |grad|, the bounds
    losses.npz and laploss.npz are held to.  L1 and max have discontinuous gradients; the fixture's inputs keep every argument of
    a sign and every difference inside a max at least `margin` >= 1e-5 from zero (float64), ten times what float32 rounding of
    the 8-tap sums can move, so no element is excluded;
  * a call without tensors raises NotImplementedError, the signatures are the reference's;
  * SegmifObjTerm / SegmifFusionObjective have gcc's layout; bad descriptors are refused before any launch.
No kernel is launched here."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _abi_headers as headers
VALUE_TOL, GRAD_TOL = 1e-5, 1e-4
THREE_ARG = ("Fusionloss", "Fusionloss_add")
FOUR_ARG = ("Fusionloss2", "Fusionloss4", "Fusionloss6", "Fusionloss_grad", "Fusionloss_grad2")
MASK_THIRD = ("Total_fusion_loss", "Total_fusion_loss2", "Total_fusion_loss3", "new_loss_sobel")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return {k: v for k, v in np.load(os.path.join(golden_dir, "fusion_objectives.npz")).items()}


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def call_class(name, t, gen):
    """the class `name` of segmif_amd.core on the fixture's tensors (dict of torch tensors), as the generator called the reference"""
    import segmif_amd.core as core
    fn = getattr(core, name)()
    if name in THREE_ARG:
        return fn(t["ir"], t["vis"], gen)
    if name in FOUR_ARG:
        return fn(t["ir"], t["vis"], gen, t["mask_soft"])
    return fn(t["ir"], t["vis"][:, :1] if name == "new_loss_sobel" else t["vis"], t["mask_bin"], gen)


def test_fixture_keeps_its_tie_margin(golden):
    assert float(golden["margin"]) >= 1e-5
    assert golden["gen"].shape == (3, 1, 37, 53) and golden["vis"].shape == golden["mask_soft"].shape == (3, 3, 37, 53)
    assert golden["gen"].min() < 0 and golden["gen"].max() > 1 and set(np.unique(golden["mask_bin"])) == {0.0, 1.0}


@pytest.mark.parametrize("name", THREE_ARG + FOUR_ARG + MASK_THIRD)
def test_class_reproduces_reference_on_cpu(golden, name):
    t = {k: torch.from_numpy(golden[k]) for k in ("ir", "vis", "mask_soft", "mask_bin")}
    gen = torch.from_numpy(golden["gen"]).clone().requires_grad_(True)
    v = call_class(name, t, gen)
    (g,) = torch.autograd.grad(v, gen)
    ref_v, ref_g = float(golden["value:" + name]), torch.from_numpy(golden["grad:" + name])
    ev = abs(float(v.detach()) - ref_v) / abs(ref_v)
    eg = float((g - ref_g).abs().max() / ref_g.abs().max())
    print(f"{name}: value rel {ev:.3e}, grad rel {eg:.3e}")
    assert ev <= VALUE_TOL and eg <= GRAD_TOL, (name, ev, eg)


def test_new_loss_sobel_is_what_upstream_computes(golden):
    """(B + B^2 D) + 0.85 (A + A^2 C) from the four means, in float64 - not the masked-gradient loss the names suggest"""
    from segmif_amd import losses
    ir, vis, m, gen = (torch.from_numpy(golden[k]).double() for k in ("ir", "vis", "mask_bin", "gen"))
    y, S = vis[:, :1], losses.sobel_xy
    A, B = ((m * gen - m * ir) ** 2).mean(), (((1 - m).abs() * gen - (1 - m).abs() * y) ** 2).mean()
    C, D = ((S(gen) - S(ir)) ** 2).mean(), ((S(gen) - S(y)) ** 2).mean()
    want = float((B + B * B * D) + 0.85 * (A + A * A * C))
    assert abs(want - float(golden["value:new_loss_sobel"])) <= VALUE_TOL * want
    assert abs(float(golden["value:Total_fusion_loss"]) - (1.2 * float(golden["value:Fusionloss"]) + 0.85 * want)) <= 2 * VALUE_TOL * float(golden["value:Total_fusion_loss"])


def test_signatures_and_calls_without_tensors():
    import segmif_amd.core as core
    from segmif_amd.core import loss
    names = THREE_ARG + FOUR_ARG + MASK_THIRD
    assert set(names) <= set(loss.__all__) and all(hasattr(core, n) for n in names)
    for n in FOUR_ARG:
        assert list(inspect.signature(getattr(core, n).forward).parameters)[1:] == ["image_ir", "image_vis", "generate_img", "mask"]
    for n in THREE_ARG:
        assert list(inspect.signature(getattr(core, n).forward).parameters)[1:4] == ["image_ir", "image_vis", "generate_img"]
    for n in MASK_THIRD[:3]:
        assert list(inspect.signature(getattr(core, n).forward).parameters)[1:] == ["image_ir", "image_vis", "mask", "generate_img"]
    assert list(inspect.signature(core.new_loss_sobel.forward).parameters)[1:] == ["ir", "vis", "mask_ir", "fused_img"]
    for n in names:
        with pytest.raises(NotImplementedError, match="torch tensors"):
            getattr(core, n)()(None)
        with pytest.raises(NotImplementedError):
            getattr(core, n)()()
    assert isinstance(core.Fusionloss_grad().lap, core.LapLoss2) and isinstance(core.Total_fusion_loss().fl, core.Fusionloss)


def test_table_validation_on_the_host():
    from segmif_amd import losses
    T = losses.ObjTerm
    x = torch.rand(1, 1, 5, 6)
    with pytest.raises(ValueError):
        losses.fusion_objective((), lambda m: m[0], x)
    with pytest.raises(ValueError):
        losses.fusion_objective((T("identity", "max"),) * 9, lambda m: m[0], x, x, x)
    with pytest.raises(ValueError):
        losses.fusion_objective((T("laplace", "max"),), lambda m: m[0], x, x, x)
    with pytest.raises(ValueError, match="vis"):
        losses.fusion_objective((T("identity", "max"),), lambda m: m[0], x, x)
    with pytest.raises(ValueError, match="mask"):
        losses.fusion_objective((T("identity", "linear", "mask", a_ir=1.0),), lambda m: m[0], x, x)
    # a 3-channel weight broadcasts: the mean runs over 3 x the pixels
    m3 = torch.rand(1, 3, 5, 6)
    got = losses.fusion_objective((T("identity", "linear", "inv_mask", "square", a_vis=1.0),), lambda m: m[0], x, None, 2 * x, m3)
    assert torch.allclose(got, (((1 - m3).abs() * (x - 2 * x)) ** 2).mean())


def test_objective_structs_match_c(lib, tmp_path):
    """(the two structs' layout: tests/test_abi_and_host.py::test_struct_layouts_match_c)"""
    from segmif_amd._lib import SegmifFusionObjective
    assert headers.c_ints("segmif_hip.h", ["SEGMIF_OBJ_MAX_TERMS"], tmp_path) == [len(SegmifFusionObjective().term)] == [8]


def test_bad_descriptors_are_refused_without_a_gpu(lib):
    """every refusal precedes the launch: with these arguments a launch would fail differently (there is no device here)"""
    from segmif_amd import autograd as ag, losses
    from segmif_amd._lib import SegmifFusionObjective
    EINVAL = -22
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def fwd(d, mask_planes=3, gen=p, ir=p, vis=p, mask=p):
        return lib.segmif_fusion_objective_f32(ctypes.byref(d), gen, ir, vis, mask, mask_planes, p, p, 1, 2, 2, None)

    def bwd(d, mask_planes=3):
        return lib.segmif_fusion_objective_bwd_f32(ctypes.byref(d), p, p, p, p, mask_planes, p, p, 1, 2, 2, None)

    good = (losses.ObjTerm("sobel", "max"), losses.ObjTerm("identity", "linear", "mask", "square", a_ir=1.0))
    for n_terms in (0, 9, -1):
        d = ag.objective_descriptor(good, 3)
        d.n_terms = n_terms
        assert fwd(d) == EINVAL and bwd(d) == EINVAL
    for field in ("op", "target", "rho", "weight"):
        for bad in (-1, 2 if field != "weight" else 3):
            d = ag.objective_descriptor(good, 3)
            setattr(d.term[0], field, bad)
            assert fwd(d) == EINVAL and bwd(d) == EINVAL, (field, bad)
    for mc in (0, 5, -3):
        d = ag.objective_descriptor(good, 3)
        d.term[1].mask_channels = mc
        assert fwd(d) == EINVAL and bwd(d) == EINVAL
    d = ag.objective_descriptor(good, 3)
    assert fwd(d, mask_planes=2) == EINVAL and fwd(d, mask_planes=5) == EINVAL   # fewer planes than a term sums over; more than 4
    assert fwd(d, mask=None) == EINVAL and fwd(d, ir=None) == EINVAL and fwd(d, gen=None) == EINVAL
    assert lib.segmif_fusion_objective_f32(ctypes.byref(d), p, p, p, p, 3, p, p, 0, 2, 2, None) == EINVAL
    assert lib.segmif_fusion_objective_f32(None, p, p, p, p, 3, p, p, 1, 2, 2, None) == EINVAL
    assert isinstance(d, SegmifFusionObjective) and lib.segmif_abi_version() == 4
    assert lib.segmif_fusion_objective_blocks(8, 480, 640) == 8 * 30 * 10 and lib.segmif_fusion_objective_blocks(1, 1, 1) == 1
    assert lib.segmif_fusion_objective_blocks(2, 33, 65) == 2 * 3 * 2 and lib.segmif_fusion_objective_blocks(0, 4, 4) == 0


def test_three_argument_classes_accept_the_trainer_hooks_fourth_argument():
    """FusionTrainer's hook calls (ir, vis_ycrcb, fused, mask3); Fusionloss / Fusionloss_add read the first three"""
    import segmif_amd.core as core
    x = torch.rand(1, 1, 6, 7)
    for cls in (core.Fusionloss, core.Fusionloss_add):
        v = cls()(x, x.repeat(1, 3, 1, 1), x * 0.5, None)
        assert v.dim() == 0 and torch.equal(v, cls()(x, x.repeat(1, 3, 1, 1), x * 0.5))
