"""CPU-only checks of the segmentation objectives (csrc/seg_objective.hip behind losses.SegObjective and core/loss.py's OhemCELoss,
SoftmaxFocalLoss, NormalLoss):
  * the float64 restatement the GPU tests hold the kernels against (tests/_seg_objective_ref.py) reproduces every value and gradient
    the REAL reference classes gave (tests/golden/seg_objectives.npz, recorded by tools/make_golden_seg_objectives.py).  Gate 1e-6:
    the reference's own float32 is within 2e-7 relative (values) and 3.3e-7 of max |grad| (gradients) of its float64 on such inputs;
  * its weighted / smoothed cross entropy is torch's F.cross_entropy in float64;
  * SegmifSegObjective has gcc's layout; every invalid descriptor is refused before any launch;
  * the classes have the reference's signatures; make_seg_loss / seg_loss_names / the command line refuse what they should;
  * CPU tensors raise RuntimeError (there is no torch formulation in the package).
No kernel is launched here."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _abi_headers as headers
import _seg_objective_ref as ref

GATE = 1e-6
CASES = {"normal": dict(reduction="mean_all"), "focal_g2": dict(gamma=2.0), "focal_g05": dict(gamma=0.5)}
OHEM_CASES = ("ohem_thresh", "ohem_thresh_low", "ohem_topk_valid", "ohem_topk_ignored")
EINVAL = -22


@pytest.fixture(scope="module")
def golden(golden_dir):
    return {k: v for k, v in np.load(os.path.join(golden_dir, "seg_objectives.npz")).items()}


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def case_settings(golden, name):
    if name in CASES:
        return dict(CASES[name])
    return dict(reduction="ohem", thresh=float(golden["thresh:" + name]), n_min=int(golden["n_min:" + name]))


def test_fixture_is_what_the_recorder_promises(golden):
    assert golden["logits"].shape == (2, 9, 29, 41) and golden["labels"].shape == (2, 29, 41) and golden["labels"].dtype == np.int64
    assert float(golden["margin"]) >= 1e-4
    frac = float((golden["labels"] == 255).mean())
    assert 0.10 < frac < 0.20 and set(np.unique(golden["labels"])) == set(range(9)) | {255}
    assert all(v.dtype.kind in "fi" for v in golden.values())  # arrays only
    x, y = torch.from_numpy(golden["logits"]).double(), torch.from_numpy(golden["labels"])
    l = F.cross_entropy(x, y, ignore_index=255, reduction="none").view(-1)
    n_valid, rows = int((y != 255).sum()), l.numel()
    # the four OHEM cases take the branches their names say
    for name, hard_branch in (("ohem_thresh", True), ("ohem_thresh_low", True), ("ohem_topk_valid", False), ("ohem_topk_ignored", False)):
        t, n_min = ref.ohem_t(float(golden["thresh:" + name])), int(golden["n_min:" + name])
        assert (int((l > t).sum()) >= n_min) == hard_branch, name
    assert int(golden["n_min:ohem_topk_valid"]) <= n_valid < int(golden["n_min:ohem_topk_ignored"]) == rows - 100


@pytest.mark.parametrize("name", tuple(CASES) + OHEM_CASES)
def test_restatement_reproduces_the_reference(golden, name):
    x = torch.from_numpy(golden["logits"]).permute(0, 2, 3, 1)
    v, g = ref.value_and_grad(x, torch.from_numpy(golden["labels"]), **case_settings(golden, name))
    ref_v, ref_g = float(golden["value:" + name]), torch.from_numpy(golden["grad:" + name]).double().permute(0, 2, 3, 1)
    ev = abs(float(v) - ref_v) / abs(ref_v)
    eg = float((g - ref_g).abs().max() / ref_g.abs().max())
    print(f"{name}: value rel {ev:.3e}, grad / max |grad| {eg:.3e}")
    assert ev <= GATE and eg <= GATE, (name, ev, eg)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_ce_is_torchs(golden, eps, weighted):
    x = torch.from_numpy(golden["logits"]).double().permute(0, 2, 3, 1).reshape(-1, 9)
    y = torch.from_numpy(golden["labels"]).reshape(-1)
    w = torch.linspace(0.25, 2.0, 9, dtype=torch.float64) if weighted else None
    l, w_y, valid = ref.pixel_losses(x, y, eps=eps, weight=w)
    want = F.cross_entropy(x, y, weight=w, ignore_index=255, label_smoothing=eps, reduction="none")
    assert float((l - want).abs().max()) <= 1e-12
    got_mean = ref.reduce_losses(l, w_y, "mean")
    want_mean = F.cross_entropy(x, y, weight=w, ignore_index=255, label_smoothing=eps)
    assert abs(float(got_mean - want_mean)) <= 1e-12 * float(want_mean)
    assert int(valid.sum()) == int((y != 255).sum())


def test_restatement_ohem_formula_without_the_sort(golden):
    """the identity the kernels use: with kappa the n_min-th largest, top-k sum = sum_{l > kappa} l + (n_min - #{l > kappa}) kappa"""
    x = torch.from_numpy(golden["logits"]).double().permute(0, 2, 3, 1).reshape(-1, 9)
    l, w_y, _ = ref.pixel_losses(x, torch.from_numpy(golden["labels"]).reshape(-1))
    for n_min in (1, 7, int(golden["n_min:ohem_topk_valid"]), l.numel() - 100, l.numel()):
        kappa = torch.sort(l, descending=True).values[n_min - 1]
        above = l[l > kappa]
        got = (above.sum() + (n_min - above.numel()) * kappa) / n_min
        want = ref.reduce_losses(l, w_y, "ohem", t=1e30, n_min=n_min)
        assert abs(float(got - want)) <= 1e-13 * max(1.0, float(want))


def test_struct_layout_matches_c(lib, tmp_path):
    """the header's enum values against autograd's (the struct's layout: tests/test_abi_and_host.py::test_struct_layouts_match_c)"""
    assert headers.c_ints("segmif_hip.h", ["SEGMIF_SEG_MEAN_VALID", "SEGMIF_SEG_MEAN_ALL", "SEGMIF_SEG_OHEM"], tmp_path) == [0, 1, 2]
    from segmif_amd import autograd as ag
    assert ag._SEG_REDUCTIONS == {"mean": 0, "mean_all": 1, "ohem": 2}


def test_bad_descriptors_are_refused_without_a_gpu(lib):
    """every refusal precedes the launch: with these arguments a launch would fail differently (there is no device here)"""
    from segmif_amd import autograd as ag
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ROWS = 100

    def fwd(d, C=9, ld=9, rows=ROWS):
        return lib.segmif_seg_objective_f32(ctypes.byref(d), p, p, None, p, p, rows, C, ld, None)

    def bwd(d, C=9, ld=9, ldd=9, rows=ROWS):
        return lib.segmif_seg_objective_bwd_f32(ctypes.byref(d), p, p, None, p, p, p, p, rows, C, ld, ldd, None)

    def refused(d, **kw):
        return fwd(d, **kw) == EINVAL and bwd(d, **kw) == EINVAL

    good = lambda **kw: ag.seg_objective_descriptor(**kw)
    for C in (0, -1, 33):
        assert refused(good(), C=C, ld=40)
    assert refused(good(), C=9, ld=8)
    assert bwd(good(), ldd=8) == EINVAL
    for gamma in (-0.5, float("nan"), float("inf")):
        assert refused(good(gamma=gamma))
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        assert refused(good(label_smoothing=eps))
    assert refused(good(gamma=2.0, label_smoothing=0.1))
    for red in (-1, 3, 17):
        d = good()
        d.reduction = red
        assert refused(d)
        assert lib.segmif_seg_objective_workspace_bytes(ROWS, red) == 0
    t = ref.ohem_t(0.7)
    for n_min in (0, -4, ROWS + 1):
        assert refused(good(reduction="ohem", ohem_t=t, ohem_n_min=n_min))
    for bad_t in (float("inf"), float("nan")):
        assert refused(good(reduction="ohem", ohem_t=bad_t, ohem_n_min=5))
    assert refused(good(), rows=0)
    assert lib.segmif_seg_objective_f32(None, p, p, None, p, p, ROWS, 9, 9, None) == EINVAL
    assert lib.segmif_seg_objective_workspace_bytes(0, 0) == 0
    # the workspace: a fixed header, five doubles per block of 256 rows, and for OHEM one float per row
    plain, ohem = lib.segmif_seg_objective_workspace_bytes(5883, 0), lib.segmif_seg_objective_workspace_bytes(5883, 2)
    assert ohem - plain == 4 * 5883 and plain == lib.segmif_seg_objective_workspace_bytes(5883, 1)
    assert plain - lib.segmif_seg_objective_workspace_bytes(5883 - 256, 0) == 5 * 8


def test_module_settings_are_validated():
    from segmif_amd.losses import SegObjective
    for kw in (dict(gamma=-1.0), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(gamma=2.0, label_smoothing=0.1),
               dict(reduction="sum"), dict(reduction="ohem"), dict(reduction="ohem", ohem_thresh=0.7),
               dict(reduction="ohem", ohem_thresh=0.0, ohem_n_min=4), dict(reduction="ohem", ohem_thresh=0.7, ohem_n_min=0),
               dict(ohem_thresh=0.7), dict(weight=[1.0, -0.5, 1.0]), dict(weight=[[1.0, 2.0]]), dict(weight=[float("nan")])):
        with pytest.raises(ValueError):
            SegObjective(**kw)
    m = SegObjective(weight=[1.0, 2.0, 0.0], reduction="ohem", ohem_thresh=0.7, ohem_n_min=16)
    assert "weight" in dict(m.named_buffers()) and m.weight.dtype == torch.float32 and not list(m.parameters())
    assert m.ohem_t == ref.ohem_t(0.7) and math.isclose(m.ohem_t, -math.log(0.7), rel_tol=1e-6) and m.ohem_n_min == 16
    c = SegObjective.from_criterion(torch.nn.CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]), ignore_index=7, label_smoothing=0.2))
    assert c.reduction == "mean" and c.ignore_index == 7 and c.label_smoothing == 0.2 and c.weight.tolist() == [1.0, 3.0]
    with pytest.raises(ValueError):
        SegObjective.from_criterion(torch.nn.CrossEntropyLoss(reduction="sum"))
    with pytest.raises(TypeError):
        SegObjective.from_criterion(torch.nn.NLLLoss())


def test_reference_named_classes_and_signatures():
    import segmif_amd.core as core
    from segmif_amd import losses
    from segmif_amd.core import loss
    names = ("OhemCELoss", "SoftmaxFocalLoss", "NormalLoss")
    assert set(names) <= set(loss.__all__) and all(hasattr(core, n) for n in names)
    assert list(inspect.signature(core.OhemCELoss.__init__).parameters)[1:4] == ["thresh", "n_min", "ignore_lb"]
    assert list(inspect.signature(core.SoftmaxFocalLoss.__init__).parameters)[1:3] == ["gamma", "ignore_lb"]
    assert list(inspect.signature(core.NormalLoss.__init__).parameters)[1:2] == ["ignore_lb"]
    for n in names:
        assert list(inspect.signature(getattr(core, n).forward).parameters)[1:] == ["logits", "labels"]
        assert inspect.signature(getattr(core, n).__init__).parameters["ignore_lb"].default == 255
    o, f, n = core.OhemCELoss(0.7, 50), core.SoftmaxFocalLoss(2.0, 11), core.NormalLoss()
    for m in (o, f, n):
        assert isinstance(m.objective, losses.SegObjective)
    assert (o.objective.reduction, o.n_min, o.thresh, o.ignore_lb) == ("ohem", 50, ref.ohem_t(0.7), 255)
    assert (f.objective.gamma, f.objective.reduction, f.objective.ignore_index) == (2.0, "mean", 11)
    assert (n.objective.gamma, n.objective.reduction, n.objective.label_smoothing) == (0.0, "mean_all", 0.0)
    assert "Left out: IQALoss" in loss.__doc__ and "OhemCELoss" not in loss.__doc__.split("Left out:")[1]


def test_cpu_tensors_raise():
    import segmif_amd.core as core
    from segmif_amd import autograd as ag, losses
    x, y = torch.randn(1, 9, 4, 5), torch.zeros(1, 4, 5, dtype=torch.long)
    for m in (core.OhemCELoss(0.7, 3), core.SoftmaxFocalLoss(2.0), core.NormalLoss(), losses.SegObjective(label_smoothing=0.1)):
        with pytest.raises(RuntimeError, match="MI355X"):
            m(x, y)
        with pytest.raises(RuntimeError, match="MI355X"):
            m.forward_nhwc(x.permute(0, 2, 3, 1), y)
    with pytest.raises(RuntimeError):
        ag.seg_objective(x.permute(0, 2, 3, 1).double(), y)


def test_make_seg_loss_and_names():
    import segmif_amd.core as core
    from segmif_amd import losses, train
    assert train.seg_loss_names() == ["ce", "ohem", "focal", "normal", "weighted"]
    ce = train.make_seg_loss("ce")
    assert type(ce) is torch.nn.CrossEntropyLoss and ce.ignore_index == 255 and ce.weight is None and ce.label_smoothing == 0.0
    assert isinstance(train.make_seg_loss("ohem", ohem_thresh=0.6, ohem_n_min=9), core.OhemCELoss)
    assert train.make_seg_loss("focal", focal_gamma=1.5).objective.gamma == 1.5
    assert isinstance(train.make_seg_loss("normal"), core.NormalLoss)
    w = train.make_seg_loss("weighted", class_weights=[1.0] * 9, label_smoothing=0.05)
    assert isinstance(w, losses.SegObjective) and w.weight.numel() == 9 and w.label_smoothing == 0.05
    assert train.make_seg_loss("ce", label_smoothing=0.1).label_smoothing == 0.1
    for bad in (dict(name="dice"), dict(name="ohem"), dict(name="weighted"), dict(name="focal", class_weights=[1.0] * 9),
                dict(name="normal", label_smoothing=0.1), dict(name="weighted", class_weights=[1.0, -1.0])):
        with pytest.raises(ValueError):
            train.make_seg_loss(**bad)


@pytest.mark.parametrize("argv", [["--seg-loss", "dice"], ["--seg-loss", "weighted"], ["--seg-loss", "weighted", "--seg-class-weights", "1", "2"],
                                  ["--seg-loss", "weighted", "--seg-class-weights"] + ["1"] * 8 + ["-1"],
                                  ["--seg-loss", "focal", "--seg-class-weights"] + ["1"] * 9, ["--label-smoothing", "1.0"],
                                  ["--seg-loss", "ohem", "--label-smoothing", "0.1"], ["--seg-loss", "ohem", "--ohem-thresh", "0"],
                                  ["--seg-loss", "ohem", "--ohem-n-min", "0"], ["--seg-loss", "focal", "--focal-gamma", "0"],
                                  ["--seg-loss", "ohem", "--crop-size", "64", "--ohem-n-min", "16385"]])
def test_command_line_refuses(argv, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--synthetic", "4"] + argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_command_line_help_names_the_flags(capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    for flag in ("--seg-loss {ce,ohem,focal,normal,weighted}", "--ohem-thresh", "--ohem-n-min", "--focal-gamma", "--label-smoothing",
                 "--seg-class-weights"):
        assert flag in out, flag
    assert "batch * crop^2 // 16 (this project's choice" in out
