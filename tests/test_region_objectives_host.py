"""CPU-only checks of the region objectives (csrc/region_objective.hip behind losses.RegionObjective and losses.SegLossSum):
  * the float64 restatement the GPU tests hold the kernels against (tests/_region_objective_ref.py) is pinned without third-party
    code: on one-hot "probabilities" the Lovasz extension coincides with the set function, so its value is mean_c (1 - IoU_c) of
    the hard prediction; Dice equals a direct loop over the classes; the Lovasz value does not depend on the order of the rows nor
    on the order of ties;
  * settings, the command line and the C entry points refuse what they should; SegmifRegionObjective has gcc's layout;
  * CPU tensors raise RuntimeError (there is no torch formulation in the package).
No kernel is launched here."""
import ctypes
import os

import pytest
import torch

import _abi_headers as headers
import _region_objective_ref as ref

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_lovasz_on_one_hot_predictions_is_one_minus_iou():
    g = torch.Generator().manual_seed(0)
    n, C = 600, 5
    y = torch.randint(0, C - 1, (n,), generator=g)  # class 4 has no pixel ...
    pred = torch.randint(0, C, (n,), generator=g)   # ... but is predicted
    pred[:200] = y[:200]
    y[torch.rand(n, generator=g) < 0.1] = 255
    x = torch.full((n, C), -40.0, dtype=torch.float64)
    x[torch.arange(n), pred] = 40.0
    v = y != 255
    ious = {c: float(((pred == c) & (y == c) & v).sum()) / float((((pred == c) | (y == c)) & v).sum()) for c in range(C)}
    present = [c for c in range(C) if bool((y == c).any())]
    assert present == [0, 1, 2, 3]
    want = sum(1.0 - ious[c] for c in present) / len(present)
    assert abs(float(ref.lovasz(x, y)) - want) <= 1e-12
    want_all = sum(1.0 - ious[c] for c in range(C)) / C  # IoU of the absent, predicted class is 0: its term is max p = 1
    assert abs(float(ref.lovasz(x, y, classes="all")) - want_all) <= 1e-12


def test_dice_is_the_loop_over_classes():
    x = torch.tensor([[2.0, 0.5, -1.0], [0.0, 1.0, 0.0], [-0.5, 0.2, 3.0], [1.0, 1.0, 1.0], [0.3, -2.0, 0.1]], dtype=torch.float64)
    y = torch.tensor([0, 1, 0, 255, 1])
    p = torch.softmax(x, 1)
    for smooth in (1.0, 0.0, 0.25):
        terms = {}
        for c in range(3):
            I = sum(float(p[i, c]) for i in range(5) if int(y[i]) == c)
            S = sum(float(p[i, c]) for i in range(5) if int(y[i]) != 255)
            G = sum(1 for i in range(5) if int(y[i]) == c)
            terms[c] = (1.0 - (2 * I + smooth) / (S + G + smooth), G)
        present = [t for t, G in terms.values() if G > 0]
        assert len(present) == 2
        assert abs(float(ref.dice(x, y, smooth=smooth)) - sum(present) / 2) <= 1e-14
        assert abs(float(ref.dice(x, y, classes="all", smooth=smooth)) - sum(t for t, _ in terms.values()) / 3) <= 1e-14


def test_lovasz_value_ignores_row_and_tie_order():
    x, y = ref.make_inputs(1, (2, 12, 20), 6)
    x, y = x.double().view(-1, 6).repeat(2, 1), y.view(-1).repeat(2)  # every row twice: ties
    want = float(ref.lovasz(x, y))
    perm = torch.randperm(len(y), generator=torch.Generator().manual_seed(2))
    assert abs(float(ref.lovasz(x[perm], y[perm])) - want) <= 1e-13
    assert abs(float(ref.lovasz(x, y, order=ref._ties_descending)) - want) <= 1e-13
    # ... while the gradient does depend on the order of ties: what the rule "ascending row index" is there for
    _, g0 = ref.value_and_grad(x, y, "lovasz")
    _, g1 = ref.value_and_grad(x, y, "lovasz", order=ref._ties_descending)
    assert float((g0 - g1).abs().max()) > 1e-4 * float(g0.abs().max())


def test_nothing_valid_is_zero():
    x, y = torch.randn(7, 4, dtype=torch.float64), torch.full((7,), 255)
    for kind in ("lovasz", "dice"):
        for classes in ("present", "all"):
            v, g = ref.value_and_grad(x, y, kind, classes=classes)
            assert float(v) == 0.0 and float(g.abs().max()) == 0.0


# ---- settings ----------------------------------------------------------------------------------------------------------------------------
def test_module_settings_are_validated():
    import segmif_amd.core as core
    from segmif_amd.losses import RegionObjective, SegLossSum, SegObjective
    for kw in (dict(kind="jaccard"), dict(kind="hinge"), dict(classes="some"), dict(classes=[0, 1]), dict(smooth=-0.5),
               dict(smooth=float("nan")), dict(smooth=float("inf"))):
        with pytest.raises(ValueError):
            RegionObjective(**kw)
    m = RegionObjective()
    assert (m.kind, m.classes, m.ignore_index, m.smooth) == ("lovasz", "present", 255, 1.0) and not list(m.parameters())
    assert RegionObjective("dice", "all", 7, 0.0).smooth == 0.0
    ce = torch.nn.CrossEntropyLoss(ignore_index=255)
    for w in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SegLossSum(ce, m, w)
    for base in (torch.nn.CrossEntropyLoss(weight=torch.ones(9)), torch.nn.CrossEntropyLoss(reduction="sum"),
                 torch.nn.CrossEntropyLoss(label_smoothing=0.1)):
        with pytest.raises(ValueError):
            SegLossSum(base, m)
    for base, region in ((torch.nn.NLLLoss(), m), (m, m), (ce, ce), (ce, SegObjective())):
        with pytest.raises(TypeError):
            SegLossSum(base, region)
    for base in (ce, SegObjective(gamma=2.0), core.OhemCELoss(0.7, 16)):
        s = SegLossSum(base, m, 0.5)
        assert s.base is base and s.region is m and s.region_weight == 0.5


def test_make_seg_region():
    from segmif_amd import losses, train
    assert train.SEG_REGIONS == ("lovasz", "dice") and train.seg_loss_names() == ["ce", "ohem", "focal", "normal", "weighted"]
    s = train.make_seg_region(train.make_seg_loss("ce"), "lovasz")
    assert isinstance(s, losses.SegLossSum) and type(s.base) is torch.nn.CrossEntropyLoss and s.region_weight == 1.0
    assert (s.region.kind, s.region.classes, s.region.ignore_index) == ("lovasz", "present", 255)
    s = train.make_seg_region(train.make_seg_loss("focal"), "dice", 0.25, "all", 0.5)
    assert (s.region.kind, s.region.classes, s.region.smooth, s.region_weight) == ("dice", "all", 0.5, 0.25)
    for bad in (dict(kind="jaccard"), dict(kind="lovasz", smooth=0.5), dict(kind="dice", weight=0.0), dict(kind="dice", classes="some"),
                dict(kind="dice", smooth=-1.0)):
        with pytest.raises(ValueError):
            train.make_seg_region(train.make_seg_loss("ce"), **bad)


# ---- the command line --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [["--seg-region", "jaccard"], ["--seg-region-weight", "0.5"], ["--seg-region-classes", "all"],
                                  ["--dice-smooth", "1.0"], ["--seg-region", "lovasz", "--dice-smooth", "1.0"],
                                  ["--seg-region", "lovasz", "--seg-region-weight", "0"],
                                  ["--seg-region", "dice", "--seg-region-weight", "-1"], ["--seg-region", "dice", "--seg-region-weight", "nan"],
                                  ["--seg-region", "dice", "--dice-smooth", "-0.1"], ["--seg-region", "dice", "--seg-region-classes", "some"],
                                  ["--seg-loss", "dice"], ["--seg-loss", "lovasz"]])
def test_command_line_refuses(argv, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--synthetic", "4"] + argv)
    assert e.value.code == 2
    assert "error:" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--seg-region", "lovasz"], ["--seg-region", "dice", "--dice-smooth", "0", "--seg-region-weight", "0.5"],
                                  ["--seg-loss", "ohem", "--seg-region", "lovasz", "--seg-region-classes", "all"]])
def test_command_line_accepts(argv, monkeypatch):
    """the arguments pass every check of the parser: the command gets as far as asking for the device (made absent here)"""
    from segmif_amd import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="MI355X"):
        train.main(["--synthetic", "4"] + argv)


def test_command_line_help_names_the_flags(capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    for flag in ("--seg-loss {ce,ohem,focal,normal,weighted}", "--seg-region {lovasz,dice}", "--seg-region-weight W",
                 "--seg-region-classes {present,all}", "--dice-smooth S", "NOT the reference's objective"):
        assert flag in out, flag


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_c(lib, tmp_path):
    """the header's enum values against autograd's (the struct's layout: tests/test_abi_and_host.py::test_struct_layouts_match_c)"""
    from segmif_amd import autograd as ag
    got = headers.c_ints("segmif_hip.h", ["SEGMIF_REGION_LOVASZ", "SEGMIF_REGION_DICE", "SEGMIF_REGION_PRESENT", "SEGMIF_REGION_ALL"], tmp_path)
    assert got == [0, 1, 0, 1]
    assert ag._REGION_KINDS == {"lovasz": 0, "dice": 1} and ag._REGION_CLASSES == {"present": 0, "all": 1}


def test_bad_calls_are_refused_without_a_gpu(lib):
    """every refusal precedes the launch: with these arguments a launch would fail differently (there is no device here)"""
    from segmif_amd import autograd as ag
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ROWS = 100

    def fwd(d, C=9, ld=9, rows=ROWS, ws=p):
        return lib.segmif_region_objective_f32(ctypes.byref(d), p, p, ws, p, rows, C, ld, None)

    def bwd(d, C=9, ld=9, ldd=9, rows=ROWS, ws=p):
        return lib.segmif_region_objective_bwd_f32(ctypes.byref(d), p, p, ws, p, p, p, rows, C, ld, ldd, None)

    def refused(d, **kw):
        return fwd(d, **kw) == EINVAL and bwd(d, **kw) == EINVAL

    good = lambda **kw: ag.region_objective_descriptor(**kw)
    size = lib.segmif_region_objective_workspace_bytes
    for C in (0, -1, 33):
        assert refused(good(), C=C, ld=40) and size(ROWS, C, 0) == 0 and size(ROWS, C, 1) == 0
    for rows in (0, -5, (2 ** 31 - 1) // 9 + 1, 2 ** 40):
        assert refused(good(), rows=rows) and size(rows, 9, 0) == 0 and size(rows, 9, 1) == 0
    assert size((2 ** 31 - 1) // 9, 9, 0) > 0 and size(2 ** 31 - 1, 1, 1) > 0  # the largest geometries that fit
    assert refused(good(), ld=8) and bwd(good(), ldd=8) == EINVAL
    for kind in (-1, 2, 9):
        d = good()
        d.kind = kind
        assert refused(d) and size(ROWS, 9, kind) == 0
    for classes in (-1, 2):
        d = good()
        d.classes = classes
        assert refused(d)
    for smooth in (-0.5, float("nan"), float("inf")):
        assert refused(good(kind="dice", smooth=smooth))
    assert refused(good(), ws=None) and refused(good(), ws=p + 4)
    assert lib.segmif_region_objective_f32(None, p, p, p, p, ROWS, 9, 9, None) == EINVAL
    # Dice: a header and three doubles per class and block of 256 rows; Lovasz: two 8-byte pairs per row and class, and more
    assert size(5883, 9, 1) - size(5883 - 256, 9, 1) == 9 * 3 * 8
    assert 2 * 8 * 9 * 5883 < size(5883, 9, 0) < 2.2 * 8 * 9 * 5883
    assert size(5883, 9, 0) % 8 == 0


def test_cpu_tensors_raise():
    from segmif_amd import autograd as ag, losses
    x, y = torch.randn(1, 9, 4, 5), torch.zeros(1, 4, 5, dtype=torch.long)
    region = losses.RegionObjective("dice")
    for m in (losses.RegionObjective(), region, losses.SegLossSum(torch.nn.CrossEntropyLoss(ignore_index=255), region),
              losses.SegLossSum(losses.SegObjective(gamma=2.0), region)):
        with pytest.raises(RuntimeError, match="MI355X"):
            m(x, y)
        with pytest.raises(RuntimeError, match="MI355X"):
            m.forward_nhwc(x.permute(0, 2, 3, 1), y)
    with pytest.raises(RuntimeError):
        ag.region_objective(x.permute(0, 2, 3, 1).double(), y)
    with pytest.raises(ValueError):
        ag.region_objective(x.permute(0, 2, 3, 1), y, kind="jaccard")
