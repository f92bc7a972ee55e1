"""CPU-only checks of the distillation objectives (csrc/distill_objective.hip behind losses.DistillObjective, segmif_amd.distill and
the train command's --distill-* flags; ABI in include/segmif_distill.h).  No kernel is launched here.

  - the header's part of what tests/test_abi_and_host.py and tests/test_abi_contract_host.py check for every header (symbols exported
    and bound, struct layouts, every row of the contract table rejected): the symbols it is expected to declare, its constants, and
    that the contract table holds every case of its EINVAL list
  - the float64 restatement tests/_distill_ref.py against F.kl_div, its zero cases, its gradient against autograd
  - parser, checks and plan of the --distill-* flags
  - the loud failures of losses.DistillObjective"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import _abi_contract_table as table
import _abi_headers as headers
import _distill_ref as ref
from test_abi_contract_host import check_rejected, records  # noqa: F401 - the fixture: the contract child's records

FWD, BWD = "segmif_distill_objective_f32", "segmif_distill_objective_bwd_f32"


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_these_symbols_and_its_source_is_built():
    from segmif_amd import build
    assert headers.declared("segmif_distill.h") == [BWD, FWD, "segmif_distill_workspace_bytes"]
    assert "distill_objective.hip" in build.SOURCES


def test_the_headers_constants(tmp_path):
    from segmif_amd._lib import DISTILL_CHANNEL, DISTILL_PIXEL
    got = headers.c_ints("segmif_distill.h", ["SEGMIF_DISTILL_PIXEL", "SEGMIF_DISTILL_CHANNEL", "SEGMIF_DISTILL_BLOCK_ROWS",
                                              "SEGMIF_DISTILL_MAX_BLOCKS_PER_SAMPLE", "SEGMIF_DISTILL_MAX_BATCH"], tmp_path)
    assert got[:2] == [DISTILL_PIXEL, DISTILL_CHANNEL] and got[2:] == [256, 64, 65535]


def test_workspace_bytes_is_positive_for_legal_sizes_and_zero_for_refused_ones(lib):
    size = lib.segmif_distill_workspace_bytes
    for mode in (0, 1):
        for rows, P, C in ((1, 1, 1), (1, 1, 9), (30, 15, 9), (3 * 391, 391, 9), (513, 513, 32), (8 * 16384, 16384, 9), (2 * 16641, 16641, 9)):
            assert size(rows, P, C, mode) > 0, (rows, P, C, mode)
        assert size(65535, 1, 9, mode) > 0
        for rows, P, C in ((0, 1, 9), (-4, 2, 9), (4, 0, 9), (4, -2, 9), (5, 2, 9), (4, 2, 0), (4, 2, 33), (4, 2, -1)):
            assert size(rows, P, C, mode) == 0, (rows, P, C, mode)
    assert size(4, 2, 9, 2) == 0 and size(4, 2, 9, -1) == 0
    assert size(65536, 1, 9, 1) == 0 and size(65536, 1, 9, 0) > 0  # the batch limit is the channel grid's
    assert size(2 ** 31 * 256, 1, 9, 0) == 0                          # and the pixel grid takes 2^31 - 1 blocks
    assert size(513, 513, 9, 0) == 3 * 8                              # pixel: one double per block of 256 rows
    table, stat = 6 * 32 * 4, 4 * 32 * 4
    assert size(2 * 513, 513, 9, 1) == 2 * (table + 3 * (8 + stat))   # channel: the table, then per block a double and its statistics
    assert size(16641, 16641, 9, 1) == table + 64 * (8 + stat)        # 66 tiles: the cap


# ---- rejections: the cases of the header's EINVAL list, each a row of tests/_abi_contract_table.py that the contract child sent -------

COMMON = [("desc", None), ("student", None), ("teacher", None), ("workspace", None), ("record4", None), ("C", 0), ("C", -1), ("C", 33),
          ("lds", 8), ("ldt", 8), ("temperature", 0.0), ("temperature", -1.0), ("temperature", math.inf), ("temperature", math.nan),
          ("mode", 2), ("mode", -1), ("rows", 0), ("rows", -512), ("rows_per_sample", 0), ("rows_per_sample", -256),
          ("rows_per_sample", 255),  # rows % rows_per_sample != 0
          ("rows", 65536 * 256)]     # B = 65536: beyond SEGMIF_DISTILL_MAX_BATCH, the grid's second dimension
MUTATIONS = {FWD: COMMON, BWD: COMMON + [("upstream", None), ("dstudent", None), ("ldd", 8)]}
CASES = [(name, arg, value) for name in (FWD, BWD) for arg, value in MUTATIONS[name]]


def test_the_cases_cover_the_headers_einval_list():
    for name in (FWD, BWD):  # every case of the header's EINVAL list is a row of each entry point
        args = {a for a, _ in MUTATIONS[name]}
        assert {"desc", "student", "teacher", "workspace", "record4", "C", "lds", "ldt", "temperature", "mode", "rows", "rows_per_sample"} <= args
    assert {"upstream", "dstudent", "ldd"} <= {a for a, _ in MUTATIONS[BWD]}


@pytest.mark.parametrize("case", CASES, ids=[f"{name}:{arg}={value}" for name, arg, value in CASES])
def test_rejected(records, case):
    check_rejected(records, table.find(*case))


# ---- the restatement, on the CPU ------------------------------------------------------------------------------------------------------------

def _pair(shape, seed=0, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64), scale * torch.randn(shape, generator=g, dtype=torch.float64))


SHAPES = [(1, 1, 1, 1), (1, 1, 1, 9), (2, 3, 5, 9), (3, 17, 23, 9), (2, 4, 3, 32)]


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_kl_div(shape, T):
    s, t = _pair(shape)
    B, h, w, C = shape
    pix = F.kl_div(F.log_softmax(s / T, dim=-1), F.softmax(t / T, dim=-1), reduction="sum") * T * T / (B * h * w)
    assert abs(float(ref.loss("pixel", s, t, T) - pix)) <= 1e-12 * max(1.0, abs(float(pix)))
    sc, tc = s.reshape(B, h * w, C) / T, t.reshape(B, h * w, C) / T
    cha = F.kl_div(F.log_softmax(sc, dim=1), F.softmax(tc, dim=1), reduction="sum") * T * T / (B * C)
    assert abs(float(ref.loss("channel", s, t, T) - cha)) <= 1e-12 * max(1.0, abs(float(cha)))
    for kind, want in (("pixel", pix), ("channel", cha)):
        assert abs(float(ref.torch_ops(kind, s, t, T) - want)) <= 1e-12 * max(1.0, abs(float(want)))
        assert float(ref.loss(kind, s, t, T)) >= -1e-15  # a KL divergence


@pytest.mark.parametrize("kind", ["pixel", "channel"])
def test_restatement_gradient_is_autograds_and_sums_to_zero_over_the_softmax_axis(kind):
    for shape in SHAPES:
        for T in (0.5, 4.0):
            s, t = _pair(shape, seed=1)
            s.requires_grad_(True)
            ref.loss(kind, s, t, T).backward()
            g = ref.grad(kind, s.detach(), t, T)
            assert float((g - s.grad).abs().max()) <= 1e-13 * max(1.0, float(s.grad.abs().max()))
            sums = g.sum(dim=-1) if kind == "pixel" else g.sum(dim=(1, 2))
            assert float(sums.abs().max()) <= 1e-14


def test_restatement_zero_cases():
    for shape in SHAPES:
        _, t = _pair(shape, seed=2)
        B, h, w, C = shape
        g = torch.Generator().manual_seed(3)
        per_row = t + torch.randn((B, h, w, 1), generator=g, dtype=torch.float64)
        per_map = t + torch.randn((B, 1, 1, C), generator=g, dtype=torch.float64)
        for kind, s in (("pixel", t.clone()), ("channel", t.clone()), ("pixel", per_row), ("channel", per_map)):
            assert abs(float(ref.loss(kind, s, t, 2.0))) <= 1e-14, (shape, kind)
            assert float(ref.grad(kind, s, t, 2.0).abs().max()) <= 1e-14, (shape, kind)
    s, t = _pair((2, 3, 5, 1), seed=4)   # C = 1 in pixel mode: one class, nothing to distil
    assert float(ref.loss("pixel", s, t, 1.0)) == 0.0 and float(ref.grad("pixel", s, t, 1.0).abs().max()) == 0.0
    s, t = _pair((3, 1, 1, 9), seed=5)   # P = 1 in channel mode: one position
    assert float(ref.loss("channel", s, t, 4.0)) == 0.0 and float(ref.grad("channel", s, t, 4.0).abs().max()) == 0.0


# ---- parser and plan ----------------------------------------------------------------------------------------------------------------------

BASE = ["--synthetic", "8", "--rounds", "1", "--fusion-iters", "2", "--seg-iters", "2", "--backbone", "mit_b1", "--crop-size", "64",
        "--synthetic-size", "96", "128", "--samples-per-gpu", "4", "--out", "somewhere"]


def _checked(argv):
    from segmif_amd import train
    ap = train.build_parser()
    args = ap.parse_args(argv)
    train.check_args(args, ap.error)
    train.resolve_defaults(args)
    return args


def _refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _checked(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_parser_refusals(tmp_path, capsys):
    ckpt = tmp_path / "teacher.pth"
    ckpt.write_bytes(b"not read by the parser")
    on = ["--distill-from", str(ckpt), "--distill-backbone", "mit_b2"]
    for flag, value in (("--distill-backbone", "mit_b2"), ("--distill-kind", "pixel"), ("--distill-temperature", "2"), ("--distill-weight", "1")):
        assert f"{flag} belongs to --distill-from, which is not given" in _refused(BASE + [flag, value], capsys)
    assert "--distill-from needs --distill-backbone" in _refused(BASE + ["--distill-from", str(ckpt)], capsys)
    assert "--distill-backbone mit_b0" in _refused(BASE + ["--distill-from", str(ckpt), "--distill-backbone", "mit_b0"], capsys)
    assert "--distill-backbone resnet" in _refused(BASE + ["--distill-from", str(ckpt), "--distill-backbone", "resnet"], capsys)
    for bad in ("0", "-1", "inf", "nan"):
        assert f"--distill-temperature {float(bad)}: must be a finite number > 0" in _refused(BASE + on + ["--distill-temperature", bad], capsys)
        assert f"--distill-weight {float(bad)}: must be a finite number > 0" in _refused(BASE + on + ["--distill-weight", bad], capsys)
    assert "invalid choice" in _refused(BASE + on + ["--distill-kind", "feature"], capsys)
    err = _refused(BASE + on + ["--ema-decay", "0.9", "--self-training"], capsys)
    assert "--distill-from with --self-training" in err and "not built" in err
    missing = str(tmp_path / "nowhere.pth")
    assert f"--distill-from {missing}: no such file" in _refused(BASE + ["--distill-from", missing, "--distill-backbone", "mit_b2"], capsys)


def test_plan_with_and_without_distillation(tmp_path):
    from segmif_amd import train
    ckpt = tmp_path / "teacher.pth"
    ckpt.write_bytes(b"not read by the plan")
    off = train.make_plan(_checked(BASE))
    assert sorted(vars(off)) == sorted(["batch", "guarded", "ema_seg", "ema_fus", "rcs_kw", "rcs_phases", "mix_kw", "mix_phases", "st_kw",
                                        "st_mix_kw", "fusion_opt_kw", "seg_opt_kw", "loader_kw", "fusion_iters", "seg_iters", "say"])
    assert getattr(off, "distill_kw", None) is None and not any("distill" in line for line in off.say)
    on = train.make_plan(_checked(BASE + ["--distill-from", str(ckpt), "--distill-backbone", "mit_b3"]))
    assert on.distill_kw == dict(path=str(ckpt), backbone="mit_b3", kind="channel", temperature=4.0, weight=3.0)
    assert sorted(set(vars(on)) - set(vars(off))) == ["distill_kw"]
    assert {k: v for k, v in vars(on).items() if k not in ("say", "distill_kw")} == {k: v for k, v in vars(off).items() if k != "say"}
    said = [line for line in on.say if "distill" in line]
    assert len(said) == 1 and [line for line in on.say if "distill" not in line] == off.say
    assert said[0].startswith(f"[train] --distill-from {ckpt} (backbone mit_b3, kind channel, temperature 4.0, weight 3.0): this project's "
                              "addition, NOT the reference's training")
    assert "mIoU" in said[0] and "\n" not in said[0]
    pix = train.make_plan(_checked(BASE + ["--distill-from", str(ckpt), "--distill-backbone", "mit_b2", "--distill-kind", "pixel"]))
    assert pix.distill_kw["temperature"] == 1.0 and pix.distill_kw["kind"] == "pixel"
    both = train.make_plan(_checked(BASE + ["--distill-from", str(ckpt), "--distill-backbone", "mit_b2", "--distill-kind", "pixel",
                                            "--distill-temperature", "2.5", "--distill-weight", "0.5"]))
    assert (both.distill_kw["temperature"], both.distill_kw["weight"]) == (2.5, 0.5)
    helps = {a.option_strings[0]: a.help for a in train.build_parser()._actions if a.option_strings}
    assert "NOT the reference's training" in helps["--distill-from"] and "mIoU" in helps["--distill-from"]


# ---- loud failures of the Python layers -------------------------------------------------------------------------------------------------------

def test_distill_objective_fails_loudly():
    from segmif_amd import losses
    with pytest.raises(ValueError, match="kind must be one of channel, pixel"):
        losses.DistillObjective("feature")
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="temperature must be finite and > 0"):
            losses.DistillObjective("pixel", bad)
    assert losses.DistillObjective("channel").temperature == 4.0 and losses.DistillObjective("pixel").temperature == 1.0
    assert losses.DistillObjective("pixel", 2).temperature == 2.0
    obj = losses.DistillObjective()
    s, t = torch.zeros(2, 3, 5, 9), torch.zeros(2, 3, 5, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obj.forward_nhwc(s, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obj(s.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match=r"\(2, 3, 5, 9\).*\(2, 3, 4, 9\)"):
        obj.forward_nhwc(s, torch.zeros(2, 3, 4, 9))
    with pytest.raises(RuntimeError, match=r"\(2, 9, 3, 5\).*\(2, 9, 3, 4\)"):
        obj(torch.zeros(2, 9, 3, 5), torch.zeros(2, 9, 3, 4))
    with pytest.raises(RuntimeError, match="teacher logits require grad"):
        obj.forward_nhwc(s, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="teacher logits require grad"):
        obj(s.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2).clone().requires_grad_(True))


def test_distill_step_and_teacher_fail_loudly():
    from segmif_amd import distill, losses
    with pytest.raises(TypeError, match="Network3"):
        distill.FrozenTeacher(torch.nn.Linear(2, 2))

    class Net(torch.nn.Linear):
        def _segment_nhwc(self, x):
            return x

    net = Net(2, 2).train()
    teacher = distill.FrozenTeacher(net)
    assert not net.training and not any(p.requires_grad for p in net.parameters())
    obj = losses.DistillObjective()
    for bad in (0.0, -3.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="weight must be finite and > 0"):
            distill.DistillStep(None, teacher, None, None, obj, weight=bad)
    with pytest.raises(TypeError, match="FrozenTeacher"):
        distill.DistillStep(None, net, None, None, obj)
    with pytest.raises(TypeError, match="DistillObjective"):
        distill.DistillStep(None, teacher, None, None, torch.nn.CrossEntropyLoss())
    assert distill.DistillStep(None, teacher, None, None, obj).weight == 3.0
