"""CPU-only checks of multi-scale + flip inference: the view plan, its argument errors, the command line's flags and the
C signatures of the two new entry points against their ctypes bindings.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


DEFAULT_VIEWS = [(240, 320), (360, 480), (480, 640), (600, 800), (720, 960), (840, 1120)]


def test_default_plan_is_the_segformer_protocol():
    from segmif_amd.tta import TTA, tta_plan
    t = TTA()
    assert t.scales == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75) and t.flip is True and t.size_divisor == 8
    want = [(h, w, f) for h, w in DEFAULT_VIEWS for f in (False, True)]
    assert tta_plan(480, 640, t.scales, t.flip, t.size_divisor) == want
    assert t.plan(480, 640) == want and len(want) == 12
    assert tta_plan(480, 640, t.scales, False) == [(h, w, False) for h, w in DEFAULT_VIEWS]
    with pytest.raises(Exception):  # frozen
        t.flip = False
    d = t.describe(480, 640)
    assert d == {"scales": list(t.scales), "flip": True, "size_divisor": 8, "views": [[h, w, f] for h, w, f in want]}


def test_plan_rounds_half_up_and_then_up_to_the_divisor():
    from segmif_amd.tta import tta_plan
    assert tta_plan(64, 96, (0.7,), False) == [(48, 72, False)]
    assert tta_plan(64, 96, (0.7,), False, 1) == [(45, 67, False)]
    assert tta_plan(64, 96, (1.5, 0.75), True) == [(96, 144, False), (96, 144, True), (48, 72, False), (48, 72, True)]  # given order


@pytest.mark.parametrize("scales,flip,div", [((), True, 8), ((1.0, 0.0), False, 8), ((-0.5,), False, 8), ((float("nan"),), False, 8),
                                             ((1.0,), False, 0), ((1.0,), True, -8), (tuple(1.0 + 0.1 * i for i in range(9)), True, 8),
                                             (tuple(1.0 + 0.01 * i for i in range(17)), False, 8)])
def test_plan_rejects(scales, flip, div):
    from segmif_amd.tta import tta_plan
    with pytest.raises(ValueError):
        tta_plan(64, 96, scales, flip, div)


def test_sixteen_views_are_admitted():
    from segmif_amd.tta import tta_plan
    assert len(tta_plan(64, 96, tuple(1.0 + 0.1 * i for i in range(8)), True)) == 16


REQUIRED = ["--ir", "a", "--vis", "b", "--mask", "c", "--out", "d"]


def test_command_line_flags():
    from segmif_amd.evaluate import parse_args
    from segmif_amd.tta import TTA
    assert parse_args(REQUIRED)[1] is None  # without the flags: the single view, as before
    assert parse_args(REQUIRED + ["--flip"])[1] == TTA((1.0,), True, 8)
    assert parse_args(REQUIRED + ["--ms-scales", "0.5", "1", "1.5"])[1] == TTA((0.5, 1.0, 1.5), False, 8)
    assert parse_args(REQUIRED + ["--ms-scales", "0.75", "1.0", "--flip", "--size-divisor", "32"])[1] == TTA((0.75, 1.0), True, 32)
    assert parse_args(REQUIRED + ["--size-divisor", "4"])[1] is None  # (a divisor alone asks for nothing)


@pytest.mark.parametrize("extra", [["--ms-scales", "0"], ["--ms-scales", "1.0", "-0.5"], ["--ms-scales", "big"], ["--ms-scales"],
                                   ["--flip", "--size-divisor", "0"], ["--flip", "--ms-scales"] + [str(1 + 0.1 * i) for i in range(9)]])
def test_command_line_rejects(extra, capsys):
    from segmif_amd.evaluate import parse_args
    with pytest.raises(SystemExit) as e:
        parse_args(REQUIRED + extra)
    assert e.value.code == 2
    capsys.readouterr()


# C parameter type -> ctypes type, as segmif_amd/_lib.py binds them (every device or host pointer but a struct's is a void*)
def _ctype(decl, structs):
    decl = decl.strip()
    base = re.sub(r"\s+\w+$", "", decl) if not decl.endswith("*") else decl  # drop the parameter's name
    base = base.replace("const ", "").strip()
    if base.endswith("*"):
        pointee = base[:-1].strip()
        return ctypes.POINTER(structs[pointee]) if pointee in structs else ctypes.c_void_p
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[base]


def _declaration(text, name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in segmif_hip.h"
    return m.group(1), [p for p in m.group(2).split(",")]


@pytest.mark.parametrize("name", ["segmif_tta_vote_f32", "segmif_resize_flip_nchw_f32"])
def test_new_signatures_match_the_header(name):
    from segmif_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "segmif_hip.h")).read(), flags=re.S)
    ret, params = _declaration(text, name)
    structs = {"SegmifTtaView": _lib.SegmifTtaView}
    res, args = _lib.SIGNATURES[name]
    assert ret == "int" and res is ctypes.c_int
    assert [_ctype(p, structs) for p in params] == list(args), (params, args)


def test_entry_points_reject_what_the_header_excludes(lib):
    """The argument checks run before any launch, so they can be exercised without a device (pointers are never followed)."""
    from segmif_amd import _lib
    EINVAL = -22
    fake = 4096  # (a non-null address; rejected calls return before anything reads it)

    def vote(n, C, ldx, ih=4, labels=fake, x=fake, B=1, OH=8):
        tab = (_lib.SegmifTtaView * 17)()
        for v in tab:
            v.x, v.ih, v.iw, v.ldx, v.flip = x, ih, 4, ldx, 0
        return lib.segmif_tta_vote_f32(tab, n, labels, None, B, OH, 8, C, None)

    for kw in (dict(n=0, C=9, ldx=9), dict(n=17, C=9, ldx=9), dict(n=1, C=0, ldx=9), dict(n=1, C=33, ldx=33),
               dict(n=2, C=9, ldx=8), dict(n=1, C=9, ldx=9, ih=0), dict(n=1, C=9, ldx=9, labels=None),
               dict(n=1, C=9, ldx=9, x=None), dict(n=1, C=9, ldx=9, B=0), dict(n=1, C=9, ldx=9, OH=65536)):
        assert vote(**kw) == EINVAL, kw
    assert lib.segmif_tta_vote_f32(None, 1, fake, None, 1, 8, 8, 9, None) == EINVAL
    for args in ((None, fake, 3, 4, 4, 8, 8, 0), (fake, None, 3, 4, 4, 8, 8, 0), (fake, fake, 0, 4, 4, 8, 8, 0),
                 (fake, fake, 3, 0, 4, 8, 8, 0), (fake, fake, 3, 4, 4, 8, 0, 1), (fake, fake, 65536, 4, 4, 8, 8, 0)):
        assert lib.segmif_resize_flip_nchw_f32(*args, None) == EINVAL, args
