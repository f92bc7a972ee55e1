"""Host tests of the arithmetic-mode table (segmif_amd/modes.py), of what the guard borrows from it, and of its documentation."""
import json
import os
import re
import subprocess
import sys

import pytest

from segmif_amd import modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [m.name for m in modes.TABLE]
ENTRY = {m.name: m for m in modes.TABLE}


def other(m):
    """A legal value that is not the default (a tuple entry's first such; the float entry's: another float)."""
    return next(v for v in m.values if v != m.default) if isinstance(m.values, tuple) else m.default * 1.75


def legal(m):
    return str(m.values) if isinstance(m.values, tuple) else m.values.__doc__


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEGMIF_")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra)
    return env


# The child only imports: it reports every switch, the ops getters built on them, and that neither a device nor the library was opened.
CHILD = """
import json, sys
import segmif_amd.ops as ops
from segmif_amd import modes, _lib
import torch
rec = {m.name: modes.get(m.name) for m in modes.TABLE}
rec["ops"] = {"conv3x3": ops.conv3x3_mode(), "linear": ops.linear_mode(), "crosspath": ops.crosspath_mode(),
              "crosspath_arith": ops.crosspath_arith(), "attention": ops.attention_mode(), "mixffn": ops.mixffn_mode(),
              "pairs": ops.pairs_mode(), "lazy_seg": ops.lazy_seg_mode(), "train_conv_f16": ops.train_conv_f16(),
              "guard_cond_bound": ops.Planes16Guard.COND_BOUND}
rec["opened"] = [torch.cuda.is_initialized(), _lib._lib is not None]
print(json.dumps(rec))
"""


def child(env):
    return subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def imported():
    """Three fresh processes for all the entries: every variable at its alternative value, set to '', and absent."""
    out = {}
    for case, env in (("other", {m.env: str(other(m)) for m in modes.TABLE}), ("empty", {m.env: "" for m in modes.TABLE}), ("unset", {})):
        r = child(clean_env(**env))
        assert r.returncode == 0, r.stderr
        out[case] = json.loads(r.stdout.strip().splitlines()[-1])
        assert out[case]["opened"] == [False, False]
    return out


@pytest.fixture(autouse=True)
def table_untouched():
    before = {n: modes.get(n) for n in NAMES}
    yield
    assert {n: modes.get(n) for n in NAMES} == before


@pytest.mark.parametrize("name", NAMES)
def test_get_set_and_the_context_manager(name):
    m = ENTRY[name]
    if m.env not in os.environ:
        assert modes.get(name) == m.default
    start, alt = modes.get(name), other(m)
    assert modes.set(name, alt) == start and modes.get(name) == alt
    assert modes.set(name, start) == alt and modes.get(name) == start
    for bad in ("no-such-value", None):
        with pytest.raises(ValueError) as e:
            modes.set(name, bad)
        assert name in str(e.value) and legal(m) in str(e.value) and modes.get(name) == start
    # restored when the body raises - the switches set before an illegal one too
    with pytest.raises(ZeroDivisionError):
        with modes.modes(**{name: alt}):
            assert modes.get(name) == alt
            1 / 0
    assert modes.get(name) == start
    neighbour = NAMES[(NAMES.index(name) + 1) % len(NAMES)]
    n0 = modes.get(neighbour)
    with pytest.raises(ValueError):
        with modes.modes(**{neighbour: other(ENTRY[neighbour]), name: "no-such-value"}):
            raise AssertionError("the body must not run")
    assert modes.get(neighbour) == n0 and modes.get(name) == start
    # nested, with an overlapping key
    with modes.modes(**{name: alt, neighbour: other(ENTRY[neighbour])}):
        with modes.modes(**{name: start}):
            assert modes.get(name) == start and modes.get(neighbour) == other(ENTRY[neighbour])
            with modes.modes(**{name: alt}):
                assert modes.get(name) == alt
            assert modes.get(name) == start
        assert modes.get(name) == alt and modes.get(neighbour) == other(ENTRY[neighbour])
    assert modes.get(name) == start and modes.get(neighbour) == n0


def test_unknown_switch_names_are_errors():
    with pytest.raises(KeyError):
        modes.get("no_such_switch")
    with pytest.raises(KeyError):
        with modes.modes(no_such_switch="1"):
            pass


@pytest.mark.parametrize("name", NAMES)
def test_environment_is_read_at_import(name, imported):
    m = ENTRY[name]
    assert imported["other"][name] == other(m) and imported["empty"][name] == imported["unset"][name] == m.default
    for rec, want in ((imported["other"], other(m)), (imported["empty"], m.default)):
        if name == "lazy_seg":
            assert rec["ops"][name] is (want == "1")
        elif name == "train_conv":
            assert rec["ops"]["train_conv_f16"] is (want == "f16x3" and rec["conv3x3"] != "fp32")
        elif name in rec["ops"]:
            assert rec["ops"][name] == want
    r = subprocess.run([sys.executable, "-c", "import segmif_amd.ops"], env=clean_env(**{m.env: "no-such-value"}),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith("RuntimeError") and m.env in last and legal(m) in last and "'no-such-value'" in last


def test_ops_keeps_its_getters_and_setters():
    from segmif_amd import ops
    for key, getter, setter in (("conv3x3", ops.conv3x3_mode, ops.set_conv3x3_mode), ("linear", ops.linear_mode, ops.set_linear_mode),
                                ("crosspath", ops.crosspath_mode, ops.set_crosspath_mode),
                                ("crosspath_arith", ops.crosspath_arith, ops.set_crosspath_arith),
                                ("attention", ops.attention_mode, ops.set_attention_mode), ("mixffn", ops.mixffn_mode, ops.set_mixffn_mode),
                                ("pairs", ops.pairs_mode, ops.set_pairs_mode)):
        start, alt = getter(), other(ENTRY[key])
        assert start == modes.get(key) and setter(alt) == start and getter() == alt and setter(start) == alt
        with pytest.raises(ValueError):
            setter("no-such-value")
    on = ops.lazy_seg_mode()
    assert isinstance(on, bool) and ops.set_lazy_seg_mode(0) is on and ops.lazy_seg_mode() is False
    assert ops.set_lazy_seg_mode("yes") is False and ops.lazy_seg_mode() is True and ops.set_lazy_seg_mode(on) is True
    with ops.modes(train_conv="bf16x6"):
        assert not ops.train_conv_f16() and ops.set_train_conv("f16x3") == "bf16x6"
        with ops.modes(conv3x3="planes"):
            assert ops.train_conv_f16()
        with ops.modes(conv3x3="fp32"):
            assert not ops.train_conv_f16()


def test_guard_restores_the_modes_it_borrows_when_the_repeat_raises():
    """A conditioning repeat runs with conv3x3 = 'fp32' AND crosspath = 'gemm'; a `redo` (or a whole-batch fn) that raises there
    leaves both as they were, no guard active, and the next guarded scope usable."""
    import torch
    from segmif_amd import ops
    B = 3
    G = ops.Planes16Guard
    big = (G.COND_BOUND / G.COND_EPS) ** 0.5 * 2.0  # k1 = k2 = big: estimate ~ 4 x the bound

    def bits(v):
        return int(torch.tensor([v], dtype=torch.float32).view(torch.int32))

    def producer(k):
        g = ops.active_guard()
        if g is None:
            seen.append(("fn", ops.conv3x3_mode(), ops.crosspath_mode()))
            raise KeyError("whole-batch repeat")
        g.slot(B)
        for b in range(B):
            g.amax[0, b] = bits(1.0)
            g.amax[g.SLOTS, b] = g.amax[g.SLOTS + 1, b] = bits(k[b])
        return ["f16x3"] * B

    def redo(out, idx):
        assert ops.active_guard() is None
        seen.append(("redo", ops.conv3x3_mode(), ops.crosspath_mode()))
        raise KeyError("per-image repeat")

    seen = []
    with ops.modes(conv3x3="planes16", crosspath="gram"):
        with pytest.raises(KeyError, match="per-image"):
            ops.run_guarded(lambda: producer([0.0, big, 0.0]), "cpu", enabled=True, images=B, redo=redo)
        assert (ops.conv3x3_mode(), ops.crosspath_mode()) == ("planes16", "gram") and ops.active_guard() is None
        with pytest.raises(KeyError, match="whole-batch"):
            ops.run_guarded(lambda: producer([big] * B), "cpu", enabled=True, images=B, redo=redo)
        assert (ops.conv3x3_mode(), ops.crosspath_mode()) == ("planes16", "gram") and ops.active_guard() is None
        assert seen == [("redo", "fp32", "gemm"), ("fn", "fp32", "gemm")]
        assert ops.run_guarded(lambda: producer([0.0] * B), "cpu", enabled=True, images=B, redo=redo) == ["f16x3"] * B  # (not suppressed)


def section4():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return re.search(r"^## 4\. .*?(?=^## )", text, re.S | re.M).group(0)


@pytest.mark.parametrize("name", NAMES)
def test_integration_md_documents_the_switch(name):
    m = ENTRY[name]
    rows = [r for r in section4().splitlines() if r.startswith("|") and f"`{m.env}`" in r.split("|")[1]]
    assert len(rows) == 1, (m.env, rows)
    key, values = rows[0].split("|")[1:3]
    assert f"`{name}`" in key
    default = m.default if isinstance(m.values, tuple) else "%.0e" % m.default
    assert f"`{default}` (default)".replace("e-0", "e-") in values
    for v in (m.values if isinstance(m.values, tuple) else ()):
        assert f"`{v}`" in values, (m.env, v)
    if not isinstance(m.values, tuple):
        assert m.values.__doc__ in key and "2e-3" not in section4()


def test_integration_md_names_no_unknown_variable():
    """Every SEGMIF_ variable in the section's table is in the mode table or is read by a getenv() in csrc/."""
    csrc = os.path.join(ROOT, "segmif_amd", "csrc")
    c_side = set()
    for f in os.listdir(csrc):
        c_side.update(re.findall(r'getenv\("(SEGMIF_[A-Z0-9_]+)"\)', open(os.path.join(csrc, f), errors="replace").read()))
    named = set()
    for row in section4().splitlines():
        if row.startswith("|"):
            named.update(re.findall(r"SEGMIF_[A-Z0-9_]+", row.split("|")[1]))
    assert named and named <= {m.env for m in modes.TABLE} | c_side, named - {m.env for m in modes.TABLE} - c_side


def c_side_switches():
    """{name: [source lines that read it]} for every getenv("SEGMIF_...") in csrc/."""
    csrc = os.path.join(ROOT, "segmif_amd", "csrc")
    reads = {}
    for f in sorted(os.listdir(csrc)):
        for line in open(os.path.join(csrc, f), errors="replace").read().splitlines():
            for name in re.findall(r'getenv\("(SEGMIF_[A-Z0-9_]+)"\)', line):
                reads.setdefault(name, []).append(line)
    return reads


# switches read inside the library that tests/test_gpu_kernel_variants.py need not name, each with its reason
VARIANTS_EXEMPT = {
    "SEGMIF_WG3_DBG": "compiled out unless the library is built with -DWG3_DBG=1",
}


def variants_text():
    return open(os.path.join(ROOT, "tests", "test_gpu_kernel_variants.py")).read()


def test_every_library_side_switch_has_a_variants_row_and_a_document_row():
    """A getenv("SEGMIF_X") added to csrc/ selects kernel code no in-process test can reach: it needs a row in VARIANTS of the
    kernel-variants GPU test (read as text: this test runs without a device) or an exemption with its reason, and a row in
    INTEGRATION.md section 4 either way."""
    reads = c_side_switches()
    assert len(reads) >= 8
    table = variants_text()
    table = table[table.index("def _rows():"):table.index("VARIANTS = _rows()")]
    missing = [n for n in reads if f'"{n}"' not in table and n not in VARIANTS_EXEMPT]
    assert not missing, f"no row in VARIANTS of tests/test_gpu_kernel_variants.py: {missing}"
    assert set(VARIANTS_EXEMPT) <= set(reads), "an exemption for a switch that is no longer read"
    assert not [n for n in VARIANTS_EXEMPT if f'"{n}"' in table], "exempt and in the table"
    documented = set()
    for row in section4().splitlines():
        if row.startswith("|"):
            documented.update(re.findall(r"SEGMIF_[A-Z0-9_]+", row.split("|")[1]))
    assert not set(reads) - documented - set(VARIANTS_EXEMPT), set(reads) - documented


def test_variants_rows_name_switches_and_values_the_library_reads():
    """The other direction: every switch a VARIANTS row sets is read by a getenv() in csrc/, and a value that the library
    compares as text stands on the line that reads it (strcmp(e, "direct"), e[0] == '0') - for the two switches whose effect cannot
    be seen from outside the kernel (GEMM_EPI, GEMM_PAIRS_SADDR) this is the only check of the spelling."""
    reads = c_side_switches()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import test_gpu_kernel_variants as tv
    finally:
        sys.path.remove(os.path.join(ROOT, "tests"))
    seen = set()
    for group, env, case, must, must_not in tv.VARIANTS:
        for name, value in env.items():
            assert name in reads, name
            lines = " ".join(reads[name])
            assert "atoi(e)" in lines and value.isdigit() or f'"{value}"' in lines or f"e[0] == '{value}'" in lines, (name, value)
            seen.add(name)
        assert (group is None) == (case is None)
    assert seen == set(reads) - set(VARIANTS_EXEMPT)
    for group in ("A", "B"):
        assert tv.group_env(group)  # (asserts one value per switch within a group)
    assert not set(tv.group_env("A")) & {"SEGMIF_PLANES_SUB"} and not set(tv.group_env("B")) & {"SEGMIF_PLANES_LEAN"}  # they interact
