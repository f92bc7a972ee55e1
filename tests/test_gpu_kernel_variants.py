"""GPU tests of the kernel variants that only a switch read INSIDE the library selects (the getenv("SEGMIF_...") reads of
csrc/, each taken once per process through a function-local static): no in-process test can reach them, so every group of
switches runs in a fresh child process (tests/_variants_child.py, started with subprocess.run, never exec).

The child computes each case through the public entry point, against the fp64 CPU reference and at the bound of the
existing test of the default variant (helpers and constants are imported from those test modules, no tolerance is new),
runs the weight-gradient and GEMM cases twice (the sources promise bitwise reproducible results) and writes one JSON record
per case; the tests below are parametrized over VARIANTS and only read the records.

Proof that the variant ran: the children run with the HIP runtime's logging at level 3, where it prints one
"ShaderName : <demangled kernel name>" line per launch; the child brackets each case with marker lines on stderr.  A row's `must`
substring has to occur between its markers and its `must_not` (the default variant's) must not; the same check applied to
the log of a child without any switch (group D) has to FAIL for every such row - a switch that is misspelt here or no
longer read by the library would otherwise pass every numeric check on the (equally correct) default kernels.

Two switches do not change the kernel's NAME and, by construction, not a bit of the result either: SEGMIF_GEMM_EPI=direct
(GemmSplitK::epi, a uniform branch between two store routes of the same registers) and SEGMIF_GEMM_PAIRS_SADDR=0
(GemmPairsK::saddr, two address forms of the same LDS-DMA).  Their rows carry must_not = None: the numeric bound and the
launch of the kernel are asserted, the branch taken is not observable from outside the kernel; tests/test_modes_host.py
holds the spelling of their names and values against the getenv lines of csrc/ instead."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_variants_child.py")

WGRAD_CASES = {  # B, H, W, Cin, N, k, stride, pad, dil, act - rows of CONV_CASES in test_gpu_backward.py
    "d2_relu": (2, 20, 28, 64, 32, 3, 1, 2, 2, 1), "d2_odd": (1, 19, 45, 96, 64, 3, 1, 2, 2, 0),
    "d1_ragged": (2, 23, 37, 64, 32, 3, 1, 1, 1, 2), "d1_prelu": (1, 14, 18, 128, 64, 3, 1, 1, 1, 2),
}
HALO = "wgrad3x3_halo_kernel<%d, true>"     # <DIL, VEC = true>: exact fp32, vector loads
SPLIT1 = "wgrad3x3_split_kernel("           # one team, 8 x 32 tiles, dilation 2 only
SPLIT2 = "wgrad3x3_split2_kernel<%d, %s>"   # <DIL, F16>: the default (two teams, 4 x 32 tiles)
PLANES = "conv3x3_planes_kernel<%d, %s, true, %d, %s>"  # <DIL, FUSE, F16 = true, SUB, LEAN>
XT = "dwconv3x3_xt_kernel<%s, %d, false>"   # <GELU, XT, PAIRS = false>
ONECOL = "dwconv3x3_gelu_kernel<%s>"        # <GELU>: one column per thread
B_ = ("false", "true")                      # (the runtime logs demangled names)


def _rows():
    """(group, child environment, case id, must, must_not).  group None: a switch that needs no child (see the row)."""
    rows = []
    for name, c in WGRAD_CASES.items():
        for tc in ("f16x3", "bf16x6"):
            dil, f16 = c[8], B_[tc == "f16x3"]
            # fp32 wins over the split arithmetic in both training modes (split_f16 set or not)
            rows.append(("A", {"SEGMIF_WGRAD3X3": "fp32"}, f"wgrad-{name}-{tc}", HALO % dil, "wgrad3x3_split"))
            if dil == 2:
                rows.append(("B", {"SEGMIF_WGRAD3X3": "split1"}, f"wgrad-{name}-{tc}", SPLIT1, "wgrad3x3_split2"))
            else:  # split1 exists for dilation 2 only: at dilation 1 it launches the two-team kernel, as the default does
                rows.append(("B", {"SEGMIF_WGRAD3X3": "split1"}, f"wgrad-{name}-{tc}", SPLIT2 % (1, f16), None))
    for case in ("gemm_split-bf16x6-4099x320x320", "gemm_split-bf16x6-2048x160x64", "gemm_split-f16x3-4099x320x320",
                 "gemm_split-f16x3-2048x160x64", "gemm_split-patch-4x60x81x64-128-k3s2p1"):
        rows.append(("A", {"SEGMIF_GEMM_EPI": "direct"}, case, "gemm_split_kernel", None))
    # (patch mode never takes the SADDR form: its row shows the switch leaves that mode alone)
    for case in ("gemm_pairs-777x1280x320-t0", "gemm_pairs-5000x320x320-t128", "gemm_pairs-5000x320x320-t256",
                 "gemm_pairs-patch-2x16x24x64-128-k3s1p1"):
        rows.append(("A", {"SEGMIF_GEMM_PAIRS_SADDR": "0"}, case, "gemm_pairs_kernel", None))
    for shape in ("2x9x13x128", "1x17x5x64", "1x30x41x128"):
        w = int(shape.split("x")[2])
        for gelu in (1, 0):
            case = f"dwconv-{'gelu' if gelu else 'bias'}-{shape}"
            default = (XT % (B_[gelu], 2)) if w >= 16 else (ONECOL % B_[gelu])
            rows.append(("A", {"SEGMIF_DWCONV_XT": "4"}, case, XT % (B_[gelu], 4), default))
            # (XT = 1 at W < 16 is what the default launches too: the row then only asserts the kernel)
            rows.append(("B", {"SEGMIF_DWCONV_XT": "1"}, case, ONECOL % B_[gelu], default if w >= 16 else None))
    for case, dil in (("planes-2x32x40x64-d2", 2), ("planes-1x48x33x96-d1", 1)):
        rows.append(("A", {"SEGMIF_PLANES_LEAN": "0"}, case, PLANES % (dil, "false", 4, "false"), PLANES % (dil, "false", 4, "true")))
        rows.append(("B", {"SEGMIF_PLANES_SUB": "2"}, case, PLANES % (dil, "false", 2, "false"), "true, 4, "))
    rows.append(("A", {"SEGMIF_PLANES_LEAN": "0"}, "planes-fused_tail-2x24x70x192", PLANES % (2, "true", 2, "false"), PLANES % (2, "true", 2, "true")))
    # covered in process through the `tile` argument of test_gemm_pairs_vs_fp64 (d->tile_rows takes the same branch)
    rows.append((None, {"SEGMIF_GEMM_PAIRS_MT": "128"}, None, None, None))
    return rows


VARIANTS = _rows()
GROUPS = ("A", "B", "D")  # D: no switch set, every case of A and B - the log the dispatch check must reject
RUN_ROWS = [r for r in VARIANTS if r[0] is not None]
IDS = [f"{r[0]}-{r[2]}" for r in RUN_ROWS]
BEGIN, END = "@@variant-case-begin ", "@@variant-case-end "
NOT_STARTED = "not started: an earlier child faulted"


def group_env(group):
    env = {}
    for g, e, *_ in VARIANTS:
        if g == group:
            assert all(env.get(k, v) == v for k, v in e.items()), (group, e)  # one value per switch and group
            env.update(e)
    return env


def group_cases(group):
    seen = []
    for g, _, case, *_ in RUN_ROWS:
        if (g == group or group == "D") and case not in seen:
            seen.append(case)
    return seen


def launches(log, case):
    """The kernel names the runtime logged between the case's markers (None: the markers are not there)."""
    names, inside = None, False
    for line in log.splitlines():
        if BEGIN in line and line.split(BEGIN, 1)[1].strip() == case:  # (`in`: another thread's log line may share the row)
            names, inside = [], True
        elif END in line and line.split(END, 1)[1].strip() == case:
            inside = False
        elif inside and "ShaderName : " in line:
            names.append(line.split("ShaderName : ", 1)[1].strip())
    return names


def dispatched(log, case, must, must_not):
    names = launches(log, case)
    assert names, f"{case}: the runtime logged no kernel launch between the markers"
    return any(must in n for n in names) and not (must_not and any(must_not in n for n in names))


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Each group's child once, in the order A, B, D.  Measured on an MI355X with torch's files already read by the parent: 3.7 s
    (A, 26 cases), 3.2 s (B, 16) and 3.4 s (D, 26) of wall time each, of which the cases are 1.0 .. 1.5 s and the rest is process
    start (torch import, library load, first launch).  The limit of 120 s is not sized by the cases but by a cold start: the
    first import of torch on a machine that has not run it can take a minute or more.  A child that dies (a signal, an abort,
    the time limit, a HIP error raised in a case) fails its group's tests with its output and keeps the later groups from
    starting; nothing is retried."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import build, _lib
    build.build()  # (a no-op when the library is current) - no child compiles
    _lib.load()
    tmp = tmp_path_factory.mktemp("variants")
    out, dead = {}, None
    for group in GROUPS:
        if dead is not None:
            out[group] = {"error": f"{NOT_STARTED} (group {dead})"}
            continue
        env = {k: v for k, v in os.environ.items() if not k.startswith("SEGMIF_") or k == "SEGMIF_HIP_LIB"}
        env.update(group_env(group) if group != "D" else {})
        env.update(AMD_LOG_LEVEL="3", PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
        rec_path, log_path = str(tmp / f"{group}.json"), str(tmp / f"{group}.log")
        cmd = ["timeout", "-k", "10", "120", sys.executable, CHILD, group, rec_path]
        t0 = time.time()
        try:
            with open(log_path, "w") as log:
                r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=log, text=True, timeout=150)
            code, stdout = r.returncode, r.stdout
        except subprocess.TimeoutExpired as e:
            code, stdout = 124, str(e)
        log = open(log_path, errors="replace").read()
        records = {r["case"]: r for r in json.load(open(rec_path))} if os.path.exists(rec_path) else {}
        out[group] = {"records": records, "log": log, "seconds": round(time.time() - t0, 1)}
        if code != 0:  # (the child itself exits 0 when a case merely misses its bound: that is the case's own failure)
            tail = "\n".join(l for l in log.splitlines() if "ShaderName" not in l and ":3:" not in l)[-4000:]
            out[group]["error"] = f"the child of group {group} ended with status {code}\n{stdout[-2000:]}\n{tail}"
            dead = group
    return out


def _group(children, group):
    g = children[group]
    assert "error" not in g, g["error"]
    return g


@pytest.mark.parametrize("row", RUN_ROWS, ids=IDS)
def test_variant(children, row):
    group, env, case, must, must_not = row
    g = _group(children, group)
    rec = g["records"].get(case)
    assert rec is not None, f"{case}: the child of group {group} wrote no record"
    assert rec["env"] == {k: env[k] for k in env}, rec["env"]  # the switch reached the child as the row states it
    assert "exception" not in rec, rec.get("exception")
    print(case, rec["errors"], "seconds", rec["seconds"])
    for name, (value, bound) in rec["errors"].items():
        assert value < bound, (case, name, value, bound)
    assert all(rec["checks"].values()), (case, rec["checks"])
    if rec["deterministic"] is not None:
        assert rec["deterministic"], f"{case}: two runs of the same launch differ bitwise"
    assert dispatched(g["log"], case, must, must_not), (case, must, must_not, sorted(set(launches(g["log"], case))))


@pytest.mark.parametrize("row", [r for r in RUN_ROWS if r[4] is not None], ids=[i for i, r in zip(IDS, RUN_ROWS) if r[4] is not None])
def test_dispatch_check_rejects_the_default_run(children, row):
    """The same check on the log of the child without switches: it has to fail, or it could not tell the variants apart."""
    group, env, case, must, must_not = row
    for need in (group, "D"):
        _group(children, need)
    d = children["D"]
    assert case in d["records"] and "exception" not in d["records"][case]
    assert not dispatched(d["log"], case, must, must_not), (case, must, sorted(set(launches(d["log"], case))))


def test_default_run_meets_the_same_bounds(children):
    """Group D's records: the default kernels at the variants' shapes (several of which no other test runs) hold the same bounds."""
    d = _group(children, "D")
    print("wall time of the children:", {g: children[g].get("seconds") for g in GROUPS})
    assert sorted(d["records"]) == sorted(group_cases("D"))
    for case, rec in d["records"].items():
        assert "exception" not in rec, (case, rec.get("exception"))
        assert all(v < b for v, b in rec["errors"].values()) and all(rec["checks"].values()), (case, rec)
        assert rec["deterministic"] in (None, True), case


def test_weight_gradient_variants_change_the_bits(children):
    """A second, independent sign that SEGMIF_WGRAD3X3 took effect: the exact-fp32 kernel and the one-team kernel sum in another
    order (or another arithmetic) than the default, so the weight gradient's bits differ from group D's."""
    d = _group(children, "D")["records"]
    for group, env, case, must, must_not in RUN_ROWS:
        if case.startswith("wgrad-") and must_not is not None:
            assert _group(children, group)["records"][case]["hash"] != d[case]["hash"], (group, case)
