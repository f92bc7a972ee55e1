"""The rejection half of the C ABI's contract (the headers under include/: every entry point returns SEGMIF_EINVAL for anything
outside its documented domain): tests/_abi_contract_table.py holds one valid baseline per entry point and its
single-argument mutations; tests/_abi_contract_child.py sends the mutations - never a baseline - in a child process that sees no
GPU and has proved so; the tests below only read its records and assert -22.

Why a child without devices: tests that are not marked `gpu` also run on machines that have one.  With no device, a call the
library fails to reject ends as a HIP launch error code; with one it would be a kernel running on the table's fake addresses.
The child's environment is this process's plus HIP_VISIBLE_DEVICES = CUDA_VISIBLE_DEVICES = -1, nothing else.  It is started with
subprocess.run (never exec) under `timeout -k 10 120`, like the children of tests/test_gpu_kernel_variants.py.  A row whose call
kills the child is recorded as such and the next child starts behind it (at most MAX_CHILDREN of them)."""
import json
import os
import subprocess
import sys
import time

import pytest

import _abi_contract_table as table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_abi_contract_child.py")
ROWS = table.all_rows()
IDS = [f"{e.key}:{label}" for _, e, label, _, _, _ in ROWS]
MAX_CHILDREN = 6
HIDE = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


_RECORDS = {}


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """{row index: return code or a string saying how the call died}, plus "error" when no child could run the table.  The host test
    of a header imports this fixture for the cases its header lists; the children run once for all of them."""
    if not _RECORDS:
        _RECORDS.update(_run_children(tmp_path_factory))
    return _RECORDS


def _run_children(tmp_path_factory):
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()  # (as the other host tests do) - the child never compiles
    rec_path = str(tmp_path_factory.mktemp("abi_contract") / "records.jsonl")
    env = dict(os.environ)
    env.update(HIDE)
    out, first, t0 = {"seconds": None}, 0, time.time()
    for _ in range(MAX_CHILDREN):
        cmd = ["timeout", "-k", "10", "120", sys.executable, CHILD, rec_path, str(first)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
            code, tail = r.returncode, (r.stdout[-1500:] + "\n" + r.stderr[-2500:])
        except subprocess.TimeoutExpired as e:
            code, tail = 124, str(e)
        lines = [json.loads(l) for l in open(rec_path)] if os.path.exists(rec_path) else []
        begun = None
        for l in lines:
            if "refused" in l:
                out["error"] = "the child refused to call anything: " + l["refused"]
            elif "begin" in l:
                begun = l["begin"]
            elif "i" in l:
                out[l["i"]] = l["rc"]
                begun = None
        if "error" in out or code == 0:
            break
        if begun is None or code in (124, 137):  # died outside a call, or hung: nothing to step over
            out["error"] = f"the child ended with status {code} outside a call\n{tail}"
            break
        out[begun] = f"the call killed the child (status {code})"
        first = begun + 1
    else:
        out["error"] = f"{MAX_CHILDREN} children died inside calls; the last at row {first - 1}"
    out["seconds"] = round(time.time() - t0, 1)
    return out


def test_the_child_saw_no_device_and_ran_every_row(records):
    assert "error" not in records, records["error"]
    print("children's wall time:", records["seconds"], "s for", len(ROWS), "rows")
    missing = [IDS[i] for i in range(len(ROWS)) if i not in records]
    assert not missing, missing[:20]


def check_rejected(records, i):
    """row i of the table was sent and came back as SEGMIF_EINVAL"""
    assert "error" not in records, records["error"]
    assert i in records, f"{IDS[i]}: the child wrote no record"
    assert records[i] == table.EINVAL, f"{IDS[i]} returned {records[i]}, not SEGMIF_EINVAL.  Forbidden by: {ROWS[i][5]}"


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_rejected(records, row):
    check_rejected(records, row[0])


def test_every_entry_point_has_a_contract_row_or_an_exemption():
    """A new entry point without a row here fails the suite.  An exemption carries its reason: a size query without pointers, or
    the existing host test that already sends its rejections."""
    from segmif_amd import _lib
    tabled = {e.name for e in table.ENTRIES}
    bound = [name for signatures in _lib.HEADERS.values() for name in signatures]
    for name in bound:
        assert (name in tabled) != (name in table.EXEMPT), f"{name}: needs rows in tests/_abi_contract_table.py or an EXEMPT reason (not both)"
    assert not (tabled | set(table.EXEMPT)) - set(bound), "the table names entry points the library does not have"
    for name, why in table.EXEMPT.items():
        assert why.startswith("size query / no pointers") or why.startswith("rejections covered by tests/"), (name, why)
        if why.startswith("rejections covered by "):
            path = why.split("rejections covered by ", 1)[1].split("::")[0]
            text = open(os.path.join(ROOT, path)).read()
            assert name in text and "-22" in text, f"{name}: {path} does not send it a rejected call"
            if "::" in why:
                assert "def " + why.split("::", 1)[1] + "(" in text, why


def test_table_shape():
    """Every baseline is mutated, labels are unique, every row has its reason, and every required pointer / count / pitch of a
    baseline has its generic rows (the tags generate them: this guards the generator)."""
    assert len(set(IDS)) == len(IDS)
    for e in table.ENTRIES:
        ms = e.mutations()
        assert ms, e.key
        labels = {m[0] for m in ms}
        for a, t in e.args + e.tail:
            if t["kind"] == "ptr" and t["req"]:
                assert f"{a}=NULL" in labels, (e.key, a)
            if t["kind"] == "count":
                assert {f"{a}=0", f"{a}=-1"} <= labels, (e.key, a)
        assert all(isinstance(m[3], str) and len(m[3]) > 8 for m in ms), e.key
