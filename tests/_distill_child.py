"""Child of tests/test_distill_host.py: sends the single-argument mutations of one valid baseline per entry point of
include/segmif_distill.h (never a baseline) to the library in a process that sees NO GPU, and writes one JSON line per row.

    python _distill_child.py RECORDS.jsonl

The parent's environment hides every device; before the first call this process proves it with tests/_abi_contract_child.py's
no_device_proof (torch, hipGetDeviceCount of every mapped HIP runtime, segmif_device_name).  If the proof fails it writes
{"refused": reason} and exits with status 3 without calling anything.  Line protocol: {"begin": i} before row i's call,
{"i": i, "label": ..., "rc": ...} after it."""
import ctypes
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FWD, BWD = "segmif_distill_objective_f32", "segmif_distill_objective_bwd_f32"
# one valid baseline per entry point, on fake addresses (16-byte aligned, never dereferenced by a call that is rejected)
BASE = {
    FWD: dict(desc="ok", temperature=2.0, mode=1, student=0x100000, teacher=0x200000, workspace=0x300000, record4=0x400000, rows=512,
              rows_per_sample=256, C=9, lds=9, ldt=9),
    BWD: dict(desc="ok", temperature=2.0, mode=1, student=0x100000, teacher=0x200000, workspace=0x300000, record4=0x400000,
              upstream=0x500000, dstudent=0x600000, rows=512, rows_per_sample=256, C=9, lds=9, ldt=9, ldd=9),
}
COMMON = [("desc", None), ("student", None), ("teacher", None), ("workspace", None), ("record4", None), ("C", 0), ("C", -1), ("C", 33),
          ("lds", 8), ("ldt", 8), ("temperature", 0.0), ("temperature", -1.0), ("temperature", math.inf), ("temperature", math.nan),
          ("mode", 2), ("mode", -1), ("rows", 0), ("rows", -512), ("rows_per_sample", 0), ("rows_per_sample", -256),
          ("rows_per_sample", 255),  # rows % rows_per_sample != 0
          ("rows", 65536 * 256)]     # B = 65536: beyond SEGMIF_DISTILL_MAX_BATCH, the grid's second dimension
MUTATIONS = {FWD: COMMON, BWD: COMMON + [("upstream", None), ("dstudent", None), ("ldd", 8)]}


def rows():
    """[(i, entry point, label, argument, value)]"""
    out = []
    for name in (FWD, BWD):
        for arg, value in MUTATIONS[name]:
            out.append((len(out), name, f"{name}:{arg}={value}", arg, value))
    return out


def call(lib, name, v):
    from segmif_amd import _lib
    desc = None
    if v["desc"] is not None:
        d = _lib.SegmifDistill()
        d.temperature, d.mode = v["temperature"], v["mode"]
        desc = ctypes.byref(d)
    if name == FWD:
        return lib.segmif_distill_objective_f32(desc, v["student"], v["teacher"], v["workspace"], v["record4"], v["rows"],
                                                v["rows_per_sample"], v["C"], v["lds"], v["ldt"], None)
    return lib.segmif_distill_objective_bwd_f32(desc, v["student"], v["teacher"], v["workspace"], v["record4"], v["upstream"],
                                                v["dstudent"], v["rows"], v["rows_per_sample"], v["C"], v["lds"], v["ldt"], v["ldd"], None)


def main():
    out_path = sys.argv[1]
    hidden = {k: os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    with open(out_path, "a") as out:
        def emit(rec):
            out.write(json.dumps(rec) + "\n")
            out.flush()
        if any(v != "-1" for v in hidden.values()):
            emit({"refused": f"the environment does not hide the devices: {hidden}"})
            return 3
        from segmif_amd import _lib
        from _abi_contract_child import no_device_proof
        lib = _lib.load()
        why = no_device_proof(lib)
        if why is not None:
            emit({"refused": why})
            return 3
        emit({"proof": "no device: torch, hipGetDeviceCount and segmif_device_name agree"})
        for i, name, label, arg, value in rows():
            v = dict(BASE[name])
            same = v[arg] is None if value is None else (v[arg] == value)
            assert not same, label  # a mutation, never the baseline
            v[arg] = value
            emit({"begin": i})
            try:
                rc = int(call(lib, name, v))
            except Exception as e:  # noqa: BLE001 - a row the binding itself refuses is this table's mistake: say so in its record
                rc = f"the call raised {e!r}"
            emit({"i": i, "label": label, "rc": rc})
    return 0


if __name__ == "__main__":
    sys.exit(main())
