"""Child of tests/test_calibration_host.py: sends the single-argument mutations of one valid baseline of
segmif_calibration_stats_f32 (include/segmif_calib.h; never the baseline) to the library in a process that sees NO GPU, and writes
one JSON line per row.

    python _calibration_child.py RECORDS.jsonl

The parent's environment hides every device; before the first call this process proves it with tests/_abi_contract_child.py's
no_device_proof.  If the proof fails it writes {"refused": reason} and exits with status 3 without calling anything.  Line
protocol: {"begin": i} before row i's call, {"i": i, "label": ..., "rc": ...} after it."""
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

NAME = "segmif_calibration_stats_f32"
# a valid baseline on fake addresses (never dereferenced by a call that is rejected)
BASE = dict(desc="ok", temperatures=(1.0, 2.0), edges=(0.25, 0.5, 0.75), thresholds=(0.9, 0.968), NT=None, NE=None, NK=None,
            x=0x100000, label=0x200000, counts=0x300000, above=0x400000, totals=0x500000, sums=0x600000, workspace=0x700000,
            conf=0x800000, pred=0x900000, B=2, IH=3, IW=5, OH=11, OW=19, C=9, ldx=9)
MUTATIONS = [("desc", None), ("x", None), ("label", None), ("counts", None), ("totals", None), ("sums", None), ("workspace", None),
             ("above", None),  # NK = 2 > 0
             ("C", 0), ("C", -1), ("C", 33), ("ldx", 8),
             ("NT", 0), ("NT", -1), ("NT", 17), ("NE", -1), ("NE", 32), ("NK", -1), ("NK", 9),
             ("temperatures", (1.0, 0.0)), ("temperatures", (-1.0, 2.0)), ("temperatures", (math.inf, 2.0)), ("temperatures", (1.0, math.nan)),
             ("edges", (0.25, 0.25, 0.75)), ("edges", (0.5, 0.25, 0.75)), ("edges", (0.0, 0.5, 0.75)), ("edges", (0.25, 0.5, 1.0)),
             ("edges", (-0.5, 0.5, 0.75)), ("edges", (0.25, math.nan, 0.75)),
             ("thresholds", (0.9, 1.5)), ("thresholds", (-0.1, 0.968)), ("thresholds", (math.nan, 0.968)),
             ("B", 0), ("B", -2), ("IH", 0), ("IW", 0), ("OH", 0), ("OW", 0), ("OW", -19),
             ("B", 65536), ("OH", 65536)]


def rows():
    """[(i, label, argument, value)]"""
    return [(i, f"{NAME}:{arg}={value}", arg, value) for i, (arg, value) in enumerate(MUTATIONS)]


def call(lib, v):
    from segmif_amd import _lib
    desc = None
    if v["desc"] is not None:
        d = _lib.SegmifCalib()
        d.n_temperatures = len(v["temperatures"]) if v["NT"] is None else v["NT"]
        d.n_edges = len(v["edges"]) if v["NE"] is None else v["NE"]
        d.n_thresholds = len(v["thresholds"]) if v["NK"] is None else v["NK"]
        for field, key in ((d.temperatures, "temperatures"), (d.edges, "edges"), (d.thresholds, "thresholds")):
            for i in range(len(field)):  # (beyond the given values: legal ones, so that a count alone is what a row mutates)
                field[i] = {"temperatures": 1.0 + i, "edges": (i + 1) / 64.0, "thresholds": 0.5}[key]
            for i, x in enumerate(v[key]):
                field[i] = x
        desc = ctypes.byref(d)
    return lib.segmif_calibration_stats_f32(desc, v["x"], v["label"], v["counts"], v["above"], v["totals"], v["sums"], v["workspace"],
                                            v["conf"], v["pred"], v["B"], v["IH"], v["IW"], v["OH"], v["OW"], v["C"], v["ldx"], None)


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
        for i, label, arg, value in rows():
            v = dict(BASE)
            assert v[arg] != value or (value is None and v[arg] is not None), label  # a mutation, never the baseline
            v[arg] = value
            emit({"begin": i})
            try:
                rc = int(call(lib, v))
            except Exception as e:  # noqa: BLE001 - a row the binding itself refuses is this table's mistake: say so in its record
                rc = f"the call raised {e!r}"
            emit({"i": i, "label": label, "rc": rc})
    return 0


if __name__ == "__main__":
    sys.exit(main())
