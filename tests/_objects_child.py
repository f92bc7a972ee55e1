"""Child of tests/test_objects_host.py: sends the single-argument mutations of one valid baseline of segmif_object_stats_i32
(include/segmif_objects.h; never the baseline) to the library in a process that sees NO GPU, and writes one JSON line per row.

    python _objects_child.py RECORDS.jsonl

The parent's environment hides every device; before the first call this process proves it with tests/_abi_contract_child.py's
no_device_proof.  If the proof fails it writes {"refused": reason} and exits with status 3 without calling anything.  Line
protocol: {"begin": i} before row i's call, {"i": i, "label": ..., "rc": ...} after it."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

NAME = "segmif_object_stats_i32"
# a valid baseline on fake addresses (never dereferenced by a call that is rejected)
BASE = dict(desc="ok", connectivity=8, n_edges=None, edges=(1024, 9216), pred=0x100000, label=0x200000, obj=0x300000, mass=0x400000,
            status=0x500000, workspace=0x600000, root_g=0x700000, root_p=0x800000, B=2, H=37, W=53, K=9)
MUTATIONS = [("desc", None), ("pred", None), ("label", None), ("obj", None), ("mass", None), ("status", None), ("workspace", None),
             ("K", 0), ("K", -1), ("K", 33),
             ("connectivity", 0), ("connectivity", 6), ("connectivity", -8), ("connectivity", 16),
             ("n_edges", -1), ("n_edges", 4),
             ("edges", (1024, 1024)), ("edges", (9216, 1024)), ("edges", (0, 9216)), ("edges", (-5, 9216)),
             ("B", 0), ("B", -2), ("H", 0), ("H", -37), ("W", 0), ("W", -53),
             ("HW", (65536, 32768)), ("HW", (46341, 46341)), ("HW", (2, 2 ** 30)),  # H * W >= 2^31
             ("B", 32768)]  # the grid's z holds 2 B


def rows():
    """[(i, label, argument, value)]"""
    return [(i, f"{NAME}:{arg}={value}", arg, value) for i, (arg, value) in enumerate(MUTATIONS)]


def call(lib, v):
    from segmif_amd import _lib
    desc = None
    if v["desc"] is not None:
        d = _lib.SegmifObjects()
        d.connectivity = v["connectivity"]
        d.n_edges = len(v["edges"]) if v["n_edges"] is None else v["n_edges"]
        for i in range(4):  # (beyond the given values: legal ones, so that a count alone is what a row mutates)
            d.edges[i] = 10 ** (5 + i)
        for i, e in enumerate(v["edges"]):
            d.edges[i] = e
        desc = ctypes.byref(d)
    return lib.segmif_object_stats_i32(desc, v["pred"], v["label"], v["obj"], v["mass"], v["status"], v["workspace"], v["root_g"],
                                       v["root_p"], v["B"], v["H"], v["W"], v["K"], None)


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
            if arg == "HW":
                v["H"], v["W"] = value
            else:
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
