"""Child of tests/test_copy_paste_host.py: sends the single-argument mutations of one valid baseline per entry of
include/segmif_paste.h (never the baseline) to the library in a process that sees NO GPU, and writes one JSON line per row.

    python _copy_paste_child.py RECORDS.jsonl

The parent's environment hides every device; before the first call this process proves it with tests/_abi_contract_child.py's
no_device_proof.  If the proof fails it writes {"refused": reason} and exits with status 3 without calling anything.  Line
protocol: {"begin": i} before row i's call, {"i": i, "label": ..., "rc": ...} after it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# valid baselines on fake, 16-byte aligned addresses (never dereferenced by a call that is rejected), in the C argument order
BASE = {
    "segmif_object_boxes_i32": dict(root=0x100000, label=0x200000, n=2, H=37, W=53, K=9, class_mask=0x1fe, min_area=64, max_box=500, frame0=0,
                                    records=0x300000, capacity=16, counter=0x400000, workspace=0x500000, stream=None),
    "segmif_object_pack_u8": dict(records=0x100000, offsets=0x200000, M=3, store_pixels=100, root=0x300000, ir=0x400000, vis=0x500000,
                                  mask=0x600000, frame0=0, n=2, H=37, W=53, patches=0x700000, stream=None),
    "segmif_copy_paste_f32": dict(ir3=0x100000, vis3=0x200000, mask3=0x300000, label=0x400000, B=2, h=8, w=12, records=0x500000,
                                  offsets=0x600000, patches=0x700000, M=3, store_pixels=100, table=0x800000, P=3, n_class=9,
                                  ir3_out=0x900000, vis3_out=0xa00000, mask3_out=0xb00000, label_out=0xc00000, pasted=0xd00000,
                                  tally=0xe00000, stream=None),
}
MUTATIONS = {
    "segmif_object_boxes_i32": [("root", None), ("label", None), ("counter", None), ("workspace", None), ("records", None),
                                ("K", 0), ("K", -1), ("K", 33), ("min_area", 0), ("min_area", -3), ("max_box", 0), ("capacity", -1),
                                ("frame0", -1), ("frame0", 2 ** 31 - 2), ("n", 0), ("n", -2), ("n", 32768), ("H", 0), ("W", 0), ("W", -53),
                                ("HW", (65536, 32768)), ("HW", (46341, 46341))],
    "segmif_object_pack_u8": [("records", None), ("offsets", None), ("root", None), ("ir", None), ("vis", None), ("mask", None),
                              ("patches", None), ("M", 0), ("M", -1), ("store_pixels", -1), ("frame0", -1), ("n", 0), ("n", 32768),
                              ("H", 0), ("W", 0), ("HW", (65536, 32768))],
    "segmif_copy_paste_f32": [("ir3", None), ("vis3", None), ("mask3", None), ("label", None), ("records", None), ("offsets", None),
                              ("patches", None), ("table", None), ("ir3_out", None), ("vis3_out", None), ("mask3_out", None),
                              ("label_out", None), ("pasted", None), ("P", 9), ("P", -1), ("w", 10), ("w", 13), ("w", 0), ("h", 0), ("B", 0),
                              ("B", 65536), ("n_class", 0), ("n_class", 256), ("M", 0), ("store_pixels", 0), ("ir3", 0x100004),
                              ("label_out", 0xc00008)],
}


def rows():
    """[(i, label, entry, argument, value)]"""
    out = []
    for entry, muts in MUTATIONS.items():
        for arg, value in muts:
            out.append((len(out), f"{entry}:{arg}={value}", entry, arg, value))
    return out


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
        for i, label, entry, arg, value in rows():
            v = dict(BASE[entry])
            if arg == "HW":
                v["H"], v["W"] = value
            else:
                assert v[arg] != value or (value is None and v[arg] is not None), label  # a mutation, never the baseline
                v[arg] = value
            emit({"begin": i})
            try:
                rc = int(getattr(lib, entry)(*v.values()))
            except Exception as e:  # noqa: BLE001 - a row the binding itself refuses is this table's mistake: say so in its record
                rc = f"the call raised {e!r}"
            emit({"i": i, "label": label, "rc": rc})
    return 0


if __name__ == "__main__":
    sys.exit(main())
