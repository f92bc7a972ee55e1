"""Child of tests/test_abi_contract_host.py: sends the mutations of tests/_abi_contract_table.py (never a baseline) to the library in
a process that sees NO GPU, and writes one JSON line per row.

    python _abi_contract_child.py RECORDS.jsonl FIRST_ROW

The parent's environment hides every device from the HIP runtime.  Before the first call this process proves it: torch counts no
device, hipGetDeviceCount of every HIP runtime mapped into the process reports none, and segmif_device_name fails.  If any of the
three says otherwise it writes {"refused": reason} and exits with status 3 without calling anything: with a device, a call the
library fails to reject would become a kernel running on the table's fake addresses.

Line protocol: {"begin": i} before row i's call, {"i": i, "entry": ..., "mutation": ..., "rc": ...} after it - a row whose call
kills the process leaves its "begin" as the last line, and the parent starts the next child behind it."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def no_device_proof(lib):
    """None when the process provably has no GPU, else the reason it may have one"""
    import torch
    try:
        n = torch.cuda.device_count()
    except Exception as e:  # noqa: BLE001
        return f"torch.cuda.device_count() raised {e!r}"
    if n != 0:
        return f"torch counts {n} device(s)"
    runtimes = set()
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split(None, 5)[-1].strip() if line.count(" ") >= 5 else ""
            if "libamdhip64" in os.path.basename(path):
                runtimes.add(path)
    if not runtimes:
        return "no HIP runtime is mapped into the process: cannot ask it for its device count"
    for path in sorted(runtimes):
        rt = ctypes.CDLL(path)  # already loaded: the same handle
        count = ctypes.c_int(-1)
        rc = rt.hipGetDeviceCount(ctypes.byref(count))
        if count.value > 0 or (rc == 0 and count.value != 0):
            return f"{path}: hipGetDeviceCount -> status {rc}, {count.value} device(s)"
        if rc == 0 and count.value == 0:
            continue
        if rc != 100:  # hipErrorNoDevice
            return f"{path}: hipGetDeviceCount failed with status {rc}, not hipErrorNoDevice: no proof either way"
    buf = ctypes.create_string_buffer(256)
    rc = lib.segmif_device_name(buf, 256)
    if rc == 0:
        return f"segmif_device_name found a device: {buf.value!r}"
    return None


def main():
    out_path, first = sys.argv[1], int(sys.argv[2])
    hidden = {k: os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    with open(out_path, "a") as out:
        def emit(rec):
            out.write(json.dumps(rec) + "\n")
            out.flush()  # (in the kernel's hands: it survives the death of this process)
        if any(v != "-1" for v in hidden.values()):
            emit({"refused": f"the environment does not hide the devices: {hidden}"})
            return 3
        from segmif_amd import _lib
        import _abi_contract_table as table
        lib = _lib.load()
        why = no_device_proof(lib)
        if why is not None:
            emit({"refused": why})
            return 3
        emit({"proof": "no device: torch, hipGetDeviceCount and segmif_device_name agree"})
        for i, entry, label, arg, value, _ in table.all_rows():
            if i < first:
                continue
            values = entry.baseline()
            for a, v in zip(arg, value) if isinstance(arg, tuple) else [(arg, value)]:  # (a tuple of names: a rule about them together)
                same = values[a] is None if v is None else values[a] == v
                assert not same, (entry.key, label)  # a mutation, never the baseline
                values[a] = v
            keep = []
            emit({"begin": i})
            try:
                rc = int(entry.call(lib, values, keep))
            except Exception as e:  # noqa: BLE001 - a row the binding itself refuses is the table's mistake: say so in its record
                rc = f"the call raised {e!r}"
            emit({"i": i, "entry": entry.key, "mutation": label, "rc": rc})
    return 0


if __name__ == "__main__":
    sys.exit(main())
