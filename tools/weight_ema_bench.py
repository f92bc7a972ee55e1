"""Times the optimizer step on the MI355X with and without the weight average (csrc/weight_ema.hip), over the parameters of
Network3('mit_b3') and of Fusion_Network3_ac with seeded random gradients:

    plain        FusedAdamW.step()                                              one multi-tensor launch
    plain+ema    FusedAdamW(ema_decay=0.9999).step()                            ... and one more over the same table
    guarded      FusedAdamW(max_grad_norm=1, skip_nonfinite=True).step()        norm (two launches) + guarded update
    guarded+ema  the same with ema_decay=0.9999                                 ... and one more

Device events around a window of --steps steps (so the host's share of a step - building and uploading the table - is inside the
figure, as it is in training), --warmup steps first, --repeats windows per leg with the legs alternating; the table reports the
median and the spread per step.  Then the two kernels on their own - segmif_adamw_f32 and segmif_weight_ema_f32 launched back
to back on one prebuilt table, no host work between them - with the bytes the algorithm moves (update: p, g, m, v read and p,
m, v written, 28 B per element; average: p, hi, lo read and hi, lo written, 20 B per element) over that time.

--parent-tree DIR: a checkout of the commit BEFORE the average.  Its plain and guarded legs are timed in fresh child processes of
this script, one before and one after this tree's legs (same session, same machine), so that "off costs nothing" is a
measurement: compare this tree's plain / guarded with the parent's, against the spread between the parent's two runs.

    python tools/weight_ema_bench.py [--parent-tree DIR] [--out profiles/weight_ema_bench.txt]
"""
import argparse
import ctypes
import inspect
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"plain": {}, "plain+ema": dict(ema_decay=0.9999), "guarded": dict(max_grad_norm=1.0, skip_nonfinite=True),
        "guarded+ema": dict(max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9999)}


def window(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def alternate(variants, args):
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in variants}
    for _ in range(args.repeats):
        for k, fn in variants:
            times[k].append(window(fn, args.steps))
    return times


def kernels_alone(params, args):
    """segmif_adamw_f32 and segmif_weight_ema_f32 on one prebuilt table: (ms per launch of each, launched alternately)"""
    from segmif_amd import _lib
    from segmif_amd.utils import optimizer as om
    lib = _lib.load()
    m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    pairs = [(p.detach().clone(), torch.zeros_like(p)) for p in params]
    items = [(p, p.grad, a, b, 1e-6, 0.01) for p, a, b in zip(params, m, v)]
    blob, (o_co, o_ce, _), nchunks = om._upload_table(items, None, params[0].device, pairs)
    base, stream = blob.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o_ema = len(items) * ctypes.sizeof(om._AdamEntry)

    def adamw():
        _lib.check(lib.segmif_adamw_f32(base, base + o_ce, base + o_co, nchunks, om._CHUNK, 0.9, 0.999, 1e-8, 0.1, 0.0316, stream), "adamw")

    def ema():
        _lib.check(lib.segmif_weight_ema_f32(base, base + o_ema, base + o_ce, base + o_co, nchunks, om._CHUNK, 0.9999, 0, 1, None, None,
                                             None, stream), "ema")

    times = alternate([("adamw", adamw), ("ema", ema)], args)
    torch.cuda.synchronize()
    del blob
    return times


def bench(name, module, args, legs):
    from segmif_amd.utils.optimizer import FusedAdamW
    params = [p for p in module.parameters() if p.requires_grad]
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
    kw = dict(lr=1e-6, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opts = {k: FusedAdamW(params, **kw, **LEGS[k]) for k in legs}
    times = alternate([(k, o.step) for k, o in opts.items()], args)
    for k, o in opts.items():
        if "guarded" in k:
            st = o.grad_stats()
            assert st["skipped"] == 0 and st["attempts"] == args.warmup + args.repeats * args.steps, st
    out = {"name": name, "tensors": len(params), "elements": sum(p.numel() for p in params), "legs": times}
    if "plain+ema" in legs:
        out["kernels"] = kernels_alone(params, args)
    return out


def report(res, lines, label):
    n = res["elements"]
    lines.append(f"{res['name']} [{label}]: {res['tensors']} tensors, {n} elements; update traffic {28 * n / 1e6:.1f} MB, "
                 f"average {20 * n / 1e6:.1f} MB more")
    base = statistics.median(res["legs"]["plain"])
    for k, t in res["legs"].items():
        med = statistics.median(t)
        lines.append(f"  {k:<12} median {med:8.4f} ms/step   min {min(t):8.4f}   max {max(t):8.4f}   x{med / base:5.3f} of plain")
    for k, nbytes in (("adamw", 28 * n), ("ema", 20 * n)):
        if k in res.get("kernels", {}):
            t = res["kernels"][k]
            med = statistics.median(t)
            lines.append(f"  kernel alone: {k:<6} median {med:8.4f} ms/launch   min {min(t):8.4f}   max {max(t):8.4f}   "
                         f"{nbytes / med / 1e6:7.1f} GB/s of algorithm bytes")


def run_here(args, legs):
    from segmif_amd.core import Fusion_Network3_ac, Network3
    torch.manual_seed(0)
    return [bench("Network3('mit_b3')", Network3("mit_b3", 9, pretrained=None).cuda(), args, legs),
            bench("Fusion_Network3_ac", Fusion_Network3_ac().cuda(), args, legs)]


def run_parent(args):
    """the plain and guarded legs of the tree at --parent-tree, in a fresh process (its own library, its own package)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--emit-json", "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--repeats", str(args.repeats)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    return json.loads([line for line in out.splitlines() if line.startswith("{")][-1])["results"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9, help="windows per leg (alternating)")
    ap.add_argument("--parent-tree", help="checkout of the commit before the average (built): its plain and guarded legs are timed too")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose segmif_amd is timed (default: this one)")
    ap.add_argument("--emit-json", action="store_true", help="print the raw windows as one JSON line instead of writing the report")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_ema_bench.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("weight_ema_bench needs the MI355X: a timing from anywhere else says nothing about it")
    sys.path.insert(0, os.path.abspath(args.tree))
    from segmif_amd.utils.optimizer import FusedAdamW
    has_ema = "ema_decay" in inspect.signature(FusedAdamW.__init__).parameters
    legs = list(LEGS) if has_ema else ["plain", "guarded"]
    if args.emit_json:
        print(json.dumps({"results": run_here(args, legs)}))
        return 0
    if not has_ema:
        raise RuntimeError(f"{args.tree}: FusedAdamW has no ema_decay; a tree without the average is timed through --parent-tree")
    lines = [f"optimizer step with and without the weight average, device events over {args.repeats} windows of {args.steps} steps after "
             f"{args.warmup} warm-up steps, {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    runs = []
    if args.parent_tree:
        runs.append(("parent commit, before", run_parent(args)))
    runs.append(("this tree", run_here(args, legs)))
    if args.parent_tree:
        runs.append(("parent commit, after", run_parent(args)))
    for i in range(2):
        for label, results in runs:
            report(results[i], lines, label)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
