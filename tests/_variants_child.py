"""Child process of tests/test_gpu_kernel_variants.py (run as a script, not collected): `_variants_child.py GROUP OUT.json`.

Runs every case of the group with the library-side switches of its environment in force, each through the public entry point
and against the fp64 CPU reference of the existing test of the default variant, whose helpers and bounds are imported from the
test modules.  One JSON record per case goes to OUT.json (rewritten after every case, so a child that dies leaves the cases it
finished): the errors with their bounds, boolean checks, whether a second run gave the same bits, a hash of the output.  Marker
lines on stderr bracket each case for the parent, which reads the runtime's kernel log between them."""
import hashlib
import json
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import test_gpu_backward as tb  # noqa: E402
import test_gpu_kernel_variants as tv  # noqa: E402
import test_gpu_kernels as tk  # noqa: E402
import test_gpu_planes16 as tp  # noqa: E402
import test_gpu_round4 as t4  # noqa: E402
import test_gpu_round5 as t5  # noqa: E402
from segmif_amd import autograd as ag, ops  # noqa: E402


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def wgrad(name, train_conv):
    """test_conv_backward's body (test_gpu_backward.py) under ops.modes(train_conv=...), the device part run twice."""
    B, H, W, Cin, N, k, s, p, d, act = tv.WGRAD_CASES[name]
    x, w, b = tb.rnd(B, Cin, H, W, seed=5), tb.rnd(N, Cin, k, k, seed=6), tb.rnd(N, seed=7)
    slope = torch.tensor([0.25])
    xr, wr, br, sr = (tb.leaf(t, double=True) for t in (x, w, b, slope))
    y = F.conv2d(xr, wr, br, stride=s, padding=p, dilation=d)
    y = F.relu(y) if act == 1 else (F.prelu(y, sr) if act == 2 else y)
    g = tb.rnd(*y.shape, seed=8)
    y.backward(g.double())
    runs = []
    with ops.modes(train_conv=train_conv):
        for _ in range(2):
            xg = tb.leaf(x.permute(0, 2, 3, 1).contiguous(), "cuda")
            wg, bg, sg = tb.leaf(w, "cuda"), tb.leaf(b, "cuda"), tb.leaf(slope, "cuda")
            yg = ag.conv2d(xg, wg, bg, k=k, stride=s, pad=p, dil=d, act=act, slope=sg if act == 2 else None)
            yg.backward(g.permute(0, 2, 3, 1).contiguous().cuda())
            runs.append((yg.detach(), xg.grad, wg.grad, bg.grad) + ((sg.grad,) if act == 2 else ()))
    got = runs[0]
    errors = {"y": (tb.err(got[0], y.permute(0, 2, 3, 1)), tb.TOL), "dx": (tb.err(got[1], xr.grad.permute(0, 2, 3, 1)), tb.TOL),
              "dw": (tb.err(got[2], wr.grad), tb.TOL), "db": (tb.err(got[3], br.grad), tb.TOL)}
    if act == 2:
        errors["dslope"] = (tb.err(got[4], sr.grad), 1e-4)
    return errors, {}, same(*runs), digest(got[2])


def gemm_split(arith, M, N, K):
    """test_gemm_split_bf16x6 (test_gpu_kernels.py) / test_gemm_split_f16x3 (test_gpu_planes16.py): bias, GELU + residual, ReLU,
    a pitched rows view; against fp64, within 3x of the exact-fp32 GEMM's error, 1e-6 of each output's conditioning."""
    f16 = arith == "f16x3"
    gen = torch.Generator().manual_seed(M + N + K)
    x = (torch.rand(M, K, generator=gen) * 2 - 1) * 10.0 ** (torch.rand(M, K, generator=gen) * 6 - 4)
    w = tk.rnd(N, K, seed=2) * 0.1
    if f16:
        w = w * 10.0 ** tp.rnd(N, 1, seed=5, lo=-2, hi=1)
    b, r = tk.rnd(N, seed=3), tk.rnd(M, N, seed=4)
    ref_lin = x.double() @ w.double().t() + b.double()
    packs = ops.pack_linear(w.cuda(), half=True) if f16 else ops.pack_linear(w.cuda())
    checks = {"split image": packs[1] is not None and (not f16 or packs[1].half is not None)}
    wide = torch.zeros(M, K + 32, device="cuda")
    wide[:, :K] = x.cuda()
    xv = wide[:, :K]
    tol = tp.TOL if f16 else tk.TOL
    errors, outs, again = {}, [], []
    guard = ops.Planes16Guard("cuda") if f16 else None
    prev = ops.install_guard(guard) if f16 else None
    try:
        for act, use_res in ((0, False), (3, True), (1, False)):
            ref = tk.act_ref(ref_lin, act)
            if use_res:
                ref = ref + r.double()
            kw = dict(bias=b.cuda(), act=act, res=r.cuda() if use_res else None)
            yv = ops.linear_auto(xv, packs, N, **kw)
            y32 = ops.linear(xv, packs[0], N, **kw)
            e, e32 = tk.err(yv, ref), tk.err(y32, ref)
            errors[f"act{act}"] = (e, tol)
            errors[f"act{act} vs fp32 tiles"] = (e, 3.0 * e32 + 1e-7)
            outs.append(yv)
            again.append(ops.linear_auto(xv, packs, N, **kw))
        cond = x.double().abs() @ w.double().abs().t() + b.double().abs()
        errors["conditioning"] = (float(((outs[0].double().cpu() - ref_lin).abs() / cond).max()), 1e-6)
    finally:
        if f16:
            ops.install_guard(prev)
    if f16:
        m = guard.maxima()
        checks["range slots"] = m.numel() == 6 and all(float(v) == float(x.abs().max().half()) for v in m)  # six f16x3 launches
        checks["guard ok"] = bool(guard.ok())
    return errors, checks, same(outs, again), digest(*outs)


def gemm_split_patch(B, H, W, C, N, k, st, pad):
    """test_patch_convs_on_the_split_gemm (test_gpu_round4.py): both arithmetics of the split GEMM in patch mode."""
    x = t4.rnd(B, H, W, C, seed=B + H) * 10.0 ** t4.rnd(B, H, W, C, seed=C, lo=-3, hi=1)
    w = t4.rnd(N, C, k, k, seed=k) * 0.05 * 10.0 ** t4.rnd(N, 1, 1, 1, seed=5, lo=-2, hi=1)
    b = t4.rnd(N, seed=9)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=st, padding=pad).permute(0, 2, 3, 1)
    xc, packs = x.cuda(), ops.pack_sr_conv(w.cuda())

    def err(t):
        return float((t.double().cpu() - ref).abs().max() / ref.abs().max())

    e32 = err(ops.conv2d(xc, packs[0], N, k, stride=st, pad=pad, bias=b.cuda()))
    runs = []
    for _ in range(2):
        y6 = ops.patch_conv_auto(xc, packs, N, k, st, pad, bias=b.cuda())
        guard = ops.Planes16Guard("cuda", B)
        prev = ops.install_guard(guard)
        try:
            y16 = ops.patch_conv_auto(xc, packs, N, k, st, pad, bias=b.cuda())
        finally:
            ops.install_guard(prev)
        runs.append((y6, y16))
    y6, y16 = runs[0]
    errors = {"bf16x6": (err(y6), t4.TOL), "bf16x6 vs fp32 tiles": (err(y6), 8.0 * e32 + 1e-7),
              "f16x3": (err(y16), t4.TOL), "f16x3 vs fp32 tiles": (err(y16), 8.0 * e32 + 1e-7)}
    checks = {"shape": y6.shape == ref.shape, "split image": packs[1] is not None,
              "three kernels": not torch.equal(y16, y6), "range slots": guard.maxima().shape == (1, B)}
    return errors, checks, same(*runs), digest(y6, y16)


def gemm_pairs(M, N, K, tile):
    """test_gemm_pairs_vs_fp64 (test_gpu_round5.py)."""
    x = t5.rnd(M, K, seed=1) * (10.0 ** (t5.rnd(M, 1, seed=2) * 1.5))
    w = t5.rnd(N, K, seed=3) * (10.0 ** (t5.rnd(N, 1, seed=4) * 2.0 - 1.0)) * 0.1
    b, res = t5.rnd(N, seed=5), t5.rnd(M, N, seed=6)
    packs = ops.pack_linear(w.cuda(), half=True)
    checks = {"pairs image": packs[1].pairs is not None}
    with t5.scope(ops, 1) as g:
        xp = ops.pairs_from_f32(x.cuda().view(1, M, K))
        y = ops.linear_pairs(xp, packs, N, bias=b.cuda(), res=res.cuda().view(1, M, N), tile_rows=tile)
        y2 = ops.linear_pairs(xp, packs, N, bias=b.cuda(), res=res.cuda().view(1, M, N), tile_rows=tile)
        back = ops.pairs_to_f32(xp).cpu().view(M, K)
    checks["guard ok"] = not bool(g.tripped().any())
    enc = float(((back.double() - x.double()).abs() / (x.double().abs() + 2.0 ** -14)).max())
    ref = back.double() @ w.double().t() + b.double() + res.double()
    yard = back.double().abs() @ w.double().abs().t() + b.double().abs() + res.double().abs()
    e = float(((y.double().cpu().view(M, N) - ref).abs() / yard).max())
    return {"encoding": (enc, 2.0 ** -21), "conditioning": (e, 2e-6)}, checks, torch.equal(y, y2), digest(y)


def gemm_pairs_patch(B, H, W, C, N, k, st, pad):
    """test_gemm_pairs_patch_mode (test_gpu_round5.py)."""
    x, w, b = t5.rnd(B, H, W, C, seed=21), t5.rnd(N, C, k, k, seed=22) * 0.1, t5.rnd(N, seed=23)
    packs = ops.pack_sr_conv(w.cuda())
    checks = {"pairs image": packs[1] is not None and packs[1].pairs is not None}
    with t5.scope(ops, B):
        xp = ops.pairs_from_f32(x.cuda().view(B, H * W, C))
        y = ops.linear_pairs(ops.Pairs(xp.t.view(B, H, W, C)), packs, N, bias=b.cuda(), patch=(k, st, pad))
        y2 = ops.linear_pairs(ops.Pairs(xp.t.view(B, H, W, C)), packs, N, bias=b.cuda(), patch=(k, st, pad))
        back = ops.pairs_to_f32(xp).cpu().view(B, H, W, C)
    ref = F.conv2d(back.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=st, padding=pad)
    yard = F.conv2d(back.double().abs().permute(0, 3, 1, 2), w.double().abs(), b.double().abs(), stride=st, padding=pad)
    got = y.double().cpu().permute(0, 3, 1, 2)
    checks["shape"] = got.shape == ref.shape
    return {"conditioning": (float(((got - ref).abs() / yard).max()), 2e-6)}, checks, torch.equal(y, y2), digest(y)


def dwconv(gelu, B, H, W, C):
    """test_dwconv_gelu (test_gpu_kernels.py); without the GELU through ops.dwconv3x3_bias, same reference minus the activation."""
    x, w, b = tk.rnd(B, H * W, C, seed=22, lo=-2, hi=2), tk.rnd(C, 1, 3, 3, seed=23), tk.rnd(C, seed=24)
    img = x.double().transpose(1, 2).reshape(B, C, H, W)
    ref = F.conv2d(img, w.double(), b.double(), padding=1, groups=C)
    ref = (F.gelu(ref) if gelu else ref).flatten(2).transpose(1, 2)
    fn = ops.dwconv3x3_gelu if gelu else ops.dwconv3x3_bias
    y = fn(x.cuda(), ops.pack_dw_weight(w.cuda()), b.cuda(), H, W)
    return {"y": (tk.err(y, ref), tk.TOL)}, {}, None, digest(y)


def planes(B, H, W, Cin, d):
    """test_conv3x3_planes_f16x3_four_subtiles (test_gpu_planes16.py) with the planes copy as the only output (no fp32 `out`)."""
    x, w, b = tp.rnd(B, Cin, H, W, seed=13), tp.rnd(32, Cin, 3, 3, seed=14), tp.rnd(32, seed=15)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=d, dilation=d)).permute(0, 2, 3, 1)
    xh = x.permute(0, 2, 3, 1).contiguous().cuda()
    guard = ops.Planes16Guard("cuda")
    pl = ops.Planes(B, H, W, Cin // 16 + 2, "cuda", guard).load_f32(xh)
    ops.conv3x3_planes(pl, Cin, ops.pack_weight_planes16(w.cuda()), dil=d, bias=b.cuda(), act=1, out_chunk0=Cin // 16)
    torch.cuda.synchronize()
    got, raw = tp._decode(pl, Cin // 16, 2)
    mask = torch.ones_like(raw, dtype=torch.bool)
    mask[:, :, 2:2 + H, 2:2 + W] = False
    checks = {"border zero": float(raw[mask].abs().max()) == 0.0, "guard ok": bool(guard.ok()), "finite": bool(torch.isfinite(got).all())}
    return {"planes": (float((got - ref).abs().max() / ref.abs().max()), tp.TOL)}, checks, None, digest(pl.data)


def planes_fused_tail():
    """test_lean_fused_tail_equals_the_general_instantiation (test_gpu_planes16.py), the call that selects the LEAN kernel."""
    B, H, W, Cin = 2, 24, 70, 192
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(B, H, W, Cin, generator=gen) * 2 - 1) * 10.0 ** (torch.rand(B, H, W, Cin, generator=gen) * 4 - 3)
    w, b = tp.rnd(32, Cin, 3, 3, seed=41) * 0.05, tp.rnd(32, seed=42)
    w1, b1 = tp.rnd(64, Cin + 32, seed=43) * 0.1, tp.rnd(64, seed=44)
    guard = ops.Planes16Guard("cuda")
    pl = ops.Planes(B, H, W, Cin // 16 + 2, "cuda", guard).load_f32(x.cuda())
    out = torch.full((B, H, W, 64), 7.0, device="cuda")
    ops.conv3x3_planes(pl, Cin, ops.pack_weight_planes16(w.cuda()), dil=2, bias=b.cuda(), act=1, out_chunk0=None,
                       tail=(ops.pack_weight_planes16(w1.cuda()), b1.cuda(), None, out, 1, True))
    torch.cuda.synchronize()
    xd = x.double().permute(0, 3, 1, 2)
    mid = F.relu(F.conv2d(xd, w.double(), b.double(), padding=2, dilation=2))
    pre = F.conv2d(torch.cat((xd, mid), dim=1), w1.double()[:, :, None, None], b1.double())
    ref = (xd[:, :64] + F.relu(pre)).permute(0, 2, 3, 1)
    return {"out1": (tp.err(out, ref), tp.TOL)}, {"guard ok": bool(guard.ok())}, None, digest(out)


def run(case):
    kind, *rest = case.split("-")
    if kind == "wgrad":
        return wgrad(*rest)
    if kind == "dwconv":
        return dwconv(rest[0] == "gelu", *map(int, rest[1].split("x")))
    if kind == "planes":
        return planes_fused_tail() if rest[0].startswith("fused_tail") else planes(*map(int, rest[0].split("x")), int(rest[1][1:]))
    if rest[0] == "patch":  # <B x H x W x C>-<N>-k<k>s<stride>p<pad>
        geom = [int(v) for v in rest[1].split("x")] + [int(rest[2])] + [int(rest[3][i]) for i in (1, 3, 5)]
        return (gemm_split_patch if kind == "gemm_split" else gemm_pairs_patch)(*geom)
    if kind == "gemm_split":
        return gemm_split(rest[0], *map(int, rest[1].split("x")))
    if kind == "gemm_pairs":
        return gemm_pairs(*map(int, rest[0].split("x")), int(rest[1][1:]))
    raise KeyError(case)


def main(group, out_path):
    env = {k: v for k, v in os.environ.items() if k in {n for _, e, *_ in tv.VARIANTS for n in e}}
    records = []
    for case in tv.group_cases(group):
        torch.cuda.synchronize()
        print(tv.BEGIN + case, file=sys.stderr, flush=True)
        t0 = time.time()
        rec = {"case": case, "errors": {}, "checks": {}, "deterministic": None, "hash": None}
        try:
            errors, checks, det, h = run(case)
            rec.update(errors={k: [float(v), float(bd)] for k, (v, bd) in errors.items()}, checks={k: bool(v) for k, v in checks.items()},
                       deterministic=None if det is None else bool(det), hash=h)
            torch.cuda.synchronize()
        except Exception:  # a HIP error among them: nothing more is started on the device, the child ends with a status of its own
            rec["exception"] = traceback.format_exc()
            print(f"{case}:\n{rec['exception']}", flush=True)
        rec["seconds"] = round(time.time() - t0, 3)
        # only the switches that bear on this case's kernel: what the parent's row states
        rows = [e for g, e, c, *_ in tv.VARIANTS if g == group and c == case]
        rec["env"] = {k: env.get(k) for e in rows for k in e}
        print(tv.END + case, file=sys.stderr, flush=True)
        records.append(rec)
        with open(out_path + ".tmp", "w") as f:
            json.dump(records, f, indent=1)
        os.replace(out_path + ".tmp", out_path)
        if "exception" in rec:
            sys.exit(3)
    print(json.dumps({"group": group, "cases": len(records), "seconds": round(sum(r["seconds"] for r in records), 2)}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
