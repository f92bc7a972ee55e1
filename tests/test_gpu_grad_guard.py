"""GPU tests of the guarded optimizer step (csrc/grad_guard.hip, utils/optimizer.py): the device-side gradient norm, clipping
against a float64 restatement of torch's AdamW + clip_grad_norm_, "off means off", skip-on-non-finite, the stand-alone
clip_grad_norm_, the state_dict round trip and the graphed segmentation step with a guarded optimizer.

The accuracy gate is not a constant: torch's own float32 AdamW with clip_grad_norm_ runs the same recipe (on the CPU) against
the float64 restatement, the guarded path is allowed four times that error (the margin of the TTA test), and the measured
yardstick must itself stay below 5e-6 so that a broken yardstick cannot widen the gate."""
import copy
import ctypes
import functools
import math

import pytest
import torch

import detweights as dw

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (128,), (32, 16, 3, 3), (1,), (255,), (257,), (65536,), (65537,), (100000,)]
LATE = 3            # index of the (1,) parameter: no gradient in steps 0 and 1
STEPS, LOUD, BAD_STEP = 6, 2, 3
YARDSTICK_MAX = 5e-6
INF = float("inf")


@pytest.fixture(scope="module")
def opt_mod():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd.utils import optimizer
    return optimizer


@functools.lru_cache(maxsize=None)
def recipe():
    """(initial parameters, gradients[step][i] or None) on the CPU, float32, seeded; computed once and never changed"""
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=g) for s in SHAPES]
    grads = []
    for it in range(STEPS):
        row = []
        for i, s in enumerate(SHAPES):
            x = torch.randn(s, generator=g) * (100.0 if it == LOUD else 1.0)
            row.append(None if (i == LATE and it < 2) else x)
        grads.append(row)
    return params, grads


def groups(ps):
    return [{"params": ps[:2], "lr": 1e-3, "weight_decay": 0.01}, {"params": ps[2:], "lr": 1e-2, "weight_decay": 0.0}]


def norm64(row):
    return math.sqrt(sum(float((x.double() ** 2).sum()) for x in row if x is not None))


@functools.lru_cache(maxsize=None)
def reference(max_norm, leave_out):
    """(float64 restatement, torch float32 AdamW + clip_grad_norm_) final parameters on the CPU for the recipe, with step
    `leave_out` (or None) left out entirely."""
    params, grads = recipe()
    p64 = [p.double().clone().requires_grad_(True) for p in params]
    p32 = [p.clone().requires_grad_(True) for p in params]
    o64 = torch.optim.AdamW(groups(p64), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    o32 = torch.optim.AdamW(groups(p32), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for it, row in enumerate(grads):
        if it == leave_out:
            continue
        coef = min(1.0, max_norm / (norm64(row) + 1e-6))
        for a, b, x in zip(p64, p32, row):
            a.grad = None if x is None else x.double() * coef
            b.grad = None if x is None else x.clone()
        if max_norm != INF:
            torch.nn.utils.clip_grad_norm_(p32, max_norm)
        o64.step()
        o32.step()
    return [p.detach() for p in p64], [p.detach() for p in p32]


def err(got, ref):
    """test_gpu_backward.err over a list: per parameter max |got - ref| / max |ref|, the largest of them"""
    worst = 0.0
    for a, b in zip(got, ref):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        assert a.shape == b.shape and torch.isfinite(a).all()
        worst = max(worst, float((a - b).abs().max() / (b.abs().max() + 1e-30)))
    return worst


def gate(max_norm, leave_out=None):
    """(float64 parameters, 4 x the measured error of torch's float32 path)"""
    p64, p32 = reference(max_norm, leave_out)
    yard = err(p32, p64)
    print(f"yardstick max_norm={max_norm} leave_out={leave_out}: torch float32 vs float64 {yard:.3e}")
    assert 0.0 < yard < YARDSTICK_MAX, yard
    return p64, 4.0 * yard


def run(opt_mod, max_grad_norm=None, skip_nonfinite=False, poison=None, each_step=None, plain=False):
    """the recipe on the device; poison = (parameter index, flat element, value) written into step BAD_STEP's gradient"""
    params, grads = recipe()
    ps = [p.clone().cuda().requires_grad_(True) for p in params]
    kw = {} if plain else dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    opt = opt_mod.FusedAdamW(groups(ps), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, **kw)
    for it, row in enumerate(grads):
        for i, (p, x) in enumerate(zip(ps, row)):
            p.grad = None if x is None else x.clone().cuda()
            if poison is not None and it == BAD_STEP and i == poison[0]:
                p.grad.view(-1)[poison[1]] = poison[2]
        if each_step is not None:
            each_step(it, opt, ps, before=True)
        opt.step()
        if each_step is not None:
            each_step(it, opt, ps, before=False)
    return ps, opt


def entry_of(stats, p):
    """the per_param entry of parameter p (table order follows the hyper-parameter groups, not the recipe's order)"""
    (e,) = [e for e in stats["per_param"] if e["param"] is p]
    return e


def test_norm_record_per_entry_and_reproducible(opt_mod):
    """record.sumsq against the float64 sum of squares within n 2^-52 relative (the squares are exact, the additions round), norm
    within 2^-23, the same per entry; two calls on one table give bitwise-equal records."""
    from segmif_amd import _lib
    _, grads = recipe()
    seen = {}

    def look(it, opt, ps, before):
        if not before and it in (0, LOUD, STEPS - 1):
            seen[it] = (opt.grad_stats(), ps)

    run(opt_mod, max_grad_norm=INF, each_step=look)
    for it, (st, ps) in seen.items():
        row = [x for x in grads[it] if x is not None]
        n = sum(x.numel() for x in row)
        ref = sum(float((x.double() ** 2).sum()) for x in row)
        print(f"step {it}: norm {st['norm']:.6f} sumsq rel err {abs(st['sumsq'] - ref) / ref:.3e}")
        assert abs(st["sumsq"] - ref) <= n * 2.0 ** -52 * ref
        assert abs(st["norm"] - math.sqrt(ref)) <= 2.0 ** -23 * math.sqrt(ref)
        assert st["nonfinite"] == 0 and st["coef"] == 1.0 and len(st["per_param"]) == len(row)
        for p, x in zip(ps, grads[it]):
            if x is None:
                assert not [e for e in st["per_param"] if e["param"] is p]
                continue
            e, r = entry_of(st, p), float((x.double() ** 2).sum())
            assert abs(e["sumsq"] - r) <= x.numel() * 2.0 ** -52 * r and e["nonfinite"] == 0
            assert abs(e["norm"] - math.sqrt(r)) <= 2.0 ** -23 * math.sqrt(r)
    assert 480 < seen[0][0]["norm"] < 500 and 48000 < seen[LOUD][0]["norm"] < 50000
    # the entry point itself, twice on one table
    lib = _lib.load()
    gs = [x.clone().cuda() for x in grads[LOUD]]
    blob, (o_co, o_ce, _), nchunks = opt_mod._upload_table([(g, g, None, None, 0.0, 0.0) for g in gs], None, gs[0].device)
    assert nchunks == 11
    o_ent = ctypes.sizeof(_lib.SegmifGradGuardRecord)
    work = torch.empty(lib.segmif_grad_norm_workspace_bytes(nchunks), dtype=torch.uint8, device="cuda")
    outs, stream = [], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        buf = torch.zeros(o_ent + 16 * len(gs), dtype=torch.uint8, device="cuda")
        work.fill_(0xA5)
        base = blob.data_ptr()
        assert lib.segmif_grad_norm_f32(base, len(gs), base + o_ce, base + o_co, nchunks, 65536, work.data_ptr(), buf.data_ptr() + o_ent,
                                        buf.data_ptr(), None, None, 1.0, 0, stream) == 0
        outs.append(buf.cpu())
    assert torch.equal(outs[0], outs[1])
    rec = _lib.SegmifGradGuardRecord.from_buffer_copy(outs[0].numpy().tobytes()[:o_ent])
    assert rec.attempts == 1 and rec.applied == 1 and rec.clipped == 1 and rec.skipped == 0 and 0.0 < rec.coef < 1e-4


@pytest.mark.parametrize("max_norm,clipped", [(1.0, 6), (500.0, 1), (INF, 0)])
def test_clipping_against_float64_restatement(opt_mod, max_norm, clipped):
    """max_norm 1 clips every step, 500 only the loud one, inf none.  Measured on the MI355X (guarded | torch float32 yardstick):
    see profiles/guarded_step_bench.txt."""
    p64, bound = gate(max_norm)
    ps, opt = run(opt_mod, max_grad_norm=max_norm)
    e = err(ps, p64)
    print(f"guarded max_norm={max_norm}: vs float64 {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (e, bound)
    st = opt.grad_stats()
    assert st["clipped"] == clipped and st["attempts"] == STEPS and st["applied"] == STEPS and st["skipped"] == 0


def test_off_means_off(opt_mod):
    """max_norm = inf and no skipping on finite gradients: the plain FusedAdamW's result within the same bound (not bitwise: the
    guarded kernel forms the bias corrections on the device)."""
    _, bound = gate(INF)
    guarded, _ = run(opt_mod, max_grad_norm=INF, skip_nonfinite=False)
    plain, opt = run(opt_mod, plain=True)
    e = err(guarded, plain)
    print(f"guarded (inf, no skip) vs plain FusedAdamW {e:.3e} (bound {bound:.3e})")
    assert e <= bound
    with pytest.raises(RuntimeError):
        opt.grad_stats()  # a plain optimizer has no guard to report


@pytest.mark.parametrize("poison", [(7, 65536, float("nan")), (LATE, 0, INF), (0, 0, -INF)],
                         ids=["nan_last_of_65537", "inf_in_1", "neginf_first_of_64x64"])
def test_skip_nonfinite(opt_mod, poison):
    """One non-finite element at step 3: that step changes no p, exp_avg or exp_avg_sq; the run ends where the float64
    restatement WITHOUT step 3 ends (bias corrections over five steps); without the guard the parameters end non-finite."""
    snap, stats = {}, {}

    def watch(it, opt, ps, before):
        if it != BAD_STEP:
            return
        state = [t for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
        if before:
            snap["before"] = [t.detach().clone() for t in state]
        else:
            assert all(torch.equal(a, b) for a, b in zip(snap["before"], state))
            stats["bad"], stats["ps"] = opt.grad_stats(), ps

    p64, bound = gate(INF, leave_out=BAD_STEP)
    ps, opt = run(opt_mod, skip_nonfinite=True, poison=poison, each_step=watch)
    bad = stats["bad"]
    assert bad["skip_now"] and bad["nonfinite"] == 1 and bad["skipped"] == 1 and bad["consecutive_skips"] == 1
    assert [entry_of(bad, p)["nonfinite"] for p in stats["ps"]] == [int(i == poison[0]) for i in range(len(SHAPES))]
    assert [entry_of(bad, p)["offended_steps"] for p in stats["ps"]] == [int(i == poison[0]) for i in range(len(SHAPES))]
    st = opt.grad_stats()
    assert st["skipped"] == 1 and st["applied"] == STEPS - 1 and st["attempts"] == STEPS and st["consecutive_skips"] == 0
    e = err(ps, p64)
    print(f"skip {poison}: vs float64 without step {BAD_STEP} {e:.3e} (bound {bound:.3e})")
    assert e <= bound
    plain, _ = run(opt_mod, plain=True, poison=poison)
    assert not all(bool(torch.isfinite(p).all()) for p in plain)  # the guard is what made the difference


def test_a_parameter_that_sat_out_the_skipped_step_keeps_its_own_count(opt_mod):
    """Bias correction counts the applied steps of EACH parameter: b has no gradient in the step that a's NaN gets skipped, so
    b's two attempts are two applied steps (a global count of skipped steps would give it one).  Float64 AdamW that never sees
    step 1 is the reference; the bound is 4 x torch's float32 error on the same three-step recipe."""
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(300, generator=g), torch.randn(70, generator=g)]
    grads = [[torch.randn(300, generator=g), torch.randn(70, generator=g)], [torch.randn(300, generator=g), None],
             [torch.randn(300, generator=g), torch.randn(70, generator=g)]]
    ends = []
    for dtype in (torch.float64, torch.float32):
        ps = [p.to(dtype).clone().requires_grad_(True) for p in init]
        opt = torch.optim.AdamW(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        for it in (0, 2):
            for p, x in zip(ps, grads[it]):
                p.grad = x.to(dtype)
            opt.step()
        ends.append([p.detach() for p in ps])
    yard = err(ends[1], ends[0])
    assert 0.0 < yard < YARDSTICK_MAX
    ps = [p.clone().cuda().requires_grad_(True) for p in init]
    opt = opt_mod.FusedAdamW(ps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, skip_nonfinite=True)
    for it in range(3):
        for p, x in zip(ps, grads[it]):
            p.grad = None if x is None else x.clone().cuda()
        if it == 1:
            ps[0].grad[17] = float("nan")
        opt.step()
    e = err(ps, ends[0])
    print(f"sat-out parameter: vs float64 {e:.3e} (bound {4 * yard:.3e})")
    assert e <= 4 * yard
    sd = opt.state_dict()
    assert [sd["state"][k]["step"] for k in (0, 1)] == [2, 2] and sd["grad_guard"]["skipped"] == 1


def test_standalone_clip_grad_norm(opt_mod):
    """clip_grad_norm_ against torch's on the same tensors: the norm within 2^-22 relative, the gradients within 2 float ulps;
    a coefficient of 1 leaves them bitwise alone; error_if_nonfinite raises on a NaN."""
    _, grads = recipe()
    for max_norm in (1.0, 1e6):
        a = [torch.zeros(s, device="cuda").requires_grad_(True) for s in SHAPES]
        b = [torch.zeros(s, device="cuda").requires_grad_(True) for s in SHAPES]
        for x, y, g in zip(a, b, grads[STEPS - 1]):
            x.grad, y.grad = g.clone().cuda(), g.clone().cuda()
        got = opt_mod.clip_grad_norm_(a, max_norm)
        want = torch.nn.utils.clip_grad_norm_(b, max_norm)
        assert got.is_cuda and got.dim() == 0
        assert abs(float(got) - float(want)) <= 2.0 ** -22 * float(want)
        for x, y, g in zip(a, b, grads[STEPS - 1]):
            ulp = torch.nextafter(y.grad.abs(), torch.full_like(y.grad, INF)) - y.grad.abs()
            assert bool(((x.grad - y.grad).abs() <= 2 * ulp).all())
            if max_norm == 1e6:
                assert torch.equal(x.grad.cpu(), g)
    a[7].grad.view(-1)[65536] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        opt_mod.clip_grad_norm_(a, 1.0, error_if_nonfinite=True)
    assert math.isnan(float(opt_mod.clip_grad_norm_(a, 1.0)))


def test_state_dict_round_trip(opt_mod):
    """Six steps with one skipped, state_dict() into a fresh guarded optimizer over cloned parameters: the stored step is 5 (applied
    steps: torch.optim.AdamW can load it), the counters travel, and one more step on both gives bitwise-equal parameters."""
    ps, opt = run(opt_mod, max_grad_norm=500.0, skip_nonfinite=True, poison=(7, 65536, float("nan")))
    sd = copy.deepcopy(opt.state_dict())
    assert all(v["step"] == (5 if k != LATE else 3) for k, v in sd["state"].items()) and len(sd["state"]) == len(SHAPES)
    assert sd["grad_guard"] == dict(attempts=6, applied=5, skipped=1, clipped=1, consecutive_skips=0)
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    opt2 = opt_mod.FusedAdamW(groups(qs), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=500.0,
                              skip_nonfinite=True)
    opt2.load_state_dict(sd)
    assert opt2.grad_stats()["skipped"] == 1
    g = torch.Generator().manual_seed(99)
    for p, q in zip(ps, qs):
        x = torch.randn(p.shape, generator=g).cuda()
        p.grad, q.grad = x.clone(), x.clone()
    opt.step()
    opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    st = opt2.grad_stats()
    assert st["attempts"] == 7 and st["applied"] == 6 and st["skipped"] == 1
    t = [torch.nn.Parameter(p.detach().clone()) for p in ps]  # torch's optimizer accepts the dictionary
    torch.optim.AdamW(groups(t), lr=1e-3).load_state_dict(copy.deepcopy(opt.state_dict()))


def test_graphed_seg_step_with_a_guarded_optimizer():
    """test_gpu_round3's graphed-step configuration (mit_b1, 2 x 64 x 96, eval-mode regime) with a guarded optimizer whose
    max_grad_norm lies below the gradient norm: three GraphedSegTrainStep steps equal three eager ones bitwise - the optimizer
    stays outside the graph and works unchanged - and all three are clipped."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core as core
    from segmif_amd.train import GraphedSegTrainStep, seg_train_step
    from segmif_amd.utils.optimizer import PolyWarmupAdamW_seg
    max_norm = 0.05

    def make():
        net = core.Network3("mit_b1", 9, pretrained=None)
        dw.load_det_weights(net, seed=0)
        net = net.cuda().eval()
        g = net.denoise_net.get_param_groups()
        opt = PolyWarmupAdamW_seg([{"params": g[0], "lr": 8e-5, "weight_decay": 0.01}, {"params": g[1], "lr": 8e-5, "weight_decay": 0.0},
                                   {"params": g[2], "lr": 8e-4, "weight_decay": 0.01}], lr=8e-5, weight_decay=0.01, betas=(0.9, 0.999),
                                  iter_curr=10000, warmup_iter=3000, max_iter=160000, warmup_ratio=1e-6, power=1.0,
                                  max_grad_norm=max_norm, skip_nonfinite=True)
        return net, opt

    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    B, H, W = 2, 64, 96
    xs = [dw.det_input(f"gs_x{i}", (B, 3, H, W)).cuda() for i in range(3)]
    ys = [dw.det_labels(f"gs_y{i}", (B, H, W), 9).cuda() for i in range(3)]
    net_e, opt_e = make()
    losses_e = [float(seg_train_step(net_e, opt_e, x, y, crit)) for x, y in zip(xs, ys)]
    net_g, opt_g = make()
    step = GraphedSegTrainStep(net_g, opt_g, crit, xs[0], ys[0], warmup=1)
    losses_g = [float(step(x, y)) for x, y in zip(xs, ys)]
    assert losses_g == losses_e, (losses_g, losses_e)
    for (n, a), (_, b) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(a, b), n
    se, sg = opt_e.grad_stats(), opt_g.grad_stats()
    print(f"seg step gradient norm {se['norm']:.4f} (max_grad_norm {max_norm})")
    assert se["norm"] > max_norm and se["norm"] == sg["norm"]
    assert se["clipped"] == 3 and sg["clipped"] == 3 and se["skipped"] == 0 and sg["skipped"] == 0
