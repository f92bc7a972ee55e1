"""GPU tests of the weight average (csrc/weight_ema.hip, utils/optimizer.py): the pair hi + lo against a float64 recurrence, "on
changes nothing else", a skipped step, a long run of steps too small for a float32 average, the swap context, the state_dict
round trip and an eval forward of the real segmentation net under the averaged weights.

The yardstick is the float64 recurrence ref += (1 - d_t) * (p - ref) on the CPU, fed the DEVICE's own p read back after every
step (so the AdamW trajectory's float32 error is not in the comparison), with d_t = ema_decay_at(decay, warmup, t) and t the
parameter's own count of applied steps.  The gate per parameter over its T updates:
    |(hi + lo) - ref| <= T * 2^-47 * max |ref|                        |hi - ref| <= 2^-24 |ref| + T * 2^-47 * max |ref|
Each update rounds the pair once, to within 2^-48 of its value (lo keeps 24 bits below hi's 24, and hi + lo is exact in double);
the bound takes twice that per step; hi is the float32 rounding of the pair.  The naive float32 recurrence misses the first gate
by orders of magnitude (test_long_run_of_small_steps_does_not_stall asserts that)."""
import copy
import functools

import pytest
import torch

import detweights as dw

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (128,), (32, 16, 3, 3), (1,), (255,), (257,), (65536,), (65537,), (100000,)]
LATE = 3            # index of the (1,) parameter: no gradient in steps 0 and 1
STEPS, LOUD, BAD_STEP = 6, 2, 3
PAIR_STEP = 2.0 ** -47
CONFIGS = [(0.9999, False), (0.999, True)]
GUARDS = {"plain": {}, "guarded": dict(max_grad_norm=1.0)}


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


def make(opt_mod, ps, **kw):
    return opt_mod.FusedAdamW(groups(ps), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, **kw)


def run(opt_mod, steps=range(STEPS), ps=None, opt=None, poison=None, each_step=None, **kw):
    """steps of the recipe on the device; poison = (parameter index, flat element, value) written into step BAD_STEP's gradient"""
    params, grads = recipe()
    if ps is None:
        ps = [p.clone().cuda().requires_grad_(True) for p in params]
    if opt is None:
        opt = make(opt_mod, ps, **kw)
    for it in steps:
        for i, (p, x) in enumerate(zip(ps, grads[it])):
            p.grad = None if x is None else x.clone().cuda()
            if poison is not None and it == BAD_STEP and i == poison[0]:
                p.grad.view(-1)[poison[1]] = poison[2]
        if each_step is not None:
            each_step(it, opt, ps, before=True)
        opt.step()
        if each_step is not None:
            each_step(it, opt, ps, before=False)
    return ps, opt


class Recurrence:
    """the float64 yardstick of one run: advance(it, ps) after every APPLIED step, with the device's own parameters"""

    def __init__(self, opt_mod, decay, warmup):
        params, self.grads = recipe()
        self.decay_at = functools.partial(opt_mod.ema_decay_at, decay, warmup)
        self.ref = [p.double().clone() for p in params]  # an average starts at the value before the parameter's first update
        self.t = [0] * len(params)

    def advance(self, it, ps):
        for i, p in enumerate(ps):
            if self.grads[it][i] is None:
                continue
            self.t[i] += 1
            self.ref[i] += (1.0 - self.decay_at(self.t[i])) * (p.detach().cpu().double() - self.ref[i])

    def check(self, opt, ps, what):
        avg = opt.ema_tensors()
        assert len(avg) == len(ps)
        worst = 0.0
        for i, p in enumerate(ps):
            check_pair(avg[p][0], avg[p][1], self.ref[i], self.t[i], f"{what} parameter {i} {SHAPES[i]}")
            worst = max(worst, pair_error(avg[p][0], avg[p][1], self.ref[i]))
        return worst


def pair_error(hi, lo, ref):
    return float(((hi.detach().cpu().double() + lo.detach().cpu().double()) - ref).abs().max() / ref.abs().max())


def check_pair(hi, lo, ref, T, what):
    """the two gates of the module docstring; prints the figures first"""
    hi, lo = hi.detach().cpu().double(), lo.detach().cpu().double()
    assert hi.shape == ref.shape and torch.isfinite(hi).all() and torch.isfinite(lo).all()
    scale = float(ref.abs().max())
    e_pair = float(((hi + lo) - ref).abs().max())
    e_hi = float(((hi - ref).abs() - 2.0 ** -24 * ref.abs()).max())
    print(f"{what}: T {T} pair {e_pair / scale:.3e} (bound {T * PAIR_STEP:.3e}) hi {float((hi - ref).abs().max()) / scale:.3e}")
    assert e_pair <= T * PAIR_STEP * scale, (what, e_pair / scale)
    assert e_hi <= T * PAIR_STEP * scale, (what, e_hi / scale)


@pytest.mark.parametrize("guard", list(GUARDS))
@pytest.mark.parametrize("decay,warmup", CONFIGS)
def test_average_matches_the_float64_recurrence(opt_mod, decay, warmup, guard):
    """Six steps, two groups, one loud step; the late parameter's average begins at its first gradient (step 2) and counts its own
    t: with warm-up its first decay is 2 / 11, which a shared count (4 / 13) would miss by far."""
    yard = Recurrence(opt_mod, decay, warmup)

    def watch(it, opt, ps, before):
        if before:
            return
        yard.advance(it, ps)
        assert (ps[LATE] in opt.ema_tensors()) == (it >= 2)
        if it == 2:  # its first update, from its untouched initial value
            hi, lo = opt.ema_tensors()[ps[LATE]]
            p0 = recipe()[0][LATE].double()
            want = p0 + (1.0 - opt_mod.ema_decay_at(decay, warmup, 1)) * (ps[LATE].detach().cpu().double() - p0)
            check_pair(hi, lo, want, 1, "late parameter, first update")

    ps, opt = run(opt_mod, each_step=watch, ema_decay=decay, ema_warmup=warmup, **GUARDS[guard])
    assert yard.t == [STEPS if i != LATE else STEPS - 2 for i in range(len(SHAPES))]
    worst = yard.check(opt, ps, f"{guard} d={decay} warmup={warmup}")
    print(f"{guard} d={decay} warmup={warmup}: worst pair error {worst:.3e}")
    for p in ps:  # the pair is normalised: lo is the remainder below hi's last bit
        hi, lo = opt.ema_tensors()[p]
        assert bool((lo.abs() <= 2.0 ** -24 * hi.abs() + 1e-45).all())


@pytest.mark.parametrize("guard", list(GUARDS))
def test_average_on_changes_nothing_else(opt_mod, guard):
    """p, exp_avg and exp_avg_sq after the six steps are bit-equal with the average on and off; off, no state holds an `ema` key."""
    on_ps, on = run(opt_mod, ema_decay=0.999, ema_warmup=True, **GUARDS[guard])
    off_ps, off = run(opt_mod, **GUARDS[guard])
    for a, b in zip(on_ps, off_ps):
        assert torch.equal(a, b)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(on.state[a][k], off.state[b][k])
        assert on.state[a]["step"] == off.state[b]["step"]
        assert set(off.state[b]) == {"step", "exp_avg", "exp_avg_sq"} and set(on.state[a]) == {"step", "exp_avg", "exp_avg_sq", "ema", "ema_lo"}
    assert set(off.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    with pytest.raises(RuntimeError):
        off.ema_tensors()


def test_skipped_step_leaves_the_average_alone(opt_mod):
    """skip_nonfinite with warm-up (so that a wrong t shows): a NaN in one gradient of step 3 - hi and lo of EVERY parameter are
    bit-equal before and after that step, and the final pair meets the gate against the recurrence that never saw step 3."""
    decay, warmup = 0.999, True
    yard = Recurrence(opt_mod, decay, warmup)
    snap = {}

    def watch(it, opt, ps, before):
        if it != BAD_STEP:
            if not before:
                yard.advance(it, ps)
            return
        pairs = [t for p in ps for t in opt.ema_tensors()[p]]
        if before:
            snap["before"] = [t.clone() for t in pairs]
        else:
            assert len(pairs) == 2 * len(SHAPES) and all(torch.equal(a, b) for a, b in zip(snap["before"], pairs))
            assert opt.grad_stats()["skip_now"]

    ps, opt = run(opt_mod, each_step=watch, poison=(7, 65536, float("nan")), skip_nonfinite=True, ema_decay=decay, ema_warmup=warmup)
    st = opt.grad_stats()
    assert st["skipped"] == 1 and st["applied"] == STEPS - 1
    assert yard.t == [STEPS - 1 if i != LATE else STEPS - 3 for i in range(len(SHAPES))]
    worst = yard.check(opt, ps, "skipped step 3")
    print(f"skipped step: worst pair error {worst:.3e}")


def test_long_run_of_small_steps_does_not_stall(opt_mod):
    """The stand-alone WeightEMA over one tensor of 4099 elements, d = 0.9999, 300 updates whose increments (8e-5 and falling) lie
    at or under half an ulp of a float32 average.  The pair meets the gate (T = 300: 2.1e-12); the naive float32 recurrence on
    the CPU over the same sequence misses it by more than 100 x - a gate that could not tell a stalled average from a working
    one would fail there.  CPU emulation of the pair: 1.9e-14; naive float32: 6.3e-6."""
    n, T, decay = 4099, 300, 0.9999
    g = torch.Generator().manual_seed(7)
    seq = [torch.randn(n, generator=g)]
    for t in range(1, T + 1):
        s = torch.sign(torch.randn(n, generator=g)).double()
        seq.append((seq[-1].double() + 8e-5 * (1.0 - t / T) * s).float())
    ref, naive = seq[0].double().clone(), seq[0].clone()
    for t in range(1, T + 1):
        ref += (1.0 - decay) * (seq[t].double() - ref)
        naive += torch.tensor(1.0 - decay, dtype=torch.float32) * (seq[t] - naive)
    dev = torch.stack(seq).cuda()
    p = torch.nn.Parameter(dev[0].clone())
    ema = opt_mod.WeightEMA([p], decay)
    with torch.no_grad():
        for t in range(1, T + 1):
            p.copy_(dev[t])
            ema.update()
    assert ema.step == T
    hi, lo = ema.ema_tensors()[p]
    check_pair(hi, lo, ref, T, "300 small steps")
    gate = T * PAIR_STEP
    e_naive = float((naive.double() - ref).abs().max() / ref.abs().max())
    print(f"naive float32 recurrence: {e_naive:.3e} ({e_naive / gate:.1e} x the gate {gate:.3e}); "
          f"hi == float32(ref) in {int((hi.cpu() == ref.float()).sum())} of {n} elements")
    assert e_naive > 100.0 * gate


def test_swap_context_and_state_dict(opt_mod):
    """A Linear, a BatchNorm1d and a parameter that never gets a gradient, three steps: inside ema_weights the averaged parameters
    are bit-equal to hi with a grown _version, buffers and the gradient-less parameter untouched; after the block, and after a
    block that raises, the raw values are back bit for bit; ema_state_dict has the module's keys and leaves the module alone."""
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3)).cuda()
    net.idle = torch.nn.Parameter(torch.randn(5, device="cuda"))
    opt = opt_mod.FusedAdamW(net.parameters(), lr=1e-2, ema_decay=0.9)
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(8, 4, generator=g).cuda(), torch.randn(8, 3, generator=g).cuda()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        ((net(x) - y) ** 2).sum().backward()
        opt.step()
    avg = opt.ema_tensors()
    named = dict(net.named_parameters())
    averaged = {n for n, p in named.items() if p in avg}
    assert averaged == {"0.weight", "0.bias", "1.weight", "1.bias"} and "idle" in named and net.idle.grad is None
    raw = {n: p.detach().clone() for n, p in named.items()}
    buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
    pointers = {n: p.data_ptr() for n, p in named.items()}
    versions = {n: p._version for n, p in named.items()}
    assert any(not torch.equal(avg[named[n]][0], raw[n]) for n in averaged)  # the average is not the raw weight

    def check_inside():
        for n, p in named.items():
            if n in averaged:
                assert torch.equal(p, avg[p][0]) and p._version > versions[n]
            else:
                assert torch.equal(p, raw[n]) and p._version == versions[n]
            assert p.data_ptr() == pointers[n]
        assert all(torch.equal(b, buffers[n]) for n, b in net.named_buffers())

    def check_restored():
        for n, p in named.items():
            assert torch.equal(p, raw[n]) and p.data_ptr() == pointers[n]
        assert all(torch.equal(b, buffers[n]) for n, b in net.named_buffers())

    with opt_mod.ema_weights(opt, net):
        check_inside()
        inside_versions = {n: p._version for n, p in named.items()}
    check_restored()
    assert all(named[n]._version > inside_versions[n] for n in averaged)  # the copy back is seen by the caches as well
    with pytest.raises(KeyError, match="boom"):
        with opt_mod.ema_weights(opt, net):
            check_inside()
            raise KeyError("boom")
    check_restored()
    sd = opt_mod.ema_state_dict(opt, net)
    assert list(sd) == list(net.state_dict())
    for k, v in net.state_dict().items():
        want = avg[named[k]][0] if k in averaged else v
        assert torch.equal(sd[k], want) and sd[k].data_ptr() not in (v.data_ptr(), want.data_ptr())
    check_restored()


@pytest.mark.parametrize("guard", list(GUARDS))
def test_state_dict_round_trip(opt_mod, guard):
    """Three steps, state_dict() into a fresh optimizer over cloned parameters, three more: hi and lo bit-equal to six uninterrupted
    steps.  A dict written WITHOUT the average, loaded into an optimizer with it, starts the average from the current p at the next
    step, with the loaded step count as t.  torch.optim.AdamW loads the dict with the average in it."""
    kw = dict(ema_decay=0.999, ema_warmup=True, **GUARDS[guard])
    whole_ps, whole = run(opt_mod, **kw)
    first_ps, first = run(opt_mod, steps=range(3), **kw)
    sd = copy.deepcopy(first.state_dict())
    assert all({"ema", "ema_lo"} <= set(v) for v in sd["state"].values()) and len(sd["state"]) == len(SHAPES)
    qs = [p.detach().clone().requires_grad_(True) for p in first_ps]
    second = make(opt_mod, qs, **kw)
    second.load_state_dict(sd)
    run(opt_mod, steps=range(3, STEPS), ps=qs, opt=second)
    for p, q in zip(whole_ps, qs):
        assert torch.equal(p, q)
        for a, b in zip(whole.ema_tensors()[p], second.ema_tensors()[q]):
            assert torch.equal(a, b)
    # written without the average, loaded with it
    off_ps, off = run(opt_mod, steps=range(3), **GUARDS[guard])
    sd_off = copy.deepcopy(off.state_dict())
    assert not any("ema" in v for v in sd_off["state"].values())
    rs = [p.detach().clone().requires_grad_(True) for p in off_ps]
    late = make(opt_mod, rs, **kw)
    late.load_state_dict(sd_off)
    assert late.ema_tensors() == {}
    before = [r.detach().cpu().double() for r in rs]
    run(opt_mod, steps=range(3, 4), ps=rs, opt=late)
    for i, (r, b) in enumerate(zip(rs, before)):
        t = sd_off["state"][i]["step"] + 1
        want = b + (1.0 - opt_mod.ema_decay_at(0.999, True, t)) * (r.detach().cpu().double() - b)
        check_pair(*late.ema_tensors()[r], want, 1, f"average begun after a load, parameter {i} (t = {t})")
    t = [torch.nn.Parameter(p.detach().clone()) for p in whole_ps]  # torch's optimizer accepts the dictionary
    torch.optim.AdamW(groups(t), lr=1e-3).load_state_dict(copy.deepcopy(whole.state_dict()))


def test_eval_forward_under_the_average_uses_the_averaged_weights():
    """Network3('mit_b1', 9) on 2 x 64 x 96, two seg_train_steps with make_seg_optimizer(ema_decay=0.9): predict_labels and the
    logits inside ema_weights(opt, net) are bit-equal to those of a deep copy of the net that loaded ema_state_dict(opt, net) -
    the PackedCache invalidation (packed weights, folded BatchNorm, fused head matrices) through the real modules - and after
    the block the net's forward is bit-equal to its forward before the block."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import segmif_amd.core as core
    from segmif_amd.train import make_seg_optimizer, seg_train_step
    from segmif_amd.utils.optimizer import ema_state_dict, ema_weights
    net = core.Network3("mit_b1", 9, pretrained=None)
    dw.load_det_weights(net, seed=0)
    net = net.cuda().eval()
    opt = make_seg_optimizer(net, iter_curr=10000, ema_decay=0.9)  # (past the warm-up: a learning rate that moves the weights)
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    B, H, W = 2, 64, 96
    for i in range(2):
        seg_train_step(net, opt, dw.det_input(f"ema_x{i}", (B, 3, H, W)).cuda(), dw.det_labels(f"ema_y{i}", (B, H, W), 9).cuda(), crit)
    x = dw.det_input("ema_eval", (B, 3, H, W)).cuda()
    avg = opt.ema_tensors()
    assert avg and any(not torch.equal(p, hi) for p, (hi, _) in avg.items())
    with torch.no_grad():
        before = net(x)[2].clone()
        before_labels = net.predict_labels(x).clone()
        with ema_weights(opt, net):
            inside = net(x)[2].clone()
            inside_labels = net.predict_labels(x).clone()
        after = net(x)[2].clone()
        after_labels = net.predict_labels(x).clone()
        twin = copy.deepcopy(net)
        twin.load_state_dict(ema_state_dict(opt, net))
        twin.eval()
        want = twin(x)[2]
        want_labels = twin.predict_labels(x)
    assert torch.equal(inside, want) and torch.equal(inside_labels, want_labels)
    assert not torch.equal(inside, before)  # the averaged weights are not the raw ones, and the forward saw them
    assert torch.equal(after, before) and torch.equal(after_labels, before_labels)
