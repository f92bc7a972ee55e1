"""Host-side checks of the weight average (no kernel is launched): the training command refuses senseless --ema-* flags before it
looks for a device, the constructors refuse senseless decays, ema_decay_at restates the kernel's d_t, the ema_weights swap and its
restore work on CPU tensors, WeightEMA.update() has no CPU path, the new constructor arguments leave the learning-rate schedule
alone, the entry point rejects bad descriptors and the average's state travels through state_dict()."""
import copy
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv,needle", [(["--ema-decay", "1.0"], "--ema-decay"), (["--ema-decay", "0"], "--ema-decay"),
                                         (["--ema-warmup"], "--ema-decay"), (["--ema-nets", "both"], "--ema-decay")])
def test_train_refuses_senseless_ema_flags_before_the_device_check(argv, needle, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--synthetic", "4"] + argv)
    assert exc.value.code == 2 and needle in capsys.readouterr().err


def test_constructors_refuse_a_senseless_decay():
    from segmif_amd.utils.optimizer import FusedAdamW, PolyWarmupAdamW, PolyWarmupAdamW_seg, WeightEMA
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError):
            FusedAdamW([p], ema_decay=bad)
        with pytest.raises(ValueError):
            WeightEMA([p], bad)
    with pytest.raises(ValueError):
        FusedAdamW([p], ema_warmup=True)
    with pytest.raises(ValueError):
        WeightEMA([p], None, warmup=True)
    with pytest.raises(ValueError):
        WeightEMA([p], None)
    opt = FusedAdamW([p], ema_decay=0.999, ema_warmup=True)
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True and opt._guarded is False and opt.ema_tensors() == {}
    assert FusedAdamW([p]).ema_decay is None
    with pytest.raises(RuntimeError):
        FusedAdamW([p]).ema_tensors()  # no average to report
    a = PolyWarmupAdamW([p], 1e-3, 0.0, (0.9, 0.999), 1, 10, 0.1, 1.0, ema_decay=0.99)
    b = PolyWarmupAdamW_seg([p], 1e-3, 0.0, (0.9, 0.999), 0, 1, 10, 0.1, 1.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True)
    assert (a.ema_decay, a.ema_warmup, b.ema_decay, b.ema_warmup, b._guarded) == (0.99, False, 0.9, True, True)


def test_train_optimizer_factories_pass_the_average_through():
    from segmif_amd import train

    class Seg:
        class denoise_net:
            @staticmethod
            def get_param_groups():
                return [[torch.nn.Parameter(torch.zeros(2))], [torch.nn.Parameter(torch.zeros(2))], [torch.nn.Parameter(torch.zeros(2))]]

    opt = train.make_seg_optimizer(Seg(), ema_decay=0.9999, ema_warmup=True)
    assert (opt.ema_decay, opt.ema_warmup) == (0.9999, True) and train.make_seg_optimizer(Seg()).ema_decay is None
    fus = torch.nn.Linear(2, 2)
    opt = train.make_fusion_optimizer(fus, 2, ema_decay=0.99)
    assert (opt.ema_decay, opt.ema_warmup) == (0.99, False) and train.make_fusion_optimizer(fus, 2).ema_decay is None


@pytest.mark.parametrize("decay", [0.9999, 0.5])
def test_ema_decay_at(decay):
    from segmif_amd.utils.optimizer import ema_decay_at
    for t in (1, 2, 9, 10, 10 ** 4):
        assert ema_decay_at(decay, True, t) == min(decay, (1 + t) / (10 + t))
        assert ema_decay_at(decay, False, t) == decay
    assert ema_decay_at(0.9999, True, 1) == 2 / 11 and ema_decay_at(0.9999, True, 10 ** 6) == 0.9999
    assert ema_decay_at(0.9999, True, 0) == 2 / 11  # floored at the first update, as the kernel floors t


def small_module():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    net.idle = torch.nn.Parameter(torch.randn(5))
    return net


def test_swap_restore_and_state_dict_on_cpu_tensors():
    """ema_weights through a WeightEMA over CPU parameters: only the averaged parameters swap, buffers stay, versions grow, the raw
    values come back bit for bit - after an exception too; ema_state_dict has the module's keys and leaves it alone."""
    from segmif_amd.utils.optimizer import WeightEMA, ema_state_dict, ema_weights
    net = small_module()
    averaged = [net[0].weight, net[0].bias, net[1].weight]  # (net[1].bias and net.idle have no average)
    ema = WeightEMA(averaged, 0.99)
    assert all(torch.equal(h, p) and not l.any() for p, (h, l) in ema.ema_tensors().items()) and len(ema.ema_tensors()) == 3
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)  # the "training": raw and averaged weights now differ
        net[1].running_mean.fill_(0.25)
    raw = {n: p.detach().clone() for n, p in net.named_parameters()}
    buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
    pointers = {n: p.data_ptr() for n, p in net.named_parameters()}
    versions = {n: p._version for n, p in net.named_parameters()}

    def check_inside():
        for n, p in net.named_parameters():
            if any(p is q for q in averaged):
                assert torch.equal(p, ema.ema_tensors()[p][0]) and not torch.equal(p, raw[n]) and p._version > versions[n]
            else:
                assert torch.equal(p, raw[n]) and p._version == versions[n]
            assert p.data_ptr() == pointers[n]
        assert all(torch.equal(b, buffers[n]) for n, b in net.named_buffers())

    def check_restored(swaps):
        for n, p in net.named_parameters():
            assert torch.equal(p, raw[n]) and p.data_ptr() == pointers[n]
            assert p._version == versions[n] + (2 * swaps if any(p is q for q in averaged) else 0)
        assert all(torch.equal(b, buffers[n]) for n, b in net.named_buffers())

    with ema_weights(ema, net) as inside:
        assert inside is net
        check_inside()
    check_restored(1)
    with pytest.raises(KeyError, match="boom"):
        with ema_weights(ema, net):
            check_inside()
            raise KeyError("boom")
    check_restored(2)
    sd = ema_state_dict(ema, net)
    assert list(sd) == list(net.state_dict())
    for k, v in net.state_dict().items():
        want = ema.ema_tensors()[dict(net.named_parameters())[k]][0] if k in ("0.weight", "0.bias", "1.weight") else v
        assert torch.equal(sd[k], want) and sd[k].data_ptr() not in (v.data_ptr(), want.data_ptr())
    check_restored(2)


def test_update_has_no_cpu_path():
    from segmif_amd.utils.optimizer import WeightEMA
    p = torch.nn.Parameter(torch.zeros(7))
    ema = WeightEMA([p], 0.9)
    with pytest.raises(RuntimeError, match="GPU"):
        ema.update()
    assert ema.step == 0 and not ema.hi[0].any()


def test_schedule_is_unchanged_by_the_ema_arguments():
    """Twelve _apply_schedule calls without a step(): the learning rates with and without the average's arguments are identical."""
    from segmif_amd.utils.optimizer import PolyWarmupAdamW, PolyWarmupAdamW_seg

    def lrs(cls, extra, **kw):
        ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2))]
        opt = cls([{"params": ps[:1], "lr": 1e-2, "weight_decay": 0.0}, {"params": ps[1:], "lr": 1e-1, "weight_decay": 0.01}], lr=1e-2,
                  weight_decay=0.0, betas=(0.9, 0.999), warmup_iter=10, max_iter=100, warmup_ratio=0.1, power=1.0, **extra, **kw)
        seen = []
        for _ in range(12):
            opt._apply_schedule()
            opt.global_step += 1
            seen.append([g["lr"] for g in opt.param_groups])
        return seen

    ema = dict(ema_decay=0.9999, ema_warmup=True)
    assert lrs(PolyWarmupAdamW, {}) == lrs(PolyWarmupAdamW, ema)
    assert lrs(PolyWarmupAdamW_seg, {}, iter_curr=5) == lrs(PolyWarmupAdamW_seg, ema, iter_curr=5)
    seen = lrs(PolyWarmupAdamW_seg, ema, iter_curr=0)
    assert abs(seen[0][0] - 1e-2 * 0.1) < 1e-12 and abs(seen[11][1] - 1e-1 * (1 - 11 / 100)) < 1e-12


def test_weight_ema_state_travels_through_state_dict_on_the_cpu():
    from segmif_amd.utils.optimizer import WeightEMA
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(5, generator=g)), torch.nn.Parameter(torch.randn(2, 3, generator=g))]
    a = WeightEMA(ps, 0.999, warmup=True)
    a.step = 17
    for t in a.hi + a.lo:
        t.copy_(torch.randn(t.shape, generator=g))
    sd = copy.deepcopy(a.state_dict())
    assert sd["step"] == 17 and sd["decay"] == 0.999 and sd["warmup"] is True
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.state_dict()["ema"], a.hi))  # clones, not views
    b = WeightEMA([torch.nn.Parameter(p.detach().clone()) for p in ps], 0.999, warmup=True)
    pointers = [t.data_ptr() for t in b.hi + b.lo]
    b.load_state_dict(sd)
    assert b.step == 17 and [t.data_ptr() for t in b.hi + b.lo] == pointers
    assert all(torch.equal(x, y) for x, y in zip(a.hi + a.lo, b.hi + b.lo))
    with pytest.raises(ValueError):
        WeightEMA(ps[:1], 0.999).load_state_dict(sd)


def test_optimizer_without_a_step_has_no_ema_state_and_torch_loads_its_dict():
    from segmif_amd.utils.optimizer import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    sd = FusedAdamW([p], ema_decay=0.9).state_dict()
    assert sd["state"] == {} and "grad_guard" not in sd
    torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))]).load_state_dict(sd)


def test_table_upload_carries_the_pointer_array():
    """_upload_table with ema pairs: the 2 n pointers sit right behind the table, the three arrays move down by 16 n bytes and keep
    their contents; without pairs the layout is what it was."""
    import numpy as np
    from segmif_amd.utils import optimizer
    ts = [torch.zeros(n) for n in (1, 65537, 0)]
    pairs = [(torch.zeros(n), torch.zeros(n)) for n in (1, 65537, 0)]
    items = [(t, t, None, None, 0.5, 0.25) for t in ts]
    plain, (p_co, p_ce, p_sl), nchunks = optimizer._upload_table(items, [2, 1, 0], "cpu")
    blob, (o_co, o_ce, o_sl), n2 = optimizer._upload_table(items, [2, 1, 0], "cpu", pairs)
    size = 3 * ctypes.sizeof(optimizer._AdamEntry)
    assert nchunks == n2 == 3 and (o_co, o_ce, o_sl) == (p_co + 48, p_ce + 48, p_sl + 48) and p_co == size and o_co % 8 == 0
    raw, old = blob.numpy().tobytes(), plain.numpy().tobytes()
    assert raw[:size] == old[:size] and raw[o_co:] == old[p_co:]
    assert np.frombuffer(raw, np.uint64, 6, size).tolist() == [t.data_ptr() for pair in pairs for t in pair]


def test_entry_point_rejects_bad_descriptors():
    from segmif_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    ok = dict(table=8, ema=8, ce=8, co=8, nchunks=1, chunk=65536, decay=0.9, warmup=0, step=1, rec=None, slot=None, count=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.segmif_weight_ema_f32(a["table"], a["ema"], a["ce"], a["co"], a["nchunks"], a["chunk"], a["decay"], a["warmup"],
                                         a["step"], a["rec"], a["slot"], a["count"], None)

    for bad in (dict(table=None), dict(ema=None), dict(ce=None), dict(co=None), dict(nchunks=0), dict(chunk=65534), dict(chunk=0),
                dict(decay=0.0), dict(decay=1.0), dict(decay=float("nan")), dict(decay=-0.1), dict(step=0), dict(slot=8),
                dict(count=8)):
        assert call(**bad) == -22, bad  # (every one returns before a launch)
