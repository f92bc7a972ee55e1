"""Host-side checks of the guarded optimizer step (no kernel is launched): the training command refuses senseless guard flags
before it looks for a device, the ctypes mirrors of csrc/grad_guard.hip's records match the library's sizes and the header's
layout, and the new constructor arguments leave the learning-rate schedule alone."""
import ctypes
import os

import pytest
import torch


@pytest.mark.parametrize("argv,needle", [(["--clip-grad-norm", "-1.0"], "--clip-grad-norm"), (["--clip-grad-norm", "0"], "--clip-grad-norm"),
                                         (["--clip-grad-norm", "inf"], "--clip-grad-norm"),
                                         (["--skip-nonfinite", "--max-consecutive-skips", "0"], "--max-consecutive-skips")])
def test_train_refuses_senseless_guard_flags_before_the_device_check(argv, needle, capsys):
    from segmif_amd import train
    with pytest.raises(SystemExit) as exc:
        train.main(["--synthetic", "4"] + argv)
    assert exc.value.code == 2 and needle in capsys.readouterr().err


def test_optimizer_refuses_a_senseless_clip_value():
    from segmif_amd.utils.optimizer import FusedAdamW, PolyWarmupAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            FusedAdamW([p], max_grad_norm=bad)
    assert FusedAdamW([p])._guarded is False and FusedAdamW([p], max_grad_norm=float("inf"))._guarded is True
    assert PolyWarmupAdamW([p], 1e-3, 0.0, (0.9, 0.999), 1, 10, 0.1, 1.0, skip_nonfinite=True)._guarded is True


def test_record_structs_match_the_library_and_the_header():
    from segmif_amd import _lib, build
    from segmif_amd.utils import optimizer
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    rec, ent, cnt = _lib.SegmifGradGuardRecord, _lib.SegmifGradEntryStat, _lib.SegmifGradParamCount
    assert ctypes.sizeof(rec) == lib.segmif_grad_guard_record_bytes() == 48
    assert ctypes.sizeof(ent) == lib.segmif_grad_entry_stat_bytes() == optimizer._ENTRY_STAT.itemsize
    assert ctypes.sizeof(cnt) == lib.segmif_grad_param_count_bytes() == optimizer._PARAM_COUNT.itemsize
    optimizer._check_guard_abi(lib)  # (the header's layout of the three: tests/test_abi_and_host.py::test_struct_layouts_match_c)
    # size rules and rejections, no launch
    assert lib.segmif_grad_norm_workspace_bytes(0) == 0 and lib.segmif_grad_norm_workspace_bytes(11) == 11 * 16
    assert lib.segmif_grad_norm_f32(None, 1, None, None, 1, 65536, None, None, None, None, None, 1.0, 0, None) == -22
    assert lib.segmif_adamw_guarded_f32(None, None, None, 1, 65536, 0.9, 0.999, 1e-8, 1, None, None, None, None) == -22
    assert lib.segmif_grad_scale_f32(None, None, None, 1, 65536, None, None) == -22


def test_table_upload_layout_on_the_host():
    """_upload_table's one buffer: table, then chunk offsets (int64), chunk entries and slots (int32), 65 536 elements per chunk."""
    import numpy as np
    from segmif_amd.utils import optimizer
    ts = [torch.zeros(n) for n in (1, 65536, 65537, 0, 100000)]
    blob, (o_co, o_ce, o_sl), nchunks = optimizer._upload_table([(t, t, None, None, 0.5, 0.25) for t in ts], [4, 3, 2, 1, 0], "cpu")
    raw = blob.numpy().tobytes()
    assert nchunks == 6 and o_co == 5 * ctypes.sizeof(optimizer._AdamEntry) and o_co % 8 == 0 and o_ce % 4 == 0
    assert np.frombuffer(raw, np.int64, nchunks, o_co).tolist() == [0, 0, 0, 65536, 0, 65536]
    assert np.frombuffer(raw, np.int32, nchunks, o_ce).tolist() == [0, 1, 2, 2, 4, 4]
    assert np.frombuffer(raw, np.int32, 5, o_sl).tolist() == [4, 3, 2, 1, 0] and len(raw) == o_sl + 20
    sz = ctypes.sizeof(optimizer._AdamEntry)
    e = optimizer._AdamEntry.from_buffer_copy(raw[2 * sz:3 * sz])
    assert e.n == 65537 and e.g == ts[2].data_ptr() and e.m is None and e.lr == 0.5 and e.wd == 0.25


def test_schedule_is_unchanged_by_the_guard_arguments():
    """Twelve _apply_schedule calls without a step(): the learning rates with and without the guard arguments are identical."""
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

    guard = dict(max_grad_norm=1.0, skip_nonfinite=True)
    assert lrs(PolyWarmupAdamW, {}) == lrs(PolyWarmupAdamW, guard)
    assert lrs(PolyWarmupAdamW_seg, {}, iter_curr=5) == lrs(PolyWarmupAdamW_seg, guard, iter_curr=5)
    seen = lrs(PolyWarmupAdamW_seg, guard, iter_curr=0)
    assert abs(seen[0][0] - 1e-2 * 0.1) < 1e-12 and abs(seen[11][1] - 1e-1 * (1 - 11 / 100)) < 1e-12


def test_guard_counters_travel_through_state_dict_without_a_device():
    """Before any step there is no device buffer: state_dict() reports zero counters, load_state_dict() keeps loaded ones."""
    from segmif_amd.utils.optimizer import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedAdamW([p], skip_nonfinite=True)
    sd = opt.state_dict()
    assert sd["grad_guard"] == dict(attempts=0, applied=0, skipped=0, clipped=0, consecutive_skips=0) and sd["state"] == {}
    sd["grad_guard"] = dict(attempts=9, applied=7, skipped=2, clipped=3, consecutive_skips=1)
    opt.load_state_dict(sd)
    st = opt.grad_stats()
    assert (st["attempts"], st["applied"], st["skipped"], st["clipped"], st["consecutive_skips"]) == (9, 7, 2, 3, 1)
    assert st["per_param"] == [] and "grad_guard" not in FusedAdamW([p]).state_dict()


def test_guard_buffer_keeps_record_and_counts_when_a_group_is_added():
    """_guard_buffer on the host: laid out for the parameters of param_groups; add_param_group appends, and the record and the
    counts so far move over into the larger buffer."""
    from segmif_amd import _lib
    from segmif_amd.utils.optimizer import FusedAdamW
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 7))
    opt = FusedAdamW([a, b], skip_nonfinite=True)
    buf, o_counts, o_entries = opt._guard_buffer(torch.device("cpu"))
    assert (o_counts, o_entries, buf.numel()) == (48, 48 + 2 * 8, 48 + 2 * 8 + 2 * 16) and opt._g_slots == {id(a): 0, id(b): 1}
    assert opt._guard_buffer(torch.device("cpu"))[0] is buf
    rec = _lib.SegmifGradGuardRecord(attempts=4, applied=3, skipped=1, norm=2.5)
    buf[:48] = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8)
    buf[o_counts + 8:o_counts + 12] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)  # b sat through one skipped step
    opt.add_param_group({"params": [c]})
    big, _, o_entries = opt._guard_buffer(torch.device("cpu"))
    assert big is not buf and big.numel() == 48 + 3 * 8 + 3 * 16 and opt._g_slots[id(c)] == 2
    got, counts, ent = opt._read_guard()
    assert (got.attempts, got.applied, got.skipped, got.norm) == (4, 3, 1, 2.5)
    assert counts["skipped"].tolist() == [0, 1, 0] and len(ent) == 0


def test_guard_log_lines_and_the_stop_after_consecutive_skips():
    """train._GuardLog over a stand-in optimizer: counts since the previous line, the worst offenders by name, and the stop
    message once more than N steps in a row were skipped."""
    from segmif_amd.train import _GuardLog
    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Linear(2, 1))
    ps = dict(net.named_parameters())

    class Opt:
        def grad_stats(self):
            return self.stats

    def stats(norm, clipped, skipped, consecutive, bad):
        return dict(norm=norm, clipped=clipped, skipped=skipped, consecutive_skips=consecutive,
                    per_param=[dict(param=p, nonfinite=bad.get(n, (0, 0))[0], offended_steps=bad.get(n, (0, 0))[1]) for n, p in ps.items()])

    opt = Opt()
    log = _GuardLog(opt, [("net", net)], max_consecutive=2)
    opt.stats = stats(3.0, 4, 0, 0, {})
    assert log.line() == " gnorm 3.0000e+00 clipped 4 skipped 0" and log.stop is None
    log.check()
    opt.stats = stats(1.5, 6, 2, 2, {"0.weight": (3, 2), "1.bias": (1, 1)})
    assert log.line() == " gnorm 1.5000e+00 clipped 2 skipped 2 non-finite gradients in net.0.weight (2 steps), net.1.bias (1 steps)"
    log.check()  # two in a row: not yet MORE than 2
    opt.stats = stats(1.5, 6, 5, 5, {"0.weight": (3, 5), "1.bias": (0, 1)})
    assert log.line().endswith("skipped 3 non-finite gradients in net.0.weight (3 steps)")
    with pytest.raises(SystemExit, match=r"5 steps in a row .*--max-consecutive-skips 2.*net\.0\.weight"):
        log.check()
