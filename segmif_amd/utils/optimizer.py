"""AdamW with warm-up + polynomial decay, on one multi-tensor HIP kernel.

Counterpart of the reference's utils/optimizer.py (PolyWarmupAdamW :3-33, PolyWarmupAdamW_seg
:36-66): same constructor arguments, same in-`step()` learning-rate schedule (per-group initial LR
times a warm-up or polynomial factor, written back into `param_groups`), same arithmetic as
torch.optim.AdamW(eps=1e-8) — decoupled weight decay, bias correction, parameters whose `.grad` is
None are skipped.  One kernel launch updates every tensor (586 of them in the
segmentation step) instead of one aten foreach chain per group.
"""
import contextlib
import ctypes

import numpy as np
import torch

from .. import _lib

_CHUNK = 65536


def _bump_versions(params):
    """The kernel writes parameters through raw pointers, which autograd's version counters do not see; every cache
    keyed on `tensor._version` (core/_util.PackedCache: packed weights, folded BatchNorm, fused head matrices) would
    keep serving pre-step copies to the next eval / no_grad forward.  Bump the counters without touching the data."""
    if not params:
        return
    setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
    if setter is not None:
        try:
            setter(params, [p._version + 1 for p in params])
            return
        except (TypeError, RuntimeError):
            pass
    torch._foreach_add_(params, 0.0)


class _AdamEntry(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("lr", ctypes.c_float), ("wd", ctypes.c_float)]


def _ema_pointers(pairs):
    """the (hi, lo) pointer array of segmif_weight_ema_f32, in table order, as bytes"""
    return np.asarray([t.data_ptr() for pair in pairs for t in pair], dtype=np.uint64).tobytes()


def _upload_table(items, slots, dev, ema=None):
    """One host buffer, one copy: [AdamEntry table | chunk_off int64 | chunk_entry int32 | entry_slot int32] for `items` =
    (p, g, m, v, lr, wd) tuples in table order.  Returns the device bytes, the byte offsets of the three arrays and the counts.
    ema: one (hi, lo) pair per item; their 2 * len(items) pointers then sit between the table and chunk_off, at byte
    len(items) * sizeof(AdamEntry), and everything after them moves down."""
    entries = (_AdamEntry * len(items))()
    chunk_entry, chunk_off = [], []
    for i, (p, g, m, v, lr, wd) in enumerate(items):
        e = entries[i]
        e.p, e.g, e.n, e.lr, e.wd = p.data_ptr(), g.data_ptr(), p.numel(), lr, wd
        e.m, e.v = (m.data_ptr(), v.data_ptr()) if m is not None else (None, None)
        for off in range(0, p.numel(), _CHUNK):
            chunk_entry.append(i)
            chunk_off.append(off)
    co = np.asarray(chunk_off, dtype=np.int64).tobytes()
    ce = np.asarray(chunk_entry, dtype=np.int32).tobytes()
    sl = np.asarray(slots if slots is not None else [], dtype=np.int32).tobytes()
    pt = _ema_pointers(ema) if ema is not None else b""
    host = bytearray(bytes(entries) + pt + co + ce + sl)
    o_co = ctypes.sizeof(entries) + len(pt)
    o_ce = o_co + len(co)
    o_sl = o_ce + len(ce)
    blob = torch.frombuffer(host, dtype=torch.uint8).to(dev)
    return blob, (o_co, o_ce, o_sl), len(chunk_entry)


def _grown(buf, nbytes, dev):
    if buf is None or buf.numel() < nbytes or buf.device != dev:
        return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    return buf


_ENTRY_STAT = np.dtype([("sumsq", "<f8"), ("nonfinite", "<u4"), ("reserved", "<u4")])
_PARAM_COUNT = np.dtype([("skipped", "<u4"), ("offended", "<u4")])
_COUNTERS = ("attempts", "applied", "skipped", "clipped", "consecutive_skips")


def ema_decay_at(decay, warmup, t):
    """The decay of the average's update number t (t = 1 is the first): `decay`, or with warm-up min(decay, (1 + t) / (10 + t)) -
    the host restatement, in Python floats, of what csrc/weight_ema.hip forms per block in double."""
    decay, t = float(decay), max(int(t), 1)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def _check_ema_args(decay, warmup, who):
    if decay is None:
        if warmup:
            raise ValueError(f"{who}: ema_warmup without ema_decay")
        return None
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) < 1.0:
        raise ValueError(f"{who}: ema_decay {decay!r} must be a float inside (0, 1) (or None)")
    return float(decay)


def _check_guard_abi(lib):
    assert lib.segmif_adamw_entry_bytes() == ctypes.sizeof(_AdamEntry)
    assert lib.segmif_grad_guard_record_bytes() == ctypes.sizeof(_lib.SegmifGradGuardRecord)
    assert lib.segmif_grad_entry_stat_bytes() == _ENTRY_STAT.itemsize and lib.segmif_grad_param_count_bytes() == _PARAM_COUNT.itemsize


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW arithmetic in one multi-tensor launch.

    max_grad_norm (a positive float, inf allowed) and skip_nonfinite are this project's additions - the reference's optimizer
    has neither - and both are off by default: then step() is the plain path, unchanged.  With either one set, step() is the
    GUARDED path (csrc/grad_guard.hip), still without a host synchronisation:
      1. the global L2 norm of all gradients and the count of their inf / NaN elements are formed on the device, in a fixed
         order (bitwise reproducible), with the clip coefficient min(1, max_grad_norm / (norm + 1e-6)) of
         torch.nn.utils.clip_grad_norm_ (1 without max_grad_norm);
      2. the update runs on g * coef; with skip_nonfinite, a step whose gradients hold a non-finite element changes no
         parameter, exp_avg or exp_avg_sq.  Without skip_nonfinite such a step is applied as it is (the norm and the
         coefficient then come from the finite elements).
    Bias correction counts APPLIED steps: state["step"] on the host counts attempts, the device keeps every parameter's skipped
    attempts, and state_dict() stores the difference (so torch.optim.AdamW can load it) next to the guard's counters.
    A learning-rate schedule wrapped around step() (PolyWarmupAdamW, PolyWarmupAdamW_seg) advances on EVERY call, attempted or
    applied: the training loops run a fixed number of iterations and the schedule stays aligned with them.
    Data parallel runs: seg_train_step and FusionTrainer.step reduce the gradients before they call step(), so every rank
    sees the same gradients, forms the same norm and takes the same decision; the guard adds no collective.
    grad_stats() reads the device record back (one copy, one synchronisation): call it at log lines, not per step.

    ema_decay (a float inside (0, 1)) adds an exponential moving average of every parameter, also this project's and also off by
    default: state["ema"] (hi, a float32 clone of the parameter made at its first step, before the update) and state["ema_lo"],
    a PAIR of floats whose sum is the average.  After each hyper-parameter group's update one more launch (csrc/weight_ema.hip)
    forms, in double, ema += (1 - d_t) * (p - ema) with d_t = ema_decay, or with ema_warmup min(ema_decay, (1 + t) / (10 + t)),
    t the parameter's count of APPLIED steps - the bias correction's count.  A skipped step moves no average and does not advance
    t; a parameter without a gradient is not in the table and its average stays where it is.  No host synchronisation and no
    copy beyond the table upload, which carries the pointers.  ema_tensors() / ema_weights() / ema_state_dict() read it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm {max_grad_norm}: must be > 0 (or None)")
        self.ema_decay = _check_ema_args(ema_decay, ema_warmup, "FusedAdamW")
        self.ema_warmup = bool(ema_warmup)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._layout = None  # (signature, chunk_entry, chunk_off) cached while the grad set is unchanged
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._g_buf = None      # device bytes: [record | per-parameter counts | per-entry statistics of the last step]
        self._g_buf_slots = 0   # the number of parameters _g_buf was laid out for
        self._g_work = None     # per-chunk partials
        self._g_slots = {}      # id(parameter) -> index in the flattened param_groups (= its index in state_dict())
        self._g_last = []       # the parameters of the last step's table, in table order
        self._g_restore = {}    # counters from load_state_dict, written into the next record that is made

    # ------------------------------------------------------------------------------------------------ plain path
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        if self._guarded:
            self._step_guarded(lib)
            return loss
        assert lib.segmif_adamw_entry_bytes() == ctypes.sizeof(_AdamEntry)
        by_hyper = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamW: parameters must be contiguous fp32 tensors on the GPU")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                if self.ema_decay is not None and "ema" not in st:
                    self._ema_begin(st, p)
                st["step"] = int(st["step"]) + 1  # a torch.optim.AdamW checkpoint stores `step` as a tensor
                key = (st["step"], group["betas"], group["eps"], p.device)
                by_hyper.setdefault(key, []).append((p, p.grad.contiguous(), st, group["lr"], group["weight_decay"]))
        for (step, betas, eps, dev), items in by_hyper.items():
            entries = (_AdamEntry * len(items))()
            chunk_entry, chunk_off = [], []
            keep = []
            for i, (p, g, st, lr, wd) in enumerate(items):
                keep.append(g)
                e = entries[i]
                e.p, e.g, e.m, e.v = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                e.n, e.lr, e.wd = p.numel(), lr, wd
                for off in range(0, p.numel(), _CHUNK):
                    chunk_entry.append(i)
                    chunk_off.append(off)
            ema = self.ema_decay is not None  # (the average's pointers ride behind the table, in the same copy)
            pointers = _ema_pointers((st["ema"], st["ema_lo"]) for _, _, st, _, _ in items) if ema else b""
            table = torch.frombuffer(bytearray(bytes(entries) + pointers), dtype=torch.uint8).to(dev)
            ce = torch.tensor(chunk_entry, dtype=torch.int32, device=dev)
            co = torch.tensor(chunk_off, dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            # bias corrections in double on the host, like torch.optim.AdamW (fp32 powf is ~3e-5 off in early steps)
            bc1 = 1.0 - float(betas[0]) ** step
            bc2_sqrt = (1.0 - float(betas[1]) ** step) ** 0.5
            _lib.check(lib.segmif_adamw_f32(table.data_ptr(), ce.data_ptr(), co.data_ptr(), len(chunk_entry), _CHUNK,
                                            betas[0], betas[1], eps, bc1, bc2_sqrt, stream), "segmif_adamw_f32")
            if ema:
                _lib.check(lib.segmif_weight_ema_f32(table.data_ptr(), table.data_ptr() + ctypes.sizeof(entries), ce.data_ptr(),
                                                     co.data_ptr(), len(chunk_entry), _CHUNK, self.ema_decay, int(self.ema_warmup), step,
                                                     None, None, None, stream), "segmif_weight_ema_f32")
            self._keepalive = (table, ce, co, keep)
            _bump_versions([p for p, *_ in items])
        return loss

    # --------------------------------------------------------------------------------------------------- average
    @staticmethod
    def _ema_begin(st, p):
        """the pair starts at the parameter's value BEFORE its first averaged update (also for a state loaded without one)"""
        st["ema"] = p.detach().clone()
        st["ema_lo"] = torch.zeros_like(p)

    def ema_tensors(self):
        """{parameter: (hi, lo)} for the parameters that have an average (those that have had a gradient).  hi + lo is the
        average, hi its float32 rounding; both are the optimizer's own state tensors."""
        if self.ema_decay is None:
            raise RuntimeError("ema_tensors(): this optimizer keeps no average (ema_decay)")
        return {p: (self.state[p]["ema"], self.state[p]["ema_lo"]) for g in self.param_groups for p in g["params"]
                if "ema" in self.state.get(p, ())}

    # ---------------------------------------------------------------------------------------------- guarded path
    def _guard_layout(self, n_slots=None):
        """byte offsets inside _g_buf: [record | one count per parameter of param_groups | one statistic per entry, at most as many]"""
        if n_slots is None:
            n_slots = sum(len(g["params"]) for g in self.param_groups)
        o_counts = ctypes.sizeof(_lib.SegmifGradGuardRecord)
        return n_slots, o_counts, o_counts + n_slots * _PARAM_COUNT.itemsize

    def _guard_buffer(self, dev):
        n_slots, o_counts, o_entries = self._guard_layout()
        old = self._g_buf
        if old is None or old.device != dev or self._g_buf_slots != n_slots:
            self._g_slots = {id(p): i for i, p in enumerate(p for g in self.param_groups for p in g["params"])}
            rec = _lib.SegmifGradGuardRecord()
            for k in _COUNTERS:
                setattr(rec, k, int(self._g_restore.get(k, 0)))
            self._g_restore = {}
            host = bytearray(o_entries + n_slots * _ENTRY_STAT.itemsize)
            host[:o_counts] = bytes(rec)
            buf = torch.frombuffer(host, dtype=torch.uint8).to(dev)
            if old is not None and old.device == buf.device:  # add_param_group appends: the record and the counts so far move over
                keep = o_counts + min(self._g_buf_slots, n_slots) * _PARAM_COUNT.itemsize
                buf[:keep].copy_(old[:keep])
            self._g_buf, self._g_buf_slots, self._g_last = buf, n_slots, []
        return self._g_buf, o_counts, o_entries

    def _step_guarded(self, lib):
        _check_guard_abi(lib)
        by_hyper, dev = {}, None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamW: parameters must be contiguous fp32 tensors on the GPU")
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError("FusedAdamW: the guarded step forms ONE norm; its parameters must share a device")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                if self.ema_decay is not None and "ema" not in st:
                    self._ema_begin(st, p)
                st["step"] = int(st["step"]) + 1  # attempts; the device subtracts the parameter's skipped ones
                key = (st["step"], tuple(group["betas"]), group["eps"])
                by_hyper.setdefault(key, []).append((p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], group["lr"],
                                                     group["weight_decay"]))
        ema = [(self.state[it[0]]["ema"], self.state[it[0]]["ema_lo"]) for its in by_hyper.values() for it in its] \
            if self.ema_decay is not None else None
        items = [it for group_items in by_hyper.values() for it in group_items]  # table order: hyper-parameter groups in a row
        if not any(it[0].numel() for it in items):
            return
        buf, o_counts, o_entries = self._guard_buffer(dev)
        blob, (o_co, o_ce, o_sl), nchunks = _upload_table(items, [self._g_slots[id(it[0])] for it in items], dev, ema)
        self._g_work = _grown(self._g_work, lib.segmif_grad_norm_workspace_bytes(nchunks), dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        base, rec = blob.data_ptr(), buf.data_ptr()
        max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
        _lib.check(lib.segmif_grad_norm_f32(base, len(items), base + o_ce, base + o_co, nchunks, _CHUNK, self._g_work.data_ptr(),
                                            rec + o_entries, rec, base + o_sl, rec + o_counts, max_norm, int(self.skip_nonfinite),
                                            stream), "segmif_grad_norm_f32")
        c0 = 0
        for (step, betas, eps), group_items in by_hyper.items():
            nc = sum((it[0].numel() + _CHUNK - 1) // _CHUNK for it in group_items)
            if nc:
                _lib.check(lib.segmif_adamw_guarded_f32(base, base + o_ce + 4 * c0, base + o_co + 8 * c0, nc, _CHUNK, float(betas[0]),
                                                        float(betas[1]), eps, step, rec, base + o_sl, rec + o_counts, stream),
                           "segmif_adamw_guarded_f32")
                if ema is not None:
                    _lib.check(lib.segmif_weight_ema_f32(base, base + len(items) * ctypes.sizeof(_AdamEntry), base + o_ce + 4 * c0,
                                                         base + o_co + 8 * c0, nc, _CHUNK, self.ema_decay, int(self.ema_warmup), step,
                                                         rec, base + o_sl, rec + o_counts, stream), "segmif_weight_ema_f32")
            c0 += nc
        self._keepalive = (blob, [it[1] for it in items])
        self._g_last = [it[0] for it in items]
        _bump_versions(self._g_last)  # (on a skipped step too: a version bump without a change is harmless)

    def _read_guard(self):
        """(record, per-parameter counts, per-entry statistics of the last step) in ONE device-to-host copy"""
        n_now = self._guard_layout()[0]
        if self._g_buf is None:
            rec = _lib.SegmifGradGuardRecord()
            for k in _COUNTERS:
                setattr(rec, k, int(self._g_restore.get(k, 0)))
            return rec, np.zeros(n_now, _PARAM_COUNT), np.zeros(0, _ENTRY_STAT)
        n_slots, o_counts, o_entries = self._guard_layout(self._g_buf_slots)
        n = len(self._g_last)
        raw = self._g_buf[:o_entries + n * _ENTRY_STAT.itemsize].cpu().numpy().tobytes()
        counts = np.zeros(max(n_now, n_slots), _PARAM_COUNT)  # (parameters added since the last step have no counts yet)
        counts[:n_slots] = np.frombuffer(raw, dtype=_PARAM_COUNT, count=n_slots, offset=o_counts)
        return (_lib.SegmifGradGuardRecord.from_buffer_copy(raw[:o_counts]), counts,
                np.frombuffer(raw, dtype=_ENTRY_STAT, count=n, offset=o_entries))

    def grad_stats(self):
        """The guard's record after the last step(): norm (over the finite elements), coef, nonfinite (elements), the running
        counters attempts / applied / skipped / clipped / consecutive_skips, and per_param - one dict per gradient of the last
        step, in table order: the parameter tensor itself (map it to a name through named_parameters()), its gradient's norm and
        non-finite count, and in how many steps so far it carried a non-finite gradient.  One readback."""
        if not self._guarded:
            raise RuntimeError("grad_stats(): this optimizer has no guard (max_grad_norm / skip_nonfinite)")
        rec, counts, ent = self._read_guard()
        out = {k: getattr(rec, k) for k in ("sumsq", "norm", "coef", "nonfinite") + _COUNTERS}
        out["skip_now"] = bool(rec.skip_now)
        out["per_param"] = [{"param": p, "sumsq": float(e["sumsq"]), "norm": float(e["sumsq"]) ** 0.5, "nonfinite": int(e["nonfinite"]),
                             "offended_steps": int(counts[self._g_slots[id(p)]]["offended"])} for p, e in zip(self._g_last, ent)]
        return out

    def state_dict(self):
        """torch's layout.  Guarded: `step` is the count of APPLIED steps (attempts minus the parameter's skipped ones, one
        readback), and "grad_guard" holds the counters."""
        sd = super().state_dict()
        if not self._guarded:
            return sd
        rec, counts, _ = self._read_guard()
        sd["state"] = {k: dict(v, step=int(v["step"]) - int(counts[k]["skipped"])) for k, v in sd["state"].items()}
        sd["grad_guard"] = {k: int(getattr(rec, k)) for k in _COUNTERS}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._guarded:  # the loaded `step`s are applied steps: the per-parameter skipped counts start again at zero
            self._g_buf, self._g_last = None, []
            self._g_restore = dict(state_dict.get("grad_guard") or {})


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ on the device kernels of csrc/grad_guard.hip, for loops that keep a torch optimizer: the
    L2 norm of all gradients in two launches (fixed order, bitwise reproducible), then g *= min(1, max_norm / (norm + 1e-6)) in
    one more (none of the gradients is written when the coefficient is 1).  Returns the norm as a device scalar; nothing
    synchronises unless error_if_nonfinite asks for the check.  Gradients with inf / NaN elements: the returned norm is NaN
    (torch: NaN or inf) and the coefficient comes from the finite elements.  `foreach` is accepted and ignored."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: the device kernels form the L2 norm only")
    if not float(max_norm) > 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm {max_norm} must be > 0")
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    dev = params[0].device
    for p in params:
        if not p.grad.is_cuda or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != dev:
            raise RuntimeError("clip_grad_norm_: gradients must be contiguous fp32 tensors on one GPU")
    lib = _lib.load()
    _check_guard_abi(lib)
    blob, (o_co, o_ce, _), nchunks = _upload_table([(p, p.grad, None, None, 0.0, 0.0) for p in params], None, dev)
    o_entries = ctypes.sizeof(_lib.SegmifGradGuardRecord)
    buf = torch.zeros(o_entries + len(params) * _ENTRY_STAT.itemsize, dtype=torch.uint8, device=dev)
    if nchunks:
        work = torch.empty(lib.segmif_grad_norm_workspace_bytes(nchunks), dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        base, rec = blob.data_ptr(), buf.data_ptr()
        _lib.check(lib.segmif_grad_norm_f32(base, len(params), base + o_ce, base + o_co, nchunks, _CHUNK, work.data_ptr(),
                                            rec + o_entries, rec, None, None, float(max_norm), 0, stream), "segmif_grad_norm_f32")
        _lib.check(lib.segmif_grad_scale_f32(base, base + o_ce, base + o_co, nchunks, _CHUNK, rec, stream), "segmif_grad_scale_f32")
    norm = buf[8:12].view(torch.float32).reshape(())
    nonfinite = buf[16:20].view(torch.int32).reshape(())
    if error_if_nonfinite and int(nonfinite) != 0:
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    return torch.where(nonfinite != 0, torch.full_like(norm, float("nan")), norm)


class WeightEMA:
    """The average of FusedAdamW(ema_decay=...) on its own, for loops that keep a torch optimizer (as clip_grad_norm_ is the
    stand-alone form of the guard): hi (a clone) and lo are made here, update() - call it after optimizer.step() - is one launch
    of csrc/weight_ema.hip over all parameters with this object's own count of updates as t.  No CPU fallback: update() on
    anything but contiguous fp32 tensors of one GPU raises."""

    def __init__(self, params, decay, warmup=False):
        if decay is None:
            raise ValueError("WeightEMA: decay must be a float inside (0, 1)")
        self.decay = _check_ema_args(decay, warmup, "WeightEMA")
        self.warmup = bool(warmup)
        self.params = [params] if isinstance(params, torch.Tensor) else list(params)
        self.hi = [p.detach().clone() for p in self.params]
        self.lo = [torch.zeros_like(p) for p in self.params]
        self.step = 0
        self._table = None  # (signature, device bytes, offsets, chunks): the pointers change only when a tensor is rebound

    def ema_tensors(self):
        return {p: (h, l) for p, h, l in zip(self.params, self.hi, self.lo)}

    @torch.no_grad()
    def update(self):
        if not self.params:
            return
        dev = self.params[0].device
        for t in self.params + self.hi + self.lo:
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError("WeightEMA.update: parameters must be contiguous fp32 tensors on one GPU (there is no CPU path)")
        lib = _lib.load()
        assert lib.segmif_adamw_entry_bytes() == ctypes.sizeof(_AdamEntry)
        sig = tuple(t.data_ptr() for t in self.params + self.hi + self.lo)
        if self._table is None or self._table[0] != sig:
            blob, offs, nchunks = _upload_table([(p, p, None, None, 0.0, 0.0) for p in self.params], None, dev,
                                                list(zip(self.hi, self.lo)))
            self._table = (sig, blob, offs, nchunks)
        _, blob, (o_co, o_ce, _), nchunks = self._table
        self.step += 1
        if nchunks:
            base = blob.data_ptr()
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.segmif_weight_ema_f32(base, base + len(self.params) * ctypes.sizeof(_AdamEntry), base + o_ce, base + o_co,
                                                 nchunks, _CHUNK, self.decay, int(self.warmup), self.step, None, None, None, stream),
                       "segmif_weight_ema_f32")

    def state_dict(self):
        return {"step": self.step, "decay": self.decay, "warmup": self.warmup, "ema": [t.clone() for t in self.hi],
                "ema_lo": [t.clone() for t in self.lo]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        hi, lo = state_dict["ema"], state_dict["ema_lo"]
        if len(hi) != len(self.hi) or len(lo) != len(self.lo) or any(a.shape != b.shape for a, b in zip(hi + lo, self.hi + self.lo)):
            raise ValueError("WeightEMA.load_state_dict: the stored averages do not match the parameters")
        for dst, src in zip(self.hi + self.lo, hi + lo):
            dst.copy_(src)  # in place: the uploaded table keeps pointing at them
        self.step = int(state_dict["step"])


@contextlib.contextmanager
def ema_weights(source, module):
    """`with ema_weights(source, module):` runs its body on the AVERAGED weights.  source: a FusedAdamW with ema_decay or a
    WeightEMA.  On entry every parameter of `module` that has an average is overwritten in place with hi (copy_ under no_grad,
    never a rebind of .data: graph captures and the gradient reducer's buckets hold the pointers), the raw values stashed first;
    on exit - after an exception too - they are copied back bit for bit.  Buffers (BatchNorm's running statistics) and
    parameters without an average are left alone.  Both copies raise the parameters' _version, so core/_util.PackedCache
    repacks.  torch operators only: works on CPU tensors as well."""
    avg = source.ema_tensors()
    swapped = [(p, p.detach().clone(), avg[p][0]) for p in module.parameters() if p in avg]
    with torch.no_grad():
        for p, _, hi in swapped:
            p.copy_(hi)
    try:
        yield module
    finally:
        with torch.no_grad():
            for p, raw, _ in swapped:
                p.copy_(raw)


def ema_state_dict(source, module):
    """module.state_dict() with hi in place of every averaged parameter: the same keys, every tensor cloned, the module untouched."""
    avg = source.ema_tensors()
    hi = {n: avg[p][0] for n, p in module.named_parameters(remove_duplicate=False) if p in avg}
    return {k: (hi[k] if k in hi else v).detach().clone() for k, v in module.state_dict().items()}


class _PolyWarmupMixin:
    def _init_schedule(self, global_step, warmup_iter, max_iter, warmup_ratio, power):
        self.global_step = global_step
        self.warmup_iter, self.warmup_ratio, self.max_iter, self.power = warmup_iter, warmup_ratio, max_iter, power
        self._init_lr = [g["lr"] for g in self.param_groups]

    def _apply_schedule(self):
        mult = None
        if self.global_step < self.warmup_iter:
            mult = 1 - (1 - self.global_step / self.warmup_iter) * (1 - self.warmup_ratio)
        elif self.global_step < self.max_iter:
            mult = (1 - self.global_step / self.max_iter) ** self.power
        if mult is not None:
            for g, lr0 in zip(self.param_groups, self._init_lr):
                g["lr"] = lr0 * mult


class PolyWarmupAdamW(_PolyWarmupMixin, FusedAdamW):
    def __init__(self, params, lr, weight_decay, betas, warmup_iter=None, max_iter=None, warmup_ratio=None, power=None,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        FusedAdamW.__init__(self, params, lr=lr, betas=tuple(betas), weight_decay=weight_decay, eps=1e-8, max_grad_norm=max_grad_norm,
                            skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup)
        self._init_schedule(0, warmup_iter, max_iter, warmup_ratio, power)

    def step(self, closure=None):
        self._apply_schedule()
        out = FusedAdamW.step(self, closure)
        self.global_step += 1
        return out


class PolyWarmupAdamW_seg(_PolyWarmupMixin, FusedAdamW):
    def __init__(self, params, lr, weight_decay, betas, iter_curr, warmup_iter=None, max_iter=None, warmup_ratio=None,
                 power=None, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        FusedAdamW.__init__(self, params, lr=lr, betas=tuple(betas), weight_decay=weight_decay, eps=1e-8, max_grad_norm=max_grad_norm,
                            skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup)
        self._init_schedule(iter_curr, warmup_iter, max_iter, warmup_ratio, power)

    def step(self, closure=None):
        self._apply_schedule()
        out = FusedAdamW.step(self, closure)
        self.global_step += 1
        return out
