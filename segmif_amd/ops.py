"""Thin tensor-level wrappers over the C ABI (include/segmif_hip.h).

Conventions: fp32 CUDA(HIP) tensors, NHWC / token layout.  A "rows view" is any tensor whose last
dimension is dense (stride 1) and whose leading dimensions collapse to `rows` with one pitch
(stride(-2)); channel slices of a wider NHWC buffer (`buf[..., :64]`) are rows views, which is how
convs read from and write into concat buffers without copies.
"""
import ctypes

from . import modes as _modes  # (before torch: a misspelt SEGMIF_ variable then fails at once)

import torch  # noqa: E402

from . import _lib  # noqa: E402
from ._lib import ACT_GELU, ACT_NONE, ACT_PRELU, ACT_RELU  # noqa: E402,F401
from .guard import (Planes16Guard, active_guard, f16x3_enabled, finish_guarded, install_guard, range_fallbacks,  # noqa: E402,F401
                    range_stats, run_guarded, run_unguarded)

# The arithmetic-mode switches live in modes.py (one table: names, environment variables, values, what each selects).
# NB `ops.modes` is that module's CONTEXT MANAGER (`with ops.modes(conv3x3="fp32", linear="fp32"): ...`), `segmif_amd.modes` the
# module itself: `from .ops import modes` and `from . import modes` give different things.
_mode, modes = _modes.get, _modes.modes


def _switch(name):
    """-> (getter, setter) of one switch of the table, documented by its entry."""
    def getter():
        return _modes.get(name)

    def setter(mode):
        return _modes.set(name, mode)
    doc = next(m.doc for m in _modes.TABLE if m.name == name)
    getter.__doc__, setter.__doc__ = doc, doc + "  Returns the previous value."
    return getter, setter


conv3x3_mode, set_conv3x3_mode = _switch("conv3x3")
linear_mode, set_linear_mode = _switch("linear")
crosspath_mode, set_crosspath_mode = _switch("crosspath")
crosspath_arith, set_crosspath_arith = _switch("crosspath_arith")
attention_mode, set_attention_mode = _switch("attention")
mixffn_mode, set_mixffn_mode = _switch("mixffn")
pairs_mode, set_pairs_mode = _switch("pairs")
_, set_train_conv = _switch("train_conv")


def train_conv_f16():
    return _mode("train_conv") == "f16x3" and _mode("conv3x3") != "fp32"


def lazy_seg_mode():
    return _mode("lazy_seg") == "1"


def set_lazy_seg_mode(on):
    return _modes.set("lazy_seg", "1" if on else "0") == "1"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"segmif_amd: {name} must be a tensor on the MI355X device "
                           "(the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"segmif_amd: {name} must be float32, got {t.dtype}")
    return t


def rows_view(t, name="tensor"):
    """-> (rows, C, pitch). Validates that `t` is a rows view."""
    _req(t, name)
    if t.dim() < 2:
        raise RuntimeError(f"{name}: need at least 2 dims")
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        raise RuntimeError(f"{name}: last dim must be dense")
    ld = t.stride(-2)
    rows = t.shape[-2]
    expect = ld * t.shape[-2]
    for d in range(t.dim() - 3, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            raise RuntimeError(f"{name}: leading dims do not collapse to rows (shape {tuple(t.shape)}, "
                               f"strides {t.stride()})")
        expect *= t.shape[d]
        rows *= t.shape[d]
    return rows, t.shape[-1], ld


def aligned16(*tensors):
    """True when every given tensor (None is skipped) can take the kernels' 16-byte vector accesses: base pointer on a
    16-byte boundary and, for rows views, a pitch that is a multiple of four floats.  Parameters normally are (torch
    allocations are 512-byte aligned); views into a flattened parameter buffer or odd channel-slice offsets may not be."""
    for t in tensors:
        if t is None:
            continue
        if t.data_ptr() % 16 or (t.dim() >= 2 and t.stride(-2) % 4):
            return False
    return True


def pack_weight(w):
    """OIHW conv weight or (N, K) linear weight -> packed [N, Kp] (tap-major, channel-minor)."""
    _req(w, "weight")
    if w.dim() == 2:
        N, cin, kh, kw = w.shape[0], w.shape[1], 1, 1
    else:
        N, cin, kh, kw = w.shape
    w = w.detach().contiguous()
    kp = (kh * kw * cin + 15) // 16 * 16
    out = torch.empty((N, kp), device=w.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_pack_conv_weight(w.data_ptr(), out.data_ptr(), N, cin, kh, kw, _stream()),
               "segmif_pack_conv_weight")
    return out


class SplitWeight:
    """bf16x6 image of a packed 3x3 conv weight (segmif_conv3x3_split_pack): three bf16 planes per fp32
    weight in the streaming order of tile 14 (csrc/conv3x3_split.hip)."""
    __slots__ = ("data", "N", "cin", "f16")

    def __init__(self, data, N, cin, f16=False):
        self.data, self.N, self.cin, self.f16 = data, N, cin, f16  # f16: the f16x3 image (segmif_conv3x3_split16_pack)


def pack_weight_split(w):
    """OIHW 3x3 weight -> SplitWeight (the geometry limits of tile 14 are checked at launch)."""
    N, cin = w.shape[0], w.shape[1]
    packed = pack_weight(w)
    lib = _lib.load()
    nbytes = lib.segmif_conv3x3_split_weight_bytes(N, cin)
    if nbytes <= 0:
        raise RuntimeError(f"split packing needs Cin % 16 == 0, got Cin={cin}")
    out = torch.empty((nbytes,), device=w.device, dtype=torch.uint8)
    _lib.check(lib.segmif_conv3x3_split_pack(packed.data_ptr(), N, cin, packed.shape[1], out.data_ptr(), _stream()),
               "segmif_conv3x3_split_pack")
    return SplitWeight(out, N, cin)


def pack_weight_split16(w):
    """OIHW 3x3 weight -> SplitWeight in the f16x3 form (rows scaled by powers of two, half planes W0 | Wl | 2^-11 W0): the
    training path's convs; conv2d then needs in_amax= (the input's range slots)."""
    N, cin = w.shape[0], w.shape[1]
    packed = pack_weight(w)
    lib = _lib.load()
    nbytes = lib.segmif_conv3x3_split16_weight_bytes(N, cin)
    if nbytes <= 0:
        raise RuntimeError(f"split packing needs Cin % 16 == 0, got Cin={cin}")
    out = torch.empty((nbytes,), device=w.device, dtype=torch.uint8)
    _lib.check(lib.segmif_conv3x3_split16_pack(packed.data_ptr(), N, cin, packed.shape[1], out.data_ptr(), _stream()),
               "segmif_conv3x3_split16_pack")
    return SplitWeight(out, N, cin, f16=True)


RANGE_WORDS = 8  # words per range slot: producers spread their one-atomic-per-workgroup over them, consumers take the maximum


def range_slots(n, device):
    """n zeroed range slots (n, RANGE_WORDS) int32: slot i receives max |.| of one tensor / channel block as IEEE bit patterns
    (amax_rows, conv2d(out_amax=)); a consumer passes the slots covering its input, flattened, as in_amax."""
    return torch.zeros((n, RANGE_WORDS), device=device, dtype=torch.int32)


def amax_rows(x, slot):
    """Fold max |x| of a rows view into slot (a contiguous int32 device tensor of 1, 2, 4 .. 64 words; zero it first)."""
    rows, C, ld = rows_view(x, "x")
    _lib.check(_lib.load().segmif_amax_f32(x.data_ptr(), rows, C, ld, slot.data_ptr(), slot.numel(), _stream()), "segmif_amax_f32")


def pack_conv3x3(w):
    """Packing for a stride-1 'same' 3x3 conv (dilation 1 or 2): the split image when the mode and the
    shape allow it, the fp32 packing otherwise.  Cache entries must be keyed on conv3x3_mode()."""
    if _mode("conv3x3") in ("bf16x6", "planes", "planes16") and w.dim() == 4 and w.shape[2] == 3 and w.shape[3] == 3 and w.shape[1] % 16 == 0 \
            and 16 <= w.shape[0] <= 256:
        return pack_weight_split(w)
    return pack_weight(w)


class Planes:
    """A planes buffer (include/segmif_hip.h, segmif_planes_*): `chunks` 16-channel chunk images per batch
    element, each activation stored as three bf16 planes (guard=None) or, with a Planes16Guard, as a pair of
    halves (f16x3); zero border already cleared."""
    __slots__ = ("data", "B", "H", "W", "chunks", "guard", "first")

    def __init__(self, B, H, W, chunks, device, guard=None):
        lib = _lib.load()
        self.B, self.H, self.W, self.chunks, self.guard, self.first = B, H, W, chunks, guard, 0
        nbytes, zero = (lib.segmif_planes_bytes, lib.segmif_planes_zero_border) if guard is None else \
            (lib.segmif_planes16_bytes, lib.segmif_planes16_zero_border)
        self.data = torch.empty((nbytes(B, H, W, chunks),), device=device, dtype=torch.uint8)
        _lib.check(zero(self.data.data_ptr(), B, H, W, chunks, _stream()), "segmif_planes_zero_border")

    @property
    def f16(self):
        return self.guard is not None

    def at(self, chunk0):
        """The same buffer addressed from chunk image `chunk0` on: producers and consumers number chunks relative to the
        base pointer they are given (the per-batch-element stride stays `chunks` images)."""
        if not 0 <= chunk0 < self.chunks:
            raise RuntimeError(f"planes: chunk {chunk0} outside a buffer of {self.chunks}")
        v = object.__new__(Planes)
        v.B, v.H, v.W, v.chunks, v.guard, v.first = self.B, self.H, self.W, self.chunks, self.guard, self.first + chunk0
        v.data = self.data[chunk0 * self.chunk_bytes:]
        return v

    def need(self, n, what):
        """n chunk images counted from this view's base must exist (the C side only knows the buffer's total)."""
        if self.first + n > self.chunks:
            raise RuntimeError(f"{what}: needs {n} chunk images from chunk {self.first} of a {self.chunks}-chunk planes buffer")

    @property
    def chunk_bytes(self):
        hp, wp = (self.H + 7) // 8 * 8 + 4, (self.W + 31) // 32 * 32 + 4
        return hp * wp * (64 if self.f16 else 96)

    def load_f32(self, x, chunk0=0):
        """x: (B, H, W, C) rows view, C % 16 == 0 -> chunks [chunk0, chunk0 + C/16)."""
        _, C, ldx = rows_view(x, "x")
        if tuple(x.shape[:3]) != (self.B, self.H, self.W) or C % 16:
            raise RuntimeError(f"planes: x shape {tuple(x.shape)} does not fit ({self.B}, {self.H}, {self.W}, 16k)")
        self.need(chunk0 + C // 16, "planes.load_f32")
        lib = _lib.load()
        if self.guard is None:
            _lib.check(lib.segmif_planes_from_f32(x.data_ptr(), ldx, self.data.data_ptr(), self.B, self.H, self.W,
                                                  self.chunks, chunk0, C // 16, _stream()), "segmif_planes_from_f32")
        else:
            amax, nimg = self.guard.slot(self.B)
            _lib.check(lib.segmif_planes16_from_f32(x.data_ptr(), ldx, self.data.data_ptr(), self.B, self.H, self.W,
                                                    self.chunks, chunk0, C // 16, amax, nimg, _stream()),
                       "segmif_planes16_from_f32")
        return self


class PlanesWeight:
    """segmif_planes_pack_weight (f16: segmif_planes16_pack_weight) image of a 3x3 (taps = 9, N = 32) or 1x1 (taps = 1,
    N = 64) weight."""
    __slots__ = ("data", "N", "cin", "taps", "f16")

    def __init__(self, data, N, cin, taps, f16=False):
        self.data, self.N, self.cin, self.taps, self.f16 = data, N, cin, taps, f16


def pack_weight_planes(w, f16=False):
    """OIHW 3x3 / 1x1 conv weight (or a Linear weight) -> PlanesWeight (f16: the f16x3 image with its row scales)."""
    N, cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
    packed = pack_weight(w)
    lib = _lib.load()
    nbytes = (lib.segmif_planes16_weight_bytes if f16 else lib.segmif_planes_weight_bytes)(N, cin, taps)
    if nbytes <= 0:
        raise RuntimeError(f"planes packing needs N % 32 == 0, Cin % 16 == 0, 3x3 or 1x1; got {tuple(w.shape)}")
    out = torch.empty((nbytes,), device=w.device, dtype=torch.uint8)
    fn = lib.segmif_planes16_pack_weight if f16 else lib.segmif_planes_pack_weight
    _lib.check(fn(packed.data_ptr(), N, cin, taps, packed.shape[1], out.data_ptr(), _stream()), "segmif_planes_pack_weight")
    return PlanesWeight(out, N, cin, taps, f16)


def pack_weight_planes16(w):
    return pack_weight_planes(w, f16=True)


def conv3x3_planes(planes, cin, wt, *, dil, bias=None, act=ACT_NONE, prelu=None, out_chunk0=None, out=None, tail=None,
                   tag=None):
    """3x3 'same' conv (dilation 1 | 2, 32 outputs) over the first `cin` channels of a Planes buffer.
    out_chunk0: write the result as chunks [out_chunk0, out_chunk0 + 2) of the same buffer; out: optional fp32
    (B, H, W, 32) rows view; tail = (w1 PlanesWeight(64, cin + 32, 1), bias1, res, out1, act1[, res_from_planes]): the fused
    1x1 conv out1 = res + act1(W1 . [input | result] + bias1); res_from_planes (f16x3, res None): the residual is the input's
    own chunks 0..3 (hi + 2^-11 lo) - the fp32 tensor behind them then needs no writer and no reader."""
    if not isinstance(wt, PlanesWeight) or (wt.N, wt.cin, wt.taps, wt.f16) != (32, cin, 9, planes.f16):
        raise RuntimeError("conv3x3_planes: weight image does not fit")
    planes.need(max(cin // 16, (out_chunk0 + 2) if out_chunk0 is not None else 0), "conv3x3_planes")
    d = _lib.SegmifConvPlanes()
    d.planes_in, d.wt = planes.data.data_ptr(), wt.data.data_ptr()
    d.B, d.H, d.W, d.cin, d.dil = planes.B, planes.H, planes.W, cin, dil
    d.in_chunks = d.out_chunks = planes.chunks
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.prelu = _req(prelu, "prelu").data_ptr() if prelu is not None else None
    d.act = act
    if out_chunk0 is not None:
        d.planes_out, d.out_chunk0 = planes.data.data_ptr(), out_chunk0
    if out is not None:
        rows, oc, ldo = rows_view(out, "out")
        if tuple(out.shape) != (planes.B, planes.H, planes.W, 32):
            raise RuntimeError("conv3x3_planes: out shape mismatch")
        d.out, d.ldo = out.data_ptr(), ldo
    if tail is not None:
        w1, bias1, res, out1, act1 = tail[:5]
        if len(tail) > 5 and tail[5]:  # residual = the conv's own input chunks 0..3 (f16x3 planes only), no fp32 tensor
            if res is not None or not planes.f16:
                raise RuntimeError("conv3x3_planes: res_from_planes needs f16x3 planes and no fp32 residual")
            d.res_from_planes = 1
        if not isinstance(w1, PlanesWeight) or (w1.N, w1.cin, w1.taps, w1.f16) != (64, cin + 32, 1, planes.f16):
            raise RuntimeError("conv3x3_planes: tail weight image does not fit")
        _, c1, ldo1 = rows_view(out1, "out1")
        if tuple(out1.shape) != (planes.B, planes.H, planes.W, 64):
            raise RuntimeError("conv3x3_planes: out1 shape mismatch")
        d.w1, d.out1, d.ldo1, d.act1 = w1.data.data_ptr(), out1.data_ptr(), ldo1, act1
        d.bias1 = _req(bias1, "bias1").data_ptr() if bias1 is not None else None
        if res is not None:
            _, rc, ldr = rows_view(res, "res")
            if tuple(res.shape) != (planes.B, planes.H, planes.W, 64):
                raise RuntimeError("conv3x3_planes: res shape mismatch")
            d.res, d.ldr = res.data_ptr(), ldr
    lib = _lib.load()
    amax, nimg = planes.guard.slot(planes.B) if planes.f16 else (None, 1)

    def go():
        if planes.f16:
            _lib.check(lib.segmif_conv3x3_planes_f16x3(ctypes.byref(d), amax, nimg, _stream()), "segmif_conv3x3_planes_f16x3")
        else:
            _lib.check(lib.segmif_conv3x3_planes_bf16x6(ctypes.byref(d), _stream()), "segmif_conv3x3_planes_bf16x6")

    if _timer is not None and tag is not None and tag == _timer.tag:
        _timer.bracket(go, 2.0 * planes.B * planes.H * planes.W * 32 * 9 * cin)
    else:
        go()


class GemmSplitWeight:
    """segmif_gemm_split_pack image of an (N, K) Linear weight (bf16x6 dense GEMM, csrc/gemm_split.hip); half: the
    segmif_gemm_split16_pack image of the same weight (f16x3) or None; pairs: (r5) the two-plane segmif_gemm_pairs_pack image
    (f16x3 with the A operand pre-split by its producer, csrc/gemm_pairs.hip) or None."""
    __slots__ = ("data", "N", "K", "half", "pairs")

    def __init__(self, data, N, K, half=None, pairs=None):
        self.data, self.N, self.K, self.half, self.pairs = data, N, K, half, pairs


GEMM_SPLIT_MIN_ROWS = 2048  # below this the 128-row tiles leave the chip idle; the fp32 tiles with split-K win
LN_SUB = 8             # rows of range slots a pairs LayerNorm spreads its reports over (csrc/rowops.hip, layernorm_pairs_kernel)
PAIRS_MIN_ROWS = 8192  # below this a transformer block's GEMMs stay on round 4's kernels (fp32 tiles with split-K for the short ones)


class Pairs:
    """Tokens (B, N, C) in PAIRS format: every row is C / 16 groups of 64 bytes, [16 hi halves | 16 lo halves], x = hi + 2^-11 lo
    (include/segmif_hip.h, segmif_gemm_pairs_f32).  `.t` is a float32 tensor of the LOGICAL shape whose storage holds those
    bytes (the byte count is fp32's): only the pairs kernels may read it.  Produced inside a guarded scope only - its producer
    has folded max |x| into the range slots."""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    @property
    def shape(self):
        return self.t.shape


def pairs_block_ok(x):
    """True when a transformer block over tokens x (B, N, C) should run its Linears on gemm_pairs: inside a guarded f16x3 scope,
    C a multiple of 16 and at least 128 (a 128-column tile), enough rows to fill the chip."""
    return (_mode("pairs") == "on" and active_guard() is not None and _mode("linear") == "f16x3" and x.dim() == 3 and x.is_contiguous()
            and x.shape[2] >= 128 and x.shape[2] % 16 == 0 and x.shape[0] * x.shape[1] >= PAIRS_MIN_ROWS and x.data_ptr() % 16 == 0)


def _pack_pairs(wc, N, K):
    """The two-plane weight image of gemm_pairs for a contiguous fp32 (N, K) matrix, or None when the kernel cannot take it."""
    if _mode("pairs") != "on" or K % 16 or N % 4 or N < 128:
        return None
    lib = _lib.load()
    img = torch.empty((lib.segmif_gemm_pairs_weight_bytes(N, K),), device=wc.device, dtype=torch.uint8)
    _lib.check(lib.segmif_gemm_pairs_pack(wc.data_ptr(), N, K, K, img.data_ptr(), _stream()), "segmif_gemm_pairs_pack")
    return img


def _need_guard(why="PAIRS tensors exist inside a guarded f16x3 scope only (ops.run_guarded / install_guard)"):
    guard = active_guard()
    if guard is None:
        raise RuntimeError(why)
    return guard


def _guard_slot(images):
    return _need_guard().slot(images)


def pairs_from_f32(x):
    """fp32 tokens (B, N, C) -> Pairs (a producer for tensors whose own kernel has no pairs epilogue; tests)."""
    rows, C, ldx = rows_view(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    images = x.shape[0] if x.dim() == 3 else None
    amax, nimg = _guard_slot(images)
    _lib.check(_lib.load().segmif_pairs_from_f32(x.data_ptr(), ldx, out.data_ptr(), 4 * C, rows, C, amax, nimg, _stream()),
               "segmif_pairs_from_f32")
    return Pairs(out)


def pairs_to_f32(xp):
    rows, C, ld = rows_view(xp.t, "pairs")
    out = torch.empty_like(xp.t)
    _lib.check(_lib.load().segmif_pairs_to_f32(xp.t.data_ptr(), 4 * ld, out.data_ptr(), C, rows, C, _stream()), "segmif_pairs_to_f32")
    return out


def layernorm_pairs(x, gamma, beta, eps):
    """LayerNorm over the last dim of contiguous tokens (B, N, C), C % 16 == 0, written as Pairs (no fp32 copy)."""
    rows, C, ldx = rows_view(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    if not aligned16(gamma, beta):
        gamma, beta = gamma.detach().clone(), beta.detach().clone()
    guard = _need_guard()
    # (the kernel's waves are short and many: its range reports are spread over LN_SUB consecutive rows of slots)
    amax, nimg, nsub = guard.slot_rows(x.shape[0] if x.dim() == 3 else None, LN_SUB)
    _lib.check(_lib.load().segmif_layernorm_pairs_f32(x.data_ptr(), _req(gamma).data_ptr(), _req(beta).data_ptr(), out.data_ptr(),
                                                      rows, C, ldx, C, float(eps), amax, nimg, nsub, guard.images, _stream()),
               "segmif_layernorm_pairs_f32")
    return Pairs(out)


def dwconv3x3_gelu_pairs(x, w9, bias, H, W):
    """dwconv3x3_gelu with the result as Pairs (the A operand of fc2)."""
    _req(x, "x")
    if not x.is_contiguous() or x.dim() != 3 or x.shape[1] != H * W or x.shape[2] % 16:
        raise RuntimeError("dwconv3x3_gelu_pairs expects contiguous (B, H*W, C) with C % 16 == 0")
    B, _, C = x.shape
    out = torch.empty_like(x)
    amax, nimg = _guard_slot(B)
    _side("dwconv", lambda: _lib.check(_lib.load().segmif_dwconv3x3_gelu_pairs_f32(
        x.data_ptr(), _req(w9).data_ptr(), _req(bias).data_ptr(), out.data_ptr(), B, H, W, C, amax, nimg, _stream()),
        "segmif_dwconv3x3_gelu_pairs_f32"), 8.0 * x.numel())
    return Pairs(out)


def linear_pairs(xp, packs, N, *, bias=None, act=ACT_NONE, res=None, out=None, patch=None, tile_rows=0):
    """out = res + act(x @ W^T + bias) for x in PAIRS format and packs = pack_linear(W) / pack_sr_conv(W) (whose GemmSplitWeight
    carries the pairs image).  patch = (k, stride, pad): x is a contiguous (B, H, W, C) pairs image and the rows are its k x k
    patches (Attention's spatial-reduction conv) -> (B, OH, OW, N)."""
    split = packs[1]
    if split is None or split.pairs is None:
        raise RuntimeError("linear_pairs: the weight carries no pairs image (N >= 128, N % 4 == 0, K % 16 == 0, SEGMIF_GEMM_PAIRS=on)")
    x = xp.t
    d = _lib.SegmifGemmPairs()
    if patch is not None:
        k, st, pad = patch
        B, H, W, C = x.shape
        if not x.is_contiguous():
            raise RuntimeError("linear_pairs: patch mode needs a contiguous (B, H, W, C) image")
        OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        rows, K = B * OH * OW, k * k * C
        d.patch_k, d.patch_st, d.patch_pad, d.patch_H, d.patch_W, d.patch_C = k, st, pad, H, W, C
        d.lda_bytes = 4 * C
        oshape = (B, OH, OW, N)
    else:
        rows, K, lda = rows_view(x, "x")
        d.lda_bytes = 4 * lda
        oshape = x.shape[:-1] + (N,)
    if (split.N, split.K) != (N, K):
        raise RuntimeError(f"linear_pairs: weight {split.N}x{split.K} does not fit N {N}, K {K}")
    if not (_vec4(out) and _vec4(res) and _vec4(bias)):
        raise RuntimeError("linear_pairs: out / res / bias must allow 16-byte accesses")
    if out is None:
        out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    orow, oc, ldo = rows_view(out, "out")
    if orow != rows or oc != N:
        raise RuntimeError(f"linear_pairs: out shape {tuple(out.shape)} does not match rows={rows}, N={N}")
    d.a, d.w, d.out = x.data_ptr(), split.pairs.data_ptr(), out.data_ptr()
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.M, d.N, d.K, d.ldo, d.act, d.tile_rows = rows, N, K, ldo, act, tile_rows
    if res is not None:
        rrow, rc, ldr = rows_view(res, "res")
        if rc != N or rrow != rows:
            raise RuntimeError("residual shape mismatch")
        d.res, d.ldr = res.data_ptr(), ldr
    _lib.check(_lib.load().segmif_gemm_pairs_f32(ctypes.byref(d), _stream()), "segmif_gemm_pairs_f32")
    return out


def _pack_gemm_split(wc, N, K, half):
    """GemmSplitWeight of a contiguous fp32 (N, K) matrix: the bf16x6 image and, with half, the f16x3 and pairs images."""
    lib = _lib.load()
    out = torch.empty((lib.segmif_gemm_split_weight_bytes(N, K),), device=wc.device, dtype=torch.uint8)
    _lib.check(lib.segmif_gemm_split_pack(wc.data_ptr(), N, K, K, out.data_ptr(), _stream()), "segmif_gemm_split_pack")
    img16 = pimg = None
    if half:
        img16 = torch.empty((lib.segmif_gemm_split16_weight_bytes(N, K),), device=wc.device, dtype=torch.uint8)
        _lib.check(lib.segmif_gemm_split16_pack(wc.data_ptr(), N, K, K, img16.data_ptr(), _stream()), "segmif_gemm_split16_pack")
        pimg = _pack_pairs(wc, N, K)
    return GemmSplitWeight(out, N, K, img16, pimg)


def pack_linear(w, half=None):
    """(N, K) Linear weight -> (fp32 packing, GemmSplitWeight or None).  Cache entries must be keyed on linear_mode().
    half: also build the f16x3 image (default: when linear_mode() is 'f16x3'; training passes False - it re-packs per step
    and never runs under a range guard)."""
    packed = pack_weight(w)
    N, K = w.shape[0], w.shape[1]
    if _mode("linear") == "fp32" or w.dim() != 2 or K % 32 or N < 32:
        return packed, None
    return packed, _pack_gemm_split(w.detach().contiguous(), N, K, _mode("linear") == "f16x3" if half is None else half)


def linear_wants_split(rows, N, K):
    """The size rule of linear_auto, for callers that would rather not build a split weight image they will not use."""
    return _mode("linear") != "fp32" and rows >= GEMM_SPLIT_MIN_ROWS and N >= 128 and N % 4 == 0 and K % 32 == 0


def _vec4(t):  # the split GEMM's 16-byte epilogue accesses
    return t is None or (t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.stride(-2) % 4 == 0))


def _gemm_split(a_ptr, rows, K, lda, split, N, bias, act, res, out, images, patch=None):
    """Launch of the split-operand GEMM (f16x3 inside a guarded scope when the weight carries its half image, bf16x6
    otherwise).  images: how many whole images the rows are (their range slots), or None; patch = (sr, H, W) or None."""
    orow, oc, ldo = rows_view(out, "out")
    if orow != rows or oc != N or (split.N, split.K) != (N, K):
        raise RuntimeError(f"split GEMM: shapes do not fit (rows {rows}/{orow}, N {N}/{oc}, weight {split.N}x{split.K})")
    guard = active_guard()
    use16 = split.half is not None and guard is not None
    d = _lib.SegmifGemmSplit()
    d.a, d.w, d.out = a_ptr, (split.half if use16 else split.data).data_ptr(), out.data_ptr()
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.M, d.N, d.K, d.lda, d.ldo, d.act = rows, N, K, lda, ldo, act
    if patch is not None:
        d.patch_k, d.patch_st, d.patch_pad, d.patch_H, d.patch_W = patch
    if res is not None:
        rrow, rc, ldr = rows_view(res, "res")
        if rc != N or rrow != rows:
            raise RuntimeError("residual shape mismatch")
        d.res, d.ldr = res.data_ptr(), ldr
    if use16:
        amax, nimg = guard.slot(images if images and rows % images == 0 else None)
        _lib.check(_lib.load().segmif_gemm_split16_f32(ctypes.byref(d), amax, nimg, _stream()), "segmif_gemm_split16_f32")
    else:
        _lib.check(_lib.load().segmif_gemm_split_f32(ctypes.byref(d), _stream()), "segmif_gemm_split_f32")
    return out


def linear_auto(x, packs, N, *, bias=None, act=ACT_NONE, res=None, out=None):
    """out = res + act(x @ W^T + bias) with packs = pack_linear(W): the split-operand GEMM for tall problems (f16x3 inside
    a guarded scope when the weight carries its half image, bf16x6 otherwise), the fp32 tiles (with split-K) for short ones."""
    packed, split = packs
    rows, K, lda = rows_view(x, "x")
    # (N < 128 would leave half of the 128-column tile idle: measured slower than the fp32 64-column tiles)
    if split is None or rows < GEMM_SPLIT_MIN_ROWS or N < 128 or N % 4 or lda % 4 or x.data_ptr() % 16:
        return linear(x, packed, N, bias=bias, act=act, res=res, out=out)
    if not (_vec4(out) and _vec4(res) and _vec4(bias)):
        return linear(x, packed, N, bias=bias, act=act, res=res, out=out)
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32)
    # rows of a (B, n, K) token tensor are B whole images: each reports to its own range slot
    images = x.shape[0] if x.dim() == 3 and rows == x.shape[0] * x.shape[1] else None
    return _gemm_split(x.data_ptr(), rows, K, lda, split, N, bias, act, res, out, images)


def pack_sr_conv(w):
    """(N, C, k, k) weight of a conv the split GEMM can take in patch mode (Attention's spatial-reduction conv: kernel =
    stride; the overlapping patch embeds of stages 2-4) -> (fp32 packing for the igemm tiles, GemmSplitWeight over K = k * k * C
    in (ky, kx, c) order, or None).  Cache entries must be keyed on linear_mode()."""
    packed = pack_weight(w)
    N, C, k = w.shape[0], w.shape[1], w.shape[2]
    K = k * k * C
    if _mode("linear") == "fp32" or w.dim() != 4 or w.shape[3] != k or C % 32 or N < 32 or packed.shape[1] != K:
        return packed, None
    return packed, _pack_gemm_split(packed, N, K, _mode("linear") == "f16x3")


def patch_conv_auto(x, packs, N, k, stride, pad, *, bias=None):
    """A k x k conv (stride, zero padding) on a contiguous NHWC batch x (B, H, W, C) -> (B, OH, OW, N): the split-operand GEMM
    reading its A rows straight out of the image (patch mode: no gather pass, taps outside the image read as zeros) when the
    problem is tall and wide enough and C % 32 == 0, the strided implicit-GEMM tiles otherwise."""
    packed, split = packs
    B, H, W, C = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    rows = B * OH * OW
    if split is None or rows < GEMM_SPLIT_MIN_ROWS or N < 128 or N % 4 or C % 32 or not x.is_contiguous() or x.data_ptr() % 16 \
            or not _vec4(bias) or _mode("sr_conv") == "igemm":
        return conv2d(x, packed, N, k, stride=stride, pad=pad, bias=bias)
    out = torch.empty((B, OH, OW, N), device=x.device, dtype=torch.float32)
    return _gemm_split(x.data_ptr(), rows, k * k * C, C, split, N, bias, ACT_NONE, None, out, B, patch=(k, stride, pad, H, W))


def sr_conv_auto(x, packs, N, sr, *, bias=None):
    """The spatial-reduction conv of Attention (kernel = stride = sr, no padding): patch_conv_auto(x, packs, N, sr, sr, 0)."""
    return patch_conv_auto(x, packs, N, sr, sr, 0, bias=bias)


def mixffn_fusable(C, hidden):
    """The one-kernel Mix-FFN (csrc/mixffn.hip) exists for C = 64 | 128 with the 4x hidden width, on f16x3 operands: it runs
    inside a guarded scope only (the bf16x6 chain is what a tripped pair is repeated on)."""
    return _mode("mixffn") == "fused" and C in (64, 128) and hidden == 4 * C and _mode("linear") == "f16x3" and active_guard() is not None


def pack_mixffn(w1, b1, dw9, dwb, w2):
    """fc1 (4C, C) weight + bias, depthwise weight as pack_dw_weight's [9][4C] + bias, fc2 (C, 4C) weight -> the
    segmif_mixffn_pack image (uint8 tensor): one contiguous block per 32 hidden channels."""
    for t, nm in ((w1, "fc1 weight"), (b1, "fc1 bias"), (dw9, "dw weight"), (dwb, "dw bias"), (w2, "fc2 weight")):
        _req(t, nm)
    C = w1.shape[1]
    if tuple(w1.shape) != (4 * C, C) or tuple(w2.shape) != (C, 4 * C) or tuple(dw9.shape) != (9, 4 * C) \
            or b1.numel() != 4 * C or dwb.numel() != 4 * C:
        raise RuntimeError(f"pack_mixffn: shapes do not fit C = {C}: {tuple(w1.shape)}, {tuple(w2.shape)}, {tuple(dw9.shape)}")
    lib = _lib.load()
    nbytes = lib.segmif_mixffn_weight_bytes(C)
    if nbytes <= 0:
        raise RuntimeError(f"pack_mixffn: C must be 64 or 128, got {C}")
    out = torch.zeros((nbytes,), device=w1.device, dtype=torch.uint8)
    c = lambda t: t.detach().contiguous()
    w1c, b1c, d9c, dbc, w2c = c(w1), c(b1), c(dw9), c(dwb), c(w2)
    _lib.check(lib.segmif_mixffn_pack(w1c.data_ptr(), b1c.data_ptr(), d9c.data_ptr(), dbc.data_ptr(), w2c.data_ptr(), C,
                                      out.data_ptr(), _stream()), "segmif_mixffn_pack")
    return out


def mixffn_fused(x, ln, wimg, b2, H, W):
    """out = x + fc2(GELU(dwconv3x3(fc1(LayerNorm(x))))) in one launch: x contiguous tokens (B, H*W, C), ln = (gamma, beta,
    eps), wimg = pack_mixffn(...), b2 = fc2's bias.  Needs an active range guard (two slot rows: the normalised tokens and
    the GELU output).  Returns a NEW tensor (halo tokens of x are read by neighbouring workgroups, so the update cannot be
    in place)."""
    _req(x, "x")
    if x.dim() != 3 or not x.is_contiguous() or x.shape[1] != H * W:
        raise RuntimeError("mixffn_fused expects contiguous (B, H*W, C) tokens")
    guard = _need_guard("mixffn_fused runs on f16x3 operands: call it inside ops.run_guarded (or install_guard)")
    B, _, C = x.shape
    lib = _lib.load()
    if wimg.dtype != torch.uint8 or wimg.numel() != lib.segmif_mixffn_weight_bytes(C):
        raise RuntimeError("mixffn_fused: wimg must be the pack_mixffn image for this C")
    out = torch.empty_like(x)
    d = _lib.SegmifMixFfn()
    d.x, d.out, d.wimg = x.data_ptr(), out.data_ptr(), wimg.data_ptr()
    d.ln_gamma, d.ln_beta, d.ln_eps = _req(ln[0]).data_ptr(), _req(ln[1]).data_ptr(), float(ln[2])
    d.b2 = _req(b2).data_ptr()
    d.B, d.H, d.W, d.C = B, H, W, C
    d.amax_a, n1 = guard.slot(B)
    d.amax_g, n2 = guard.slot(B)
    d.amax_images = n1
    _side("mixffn", lambda: _lib.check(lib.segmif_mixffn_f16x3(ctypes.byref(d), _stream()), "segmif_mixffn_f16x3"),
          8.0 * x.numel())
    return out


class LaunchTimer:
    """Brackets tagged kernel launches with HIP events on the launch stream (torch's current
    stream) so bench.py can report a kernel's average duration live.  `work` is whatever the caller wants averaged
    beside the time: flops for the matrix-pipe kernels, algorithmic bytes for the bandwidth-bound ones."""

    def __init__(self, tag):
        self.tag = tag
        self.events = []  # (start, end, work)

    def bracket(self, fn, work):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        self.events.append((s, e, work))

    def summary(self):
        """-> (launches, mean ms per launch, mean work per launch); call after a device sync."""
        if not self.events:
            return 0, 0.0, 0.0
        ms = [s.elapsed_time(e) for s, e, _ in self.events]
        return len(ms), sum(ms) / len(ms), sum(f for _, _, f in self.events) / len(ms)


_timer = None      # the dominant kernel's timer (bench.py's `roofline` object)
_side_timers = {}  # tag -> LaunchTimer for the bandwidth-bound kernels bench.py also reports


def set_launch_timer(timer, side=None):
    """timer: LaunchTimer for the tagged matrix-pipe launches (or None); side: optional {tag: LaunchTimer} for the
    bandwidth-bound kernels ('dwconv', 'cp_gram', 'cp_tail', 'bilinear')."""
    global _timer, _side_timers
    _timer = timer
    _side_timers = dict(side or {})


def launch_timer_active():
    return _timer is not None or bool(_side_timers)


def _side(tag, fn, nbytes):
    t = _side_timers.get(tag)
    if t is None:
        fn()
    else:
        t.bracket(fn, float(nbytes))


def _igemm(desc, tag=None, dev="cuda"):
    lib = _lib.load()
    need = lib.segmif_igemm_workspace_floats(ctypes.byref(desc))
    ws = None
    if need > 0:  # split-K scratch for problems whose tile grid would leave most CUs idle
        ws = torch.empty((need,), device=dev, dtype=torch.float32)
        desc.workspace, desc.workspace_floats = ws.data_ptr(), need

    def go():
        _lib.check(lib.segmif_igemm_f32(ctypes.byref(desc), _stream()), "segmif_igemm_f32")

    if _timer is not None and tag is not None and tag == _timer.tag:
        _timer.bracket(go, 2.0 * desc.M * max(desc.nz, 1) * desc.N * desc.K)
    else:
        go()


def linear(x, wt, N, *, bias=None, act=ACT_NONE, prelu=None, res=None, out=None, x2=None, tile=-1,
           batched_weight=False, ln=None, mask=None):
    """out = res + act(x @ wt^T + bias).  x: rows view (..., K); wt: packed (N, Kp).
    mask: rows view shaped like out; out = mask > 0 ? (that) : 0 - a gradient written through a ReLU whose output mask is.
    x2: optional second source (..., K2): A = [x | x2] along K (no concat materialised).
    batched_weight: wt is (B, N, Kp) with one weight per leading batch index of x (x.dim() == 3)."""
    if ln is not None and not aligned16(out, res, bias, ln[0], ln[1]):
        # the fused LayerNorm epilogue only exists in its 16-byte form: run the GEMM and the normalisation apart
        y = linear(x, wt, N, bias=bias, act=act, prelu=prelu, res=res, out=out, x2=x2, tile=tile, batched_weight=batched_weight)
        return layernorm(y, ln[0], ln[1], ln[2], out=y)
    if mask is not None and ln is not None:
        raise RuntimeError("linear: mask= and ln= exclude each other")
    rows, K1, lda = rows_view(x, "x")
    K = K1
    d = _lib.SegmifIgemm()
    d.in_ = x.data_ptr()
    if x2 is not None:
        rows2, K2, lda2 = rows_view(x2, "x2")
        if rows2 != rows:
            raise RuntimeError("x and x2 row counts differ")
        d.in2, d.lda2, d.K1 = x2.data_ptr(), lda2, K1
        K = K1 + K2
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32)
    orow, oc, ldo = rows_view(out, "out")
    if orow != rows or oc != N:
        raise RuntimeError(f"out shape {tuple(out.shape)} does not match rows={rows}, N={N}")
    _req(wt, "wt")
    kp = (K + 15) // 16 * 16
    nz = 1
    if batched_weight:
        if x.dim() != 3 or wt.dim() != 3 or wt.shape[0] != x.shape[0] or not wt.is_contiguous():
            raise RuntimeError("batched_weight needs x (B, n, K) and contiguous wt (B, N, Kp)")
        nz = x.shape[0]
        rows = x.shape[1]
        d.in_zstride = x.stride(0)
        d.wt_zstride = wt.stride(0)
        d.out_zstride = out.stride(0)
        if x2 is not None:
            d.in2_zstride = x2.stride(0)
    if tuple(wt.shape[-2:]) != (N, kp) or not wt.is_contiguous():
        raise RuntimeError(f"packed weight must be contiguous (..., {N}, {kp}), got {tuple(wt.shape)}")
    d.wt = wt.data_ptr()
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.prelu = _req(prelu, "prelu").data_ptr() if prelu is not None else None
    d.out = out.data_ptr()
    if res is not None:
        rrow, rc, ldr = rows_view(res, "res")
        if rc != N or rrow != orow:
            raise RuntimeError("residual shape mismatch")
        d.res, d.ldr = res.data_ptr(), ldr
        if batched_weight:
            d.res_zstride = res.stride(0)
    if mask is not None:
        mrow, mc, ldm = rows_view(mask, "mask")
        if mc != N or mrow != orow:
            raise RuntimeError("mask shape mismatch")
        d.relu_mask, d.ld_mask = mask.data_ptr(), ldm
        if batched_weight:
            d.mask_zstride = mask.stride(0)
    d.M, d.N, d.K = rows, N, K
    d.lda, d.ldo = lda, ldo
    d.H = d.OH = 1
    d.W = d.OW = 1
    d.Cin = K
    d.KH = d.KW = d.stride = d.dil = 1
    d.pad = 0
    d.act, d.nz, d.tile = act, nz, tile
    if ln is not None:  # (gamma, beta, eps): LayerNorm over the N = 64 outputs fused into the epilogue
        d.ln_gamma, d.ln_beta, d.ln_eps = _req(ln[0]).data_ptr(), _req(ln[1]).data_ptr(), float(ln[2])
    _igemm(d, dev=x.device)
    return out


def conv2d(x, wt, N, k, *, stride=1, pad=0, dil=1, bias=None, act=ACT_NONE, prelu=None, res=None, out=None,
           tile=-1, tag=None, planes=None, planes_chunk0=0, ln=None, planes_only=False, mask=None, in_amax=None, out_amax=None):
    """NHWC convolution.  x: (B, H, W, Cin) rows view (may be a channel slice of a wider buffer);
    wt packed (N, Kp); out: (B, OH, OW, N) rows view (may be a channel slice) or None.
    planes: optional ops.Planes of the output geometry that also receives the result, split, as chunks
    [planes_chunk0, planes_chunk0 + N / 16) (fp32-packed weights only).
    ln = (gamma, beta, eps): LayerNorm over the N = 64 output channels in the conv's epilogue (conv_ln_fusable).
    planes_only: write the planes copy and nothing else (returns None): the fp32 tensor has no reader.
    mask: (B, OH, OW, N) rows view; out = mask > 0 ? act(conv + bias) + res : 0 (split 3x3 weights only: the DRDB backward).
    in_amax: int32 device tensor of range words covering the input's channel blocks (required by f16x3 split weights);
    out_amax: contiguous int32 device tensor of 1, 2, 4 .. 64 words receiving max |out| (split weights only)."""
    if x.dim() != 4:
        raise RuntimeError("conv2d expects (B, H, W, C)")
    if mask is not None and (planes is not None or ln is not None or not isinstance(wt, SplitWeight)):
        raise RuntimeError("conv2d: mask= needs split 3x3 weights and no planes / LayerNorm epilogue")
    if planes_only:
        if planes is None or out is not None or res is not None or ln is not None or isinstance(wt, SplitWeight):
            raise RuntimeError("conv2d: planes_only needs a planes buffer, fp32-packed weights and no fp32 output / residual / LayerNorm")
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
        OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
        OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
        return _conv2d_planes_only(x, wt, N, k, stride, pad, dil, bias, act, prelu, tile, tag, planes, planes_chunk0, (B, OH, OW))
    if ln is not None and not aligned16(out, res, bias, ln[0], ln[1]):
        y = conv2d(x, wt, N, k, stride=stride, pad=pad, dil=dil, bias=bias, act=act, prelu=prelu, res=res, out=out, tile=tile,
                   tag=tag, planes=planes, planes_chunk0=planes_chunk0)
        return layernorm(y, ln[0], ln[1], ln[2], out=y)
    _, cin, lda = rows_view(x, "x")
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    OH = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    if out is None:
        out = torch.empty((B, OH, OW, N), device=x.device, dtype=torch.float32)
    orow, oc, ldo = rows_view(out, "out")
    if tuple(out.shape) != (B, OH, OW, N):
        raise RuntimeError(f"out shape {tuple(out.shape)} != {(B, OH, OW, N)}")
    K = k * k * cin
    kp = (K + 15) // 16 * 16
    if isinstance(wt, SplitWeight):
        if (wt.N, wt.cin) != (N, cin) or k != 3 or tile not in (-1, 14):
            raise RuntimeError(f"split weight ({wt.N}, {wt.cin}) does not fit conv N={N} Cin={cin} k={k} tile={tile}")
        if not wt.data.is_cuda or wt.data.dtype != torch.uint8:
            raise RuntimeError("segmif_amd: split weight image must be a uint8 tensor on the MI355X device")
        wt_ptr, tile = wt.data.data_ptr(), 14
    else:
        if tuple(_req(wt, "wt").shape) != (N, kp) or not wt.is_contiguous():
            raise RuntimeError(f"packed weight must be contiguous ({N}, {kp}), got {tuple(wt.shape)}")
        wt_ptr = wt.data_ptr()
    d = _lib.SegmifIgemm()
    d.in_, d.wt, d.out = x.data_ptr(), wt_ptr, out.data_ptr()
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.prelu = _req(prelu, "prelu").data_ptr() if prelu is not None else None
    if res is not None:
        rrow, rc, ldr = rows_view(res, "res")
        if rc != N or rrow != orow:
            raise RuntimeError("residual shape mismatch")
        d.res, d.ldr = res.data_ptr(), ldr
    d.M, d.N, d.K = B * OH * OW, N, K
    d.lda, d.ldo = lda, ldo
    d.H, d.W, d.Cin, d.KH, d.KW = H, W, cin, k, k
    d.stride, d.pad, d.dil, d.OH, d.OW = stride, pad, dil, OH, OW
    d.act, d.nz, d.tile = act, 1, tile
    if isinstance(wt, SplitWeight) and wt.f16:
        if in_amax is None or in_amax.dtype != torch.int32 or not in_amax.is_cuda or not in_amax.is_contiguous() or not 1 <= in_amax.numel() <= 64:
            raise RuntimeError("conv2d: f16x3 split weights need in_amax= (1..64 contiguous int32 range slots on the device)")
        d.split_f16, d.split_in_amax, d.split_in_amax_n = 1, in_amax.data_ptr(), in_amax.numel()
    elif in_amax is not None and not isinstance(wt, SplitWeight):
        raise RuntimeError("conv2d: in_amax= is for split 3x3 weights")
    if out_amax is not None:
        if not isinstance(wt, SplitWeight) or out_amax.dtype != torch.int32 or not out_amax.is_cuda or not out_amax.is_contiguous():
            raise RuntimeError("conv2d: out_amax= needs split 3x3 weights and a contiguous int32 device slot")
        d.split_out_amax, d.split_out_amax_n = out_amax.data_ptr(), out_amax.numel()
    if mask is not None:
        mrow, mc, ldm = rows_view(mask, "mask")
        if (mrow, mc) != (orow, N):
            raise RuntimeError("mask shape mismatch")
        d.relu_mask, d.ld_mask = mask.data_ptr(), ldm
    if ln is not None:
        if isinstance(wt, SplitWeight) or N != 64 or act != ACT_NONE:
            raise RuntimeError("conv2d: the fused LayerNorm epilogue needs fp32-packed weights, N = 64 and no activation")
        d.ln_gamma, d.ln_beta, d.ln_eps = _req(ln[0]).data_ptr(), _req(ln[1]).data_ptr(), float(ln[2])
    if planes is not None:
        if isinstance(wt, SplitWeight) or (planes.B, planes.H, planes.W) != (B, OH, OW):
            raise RuntimeError("conv2d: planes output needs fp32-packed weights and a planes buffer of the output geometry")
        planes.need(planes_chunk0 + N // 16, "conv2d planes output")
        d.planes_out, d.planes_chunks, d.planes_chunk0 = planes.data.data_ptr(), planes.chunks, planes_chunk0
        if planes.f16:
            d.planes_f16 = 1
            d.planes_amax, d.planes_amax_images = planes.guard.slot(B)
    _igemm(d, tag, dev=x.device)
    return out


def _conv2d_planes_only(x, wt, N, k, stride, pad, dil, bias, act, prelu, tile, tag, planes, planes_chunk0, oshape):
    """conv2d's launch with a NULL fp32 output: the epilogue writes the planes copy only."""
    _, cin, lda = rows_view(x, "x")
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    _, OH, OW = oshape
    K = k * k * cin
    kp = (K + 15) // 16 * 16
    if tuple(_req(wt, "wt").shape) != (N, kp) or not wt.is_contiguous():
        raise RuntimeError(f"packed weight must be contiguous ({N}, {kp}), got {tuple(wt.shape)}")
    if (planes.B, planes.H, planes.W) != (B, OH, OW):
        raise RuntimeError("conv2d: planes output needs a planes buffer of the output geometry")
    planes.need(planes_chunk0 + N // 16, "conv2d planes output")
    d = _lib.SegmifIgemm()
    d.in_, d.wt, d.out = x.data_ptr(), wt.data_ptr(), None
    d.bias = _req(bias, "bias").data_ptr() if bias is not None else None
    d.prelu = _req(prelu, "prelu").data_ptr() if prelu is not None else None
    d.M, d.N, d.K = B * OH * OW, N, K
    d.lda, d.ldo = lda, N
    d.H, d.W, d.Cin, d.KH, d.KW = H, W, cin, k, k
    d.stride, d.pad, d.dil, d.OH, d.OW = stride, pad, dil, OH, OW
    d.act, d.nz, d.tile = act, 1, tile
    d.planes_out, d.planes_chunks, d.planes_chunk0 = planes.data.data_ptr(), planes.chunks, planes_chunk0
    if planes.f16:
        d.planes_f16 = 1
        d.planes_amax, d.planes_amax_images = planes.guard.slot(B)
    _igemm(d, tag, dev=x.device)
    return None


def conv3x3_c32to1(x, wt, *, bias=None, act=ACT_NONE, prelu=None):
    """3x3 'same' conv from 32 channels to one (+ bias + act) as a vector-ALU stencil: x (B, H, W, 32) rows view, wt the
    fp32 packing (1, 288) of the (1, 32, 3, 3) weight -> (B, H, W, 1)."""
    _, cin, ldx = rows_view(x, "x")
    if x.dim() != 4 or cin != 32 or tuple(_req(wt, "wt").shape) != (1, 288) or not wt.is_contiguous():
        raise RuntimeError("conv3x3_c32to1 expects (B, H, W, 32) input and the packed (1, 288) weight")
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    out = torch.empty((B, H, W, 1), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_conv3x3_c32to1_f32(x.data_ptr(), ldx, wt.data_ptr(),
                                                     _req(bias, "bias").data_ptr() if bias is not None else None,
                                                     _req(prelu, "prelu").data_ptr() if prelu is not None else None, act,
                                                     out.data_ptr(), B, H, W, _stream()), "segmif_conv3x3_c32to1_f32")
    return out


def conv3x3_c1(x, w, *, bias=None, act=ACT_NONE, prelu=None, planes=None, planes_chunk0=0, planes_only=False):
    """(r6) 3x3 'same' conv from ONE channel to 64 (+ bias + act) as a store-bound stencil (csrc/conv3x3_planes.hip,
    conv3x3_c1_kernel): x contiguous (B, H, W, 1), w the RAW (64, 1, 3, 3) weight.  planes: an f16x3 ops.Planes receiving chunks
    [planes_chunk0, planes_chunk0 + 4); planes_only: no fp32 result (returns None)."""
    _req(x, "x"), _req(w, "w")
    if x.dim() != 4 or x.shape[-1] != 1 or not x.is_contiguous() or tuple(w.shape) != (64, 1, 3, 3) or not w.is_contiguous():
        raise RuntimeError("conv3x3_c1 expects a contiguous (B, H, W, 1) image and the raw contiguous (64, 1, 3, 3) weight")
    B, H, W = x.shape[0], x.shape[1], x.shape[2]
    if planes is not None and (not planes.f16 or (planes.B, planes.H, planes.W) != (B, H, W)):
        raise RuntimeError("conv3x3_c1: planes output needs an f16x3 planes buffer of the image's geometry")
    if planes_only and planes is None:
        raise RuntimeError("conv3x3_c1: planes_only needs a planes buffer")
    out = None if planes_only else torch.empty((B, H, W, 64), device=x.device, dtype=torch.float32)
    pl_ptr, chunks, amax, nimg = None, 0, None, 1
    if planes is not None:
        planes.need(planes_chunk0 + 4, "conv3x3_c1 planes output")
        pl_ptr, chunks = planes.data.data_ptr(), planes.chunks
        amax, nimg = planes.guard.slot(B)
    _lib.check(_lib.load().segmif_conv3x3_c1_f16x3(
        x.data_ptr(), w.data_ptr(), _req(bias, "bias").data_ptr() if bias is not None else None,
        _req(prelu, "prelu").data_ptr() if prelu is not None else None, act, pl_ptr, chunks, planes_chunk0,
        out.data_ptr() if out is not None else None, 64, B, H, W, amax, nimg, _stream()), "segmif_conv3x3_c1_f16x3")
    return out


def conv_ln_fusable(N):
    """True when a conv's LayerNorm can ride in its epilogue: the row (all N channels) must sit in one wave tile - N = 64,
    i.e. the stage-1 patch embed of mit_b1 .. b5 (614 400 rows at 32 images of 480x640: the only patch-embed LayerNorm over
    a large tensor); wider stages (128 .. 512 channels) would need a 32-row x full-N workgroup tile that re-reads the whole
    weight matrix per 32 rows, and the spatial-reduction convs run split-K."""
    return N == 64


def layernorm(x, gamma, beta, eps, out=None):
    rows, C, ldx = rows_view(x, "x")
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    orow, oc, ldy = rows_view(out, "out")
    if (orow, oc) != (rows, C):
        raise RuntimeError("layernorm out shape mismatch")
    if not aligned16(gamma, beta):  # parameters at an odd offset of a flattened buffer: the kernel loads them 16 bytes at a time
        gamma, beta = gamma.detach().clone(), beta.detach().clone()
    _lib.check(_lib.load().segmif_layernorm_f32(x.data_ptr(), _req(gamma).data_ptr(), _req(beta).data_ptr(),
                                                out.data_ptr(), rows, C, ldx, ldy, float(eps), _stream()),
               "segmif_layernorm_f32")
    return out


def pack_dw_weight(w):
    """(C, 1, 3, 3) depthwise weight -> [9][C]."""
    return _req(w).detach().reshape(w.shape[0], 9).t().contiguous()


def dwconv3x3_gelu(x, w9, bias, H, W):
    """x: contiguous tokens (B, H*W, C) -> same shape."""
    _req(x, "x")
    if not x.is_contiguous() or x.dim() != 3 or x.shape[1] != H * W:
        raise RuntimeError("dwconv3x3_gelu expects contiguous (B, H*W, C)")
    B, _, C = x.shape
    out = torch.empty_like(x)
    _side("dwconv", lambda: _lib.check(_lib.load().segmif_dwconv3x3_gelu_f32(
        x.data_ptr(), _req(w9).data_ptr(), _req(bias).data_ptr(), out.data_ptr(), B, H, W, C, _stream()),
        "segmif_dwconv3x3_gelu_f32"), 8.0 * x.numel())
    return out


def dwconv3x3_bias(x, w9, bias, H, W):
    """DWConv.forward (core/mix_transformer.py:381-387): depthwise 3x3 + bias on contiguous tokens (B, H*W, C)."""
    _req(x, "x")
    if not x.is_contiguous() or x.dim() != 3 or x.shape[1] != H * W:
        raise RuntimeError("dwconv3x3_bias expects contiguous (B, H*W, C)")
    B, _, C = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().segmif_dwconv3x3_bias_f32(x.data_ptr(), _req(w9).data_ptr(), _req(bias).data_ptr(),
                                                     out.data_ptr(), B, H, W, C, _stream()),
               "segmif_dwconv3x3_bias_f32")
    return out


def bilinear(x, OH, OW, out=None):
    """x: (B, IH, IW, C) rows view -> (B, OH, OW, C) (out may be a channel slice of a wider buffer)."""
    if x.dim() != 4:
        raise RuntimeError("bilinear expects (B, H, W, C)")
    _, C, ldx = rows_view(x, "x")
    B, IH, IW = x.shape[0], x.shape[1], x.shape[2]
    if out is None:
        out = torch.empty((B, OH, OW, C), device=x.device, dtype=torch.float32)
    _, oc, ldo = rows_view(out, "out")
    if tuple(out.shape) != (B, OH, OW, C):
        raise RuntimeError("bilinear out shape mismatch")
    _side("bilinear", lambda: _lib.check(_lib.load().segmif_bilinear_nhwc_f32(
        x.data_ptr(), out.data_ptr(), B, IH, IW, OH, OW, C, ldx, ldo, _stream()), "segmif_bilinear_nhwc_f32"),
        4.0 * C * B * (IH * IW + OH * OW))
    return out


def upsum_act(base, srcs, OH, OW, bias=None, act=ACT_NONE, out=None):
    """out = act(base + bias + sum_i bilinear(srcs[i] -> OH x OW)); base (B,OH,OW,C) rows view or None, srcs: up
    to three contiguous (B, ih, iw, C) maps."""
    if not 1 <= len(srcs) <= 3:
        raise RuntimeError("upsum_act takes one to three sources")
    B, C = srcs[0].shape[0], srcs[0].shape[-1]
    for s in srcs:
        if _req(s, "src").dim() != 4 or not s.is_contiguous() or s.shape[0] != B or s.shape[-1] != C:
            raise RuntimeError("upsum_act sources must be contiguous (B, ih, iw, C) with a common B and C")
    if out is None:
        out = torch.empty((B, OH, OW, C), device=srcs[0].device, dtype=torch.float32)
    _, oc, ldo = rows_view(out, "out")
    ldb = 0
    if base is not None:
        _, bc, ldb = rows_view(_req(base, "base"), "base")
        if tuple(base.shape) != (B, OH, OW, C):
            raise RuntimeError("upsum_act base shape mismatch")
    if tuple(out.shape) != (B, OH, OW, C):
        raise RuntimeError("upsum_act out shape mismatch")
    args = []
    for i in range(3):
        if i < len(srcs):
            args += [srcs[i].data_ptr(), srcs[i].shape[1], srcs[i].shape[2]]
        else:
            args += [None, 0, 0]
    _lib.check(_lib.load().segmif_upsum_act_nhwc_f32(base.data_ptr() if base is not None else None, ldb, *args,
                                                     _req(bias, "bias").data_ptr() if bias is not None else None,
                                                     out.data_ptr(), ldo, B, OH, OW, C, act, _stream()),
               "segmif_upsum_act_nhwc_f32")
    return out


def sr_attention(q, kv, heads, scale, pairs=False):
    """q: (B, N, C) contiguous; kv: (B, Nk, 2C) contiguous (k | v) -> (B, N, C).  pairs=True: return the result as ops.Pairs
    when the f16x3 kernel runs (inside a guarded scope, head_dim 64, N >= 1024), the fp32 tensor otherwise."""
    _req(q, "q"), _req(kv, "kv")
    B, N, C = q.shape
    Nk = kv.shape[1]
    hd = C // heads
    if not q.is_contiguous() or not kv.is_contiguous() or kv.shape[2] != 2 * C:
        raise RuntimeError("sr_attention expects contiguous q (B,N,C) and kv (B,Nk,2C)")
    out = torch.empty_like(q)
    kptr = kv.data_ptr()
    lib = _lib.load()
    if hd == 64 and _mode("attention") != "fp32" and N >= 1024:  # below that the K/V pack launch outweighs the matrix-pipe gain
        ws = torch.empty((lib.segmif_sr_attention_split_workspace(B, heads, Nk),), device=q.device, dtype=torch.uint8)
        guard = active_guard()
        if _mode("attention") == "f16x3" and guard is not None and pairs:
            amax, nimg = guard.slot(B)
            oamax, _ = guard.slot(B)
            _lib.check(lib.segmif_sr_attention_split16_pairs_f32(q.data_ptr(), kptr, kptr + 4 * C, out.data_ptr(), ws.data_ptr(), B,
                                                                 heads, N, Nk, hd, C, 2 * C, C, float(scale), amax, oamax, nimg,
                                                                 _stream()), "segmif_sr_attention_split16_pairs_f32")
            return Pairs(out)
        if _mode("attention") == "f16x3" and guard is not None:
            amax, nimg = guard.slot(B)
            _lib.check(lib.segmif_sr_attention_split16_f32(q.data_ptr(), kptr, kptr + 4 * C, out.data_ptr(), ws.data_ptr(), B, heads,
                                                           N, Nk, hd, C, 2 * C, C, float(scale), amax, nimg, _stream()),
                       "segmif_sr_attention_split16_f32")
            return out
        _lib.check(lib.segmif_sr_attention_split_f32(q.data_ptr(), kptr, kptr + 4 * C, out.data_ptr(), ws.data_ptr(), B, heads, N,
                                                     Nk, hd, C, 2 * C, C, float(scale), _stream()),
                   "segmif_sr_attention_split_f32")
        return out
    _lib.check(lib.segmif_sr_attention_f32(q.data_ptr(), kptr, kptr + 4 * C, out.data_ptr(), B, heads, N, Nk,
                                           hd, C, 2 * C, C, float(scale), _stream()),
               "segmif_sr_attention_f32")
    return out


def sr_attention_bwd(q, kv, out, dout, heads, scale):
    """Backward of sr_attention for head_dim 64 without materialising the scores (csrc/attention_bwd.hip): q, out, dout (B, N, C)
    contiguous, kv (B, Nk, 2C) contiguous -> (dq (B, N, C), dkv (B, Nk, 2C))."""
    B, N, C = q.shape
    Nk = kv.shape[1]
    if C != heads * 64 or not (q.is_contiguous() and kv.is_contiguous() and out.is_contiguous() and dout.is_contiguous()) \
            or kv.shape[2] != 2 * C:
        raise RuntimeError("sr_attention_bwd expects contiguous q / out / dout (B, N, 64 heads) and kv (B, Nk, 128 heads)")
    lib = _lib.load()
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    ws = torch.empty((lib.segmif_sr_attention_bwd_workspace_floats(B, heads, N, Nk, C),), device=q.device, dtype=torch.float32)
    kptr = kv.data_ptr()
    _lib.check(lib.segmif_sr_attention_bwd_f32(_req(q, "q").data_ptr(), kptr, kptr + 4 * C, _req(out, "out").data_ptr(),
                                               _req(dout, "dout").data_ptr(), dq.data_ptr(), dkv.data_ptr(), ws.data_ptr(), B, heads, N,
                                               Nk, 64, 2 * C, float(scale), _stream()), "segmif_sr_attention_bwd_f32")
    return dq, dkv


def linattn_partial(kv, heads=8):
    """kv: (B, N, 2C) contiguous -> fp64 partial sums (B, nblk, heads*d*d)."""
    _req(kv, "kv")
    B, N, C2 = kv.shape
    d = C2 // 2 // heads
    nblk = _lib.load().segmif_linattn_num_blocks(N)
    part = torch.empty((B, nblk, heads * d * d), device=kv.device, dtype=torch.float64)
    _lib.check(_lib.load().segmif_linattn_partial_f32(kv.data_ptr(), part.data_ptr(), B, N, heads, d, kv.stride(1),
                                                      _stream()), "segmif_linattn_partial_f32")
    return part


def linattn_kv_fusable(C, heads):
    """The one geometry linattn_kvpartial (kv projection + K^T V reduction in one kernel) is built for: C = 64, 8 heads of 8.
    Every caller that chooses between it and GEMM + linattn_partial asks here."""
    return C == 64 and heads == 8


def linattn_kvpartial(y, wkv, heads=8):
    """Fused kv projection (no bias) + K^T V partial sums. y: (B, N, 64) rows view; wkv: raw (128, 64)
    Linear weight -> fp64 partial sums (B, nblk, 512); kv itself never reaches HBM."""
    _req(y, "y"), _req(wkv, "wkv")
    if y.dim() != 3 or y.shape[2] != 64 or y.stride(2) != 1 or y.stride(0) != y.shape[1] * y.stride(1):
        raise RuntimeError("linattn_kvpartial expects a (B, N, 64) rows view")
    if tuple(wkv.shape) != (128, 64) or not wkv.is_contiguous():
        raise RuntimeError("linattn_kvpartial expects the raw contiguous (128, 64) kv weight")
    B, N, _ = y.shape
    nblk = _lib.load().segmif_linattn_num_blocks(N)
    part = torch.empty((B, nblk, 512), device=y.device, dtype=torch.float64)
    _lib.check(_lib.load().segmif_linattn_kvpartial_f32(y.data_ptr(), wkv.data_ptr(), part.data_ptr(), B, N, heads, 8,
                                                        y.stride(1), _stream()), "segmif_linattn_kvpartial_f32")
    return part


def linattn_fold(part, wend, weff, wofs, kofs, scale, heads=8):
    """Fold softmax((K^T V)*scale) into end_proj: writes weff[:, :, kofs:kofs+64] (weff: (B, Nout, Kp))."""
    B, nblk, e = part.shape
    d = int(round((e // heads) ** 0.5))
    Nout = wend.shape[0]
    _lib.check(_lib.load().segmif_linattn_fold_f32(part.data_ptr(), _req(wend).data_ptr(), _req(weff).data_ptr(), B,
                                                   nblk, heads, d, Nout, wend.stride(0), wofs, weff.stride(1), kofs,
                                                   float(scale), _stream()), "segmif_linattn_fold_f32")
    return weff


def linattn_fold_bwd(ktv, wend, dweff, dktv, dwend_part, wofs, kofs, scale, heads):
    """Backward of linattn_fold (heads * d <= 64 a multiple of 16, d <= 8): ktv / dktv (B, heads, d, d) fp64 contiguous, wend
    (Nout, ldw), dweff (B, Nout, ldweff) and dwend_part (B, Nout, ldp) with unit column stride.  Writes dktv and
    dwend_part[:, :, wofs:wofs + heads * d] (this image's share of d end_proj; the caller sums over images)."""
    B, h, d, _ = ktv.shape
    if h != heads or not ktv.is_contiguous() or not dktv.is_contiguous() or dktv.shape != ktv.shape:
        raise RuntimeError("linattn_fold_bwd expects contiguous (B, heads, d, d) ktv / dktv")
    for t, n in ((wend, "wend"), (dweff, "dweff"), (dwend_part, "dwend_part")):
        if _req(t, n).stride(-1) != 1:
            raise RuntimeError(f"linattn_fold_bwd: {n} needs unit column stride")
    if dweff.stride(0) != dweff.shape[1] * dweff.stride(1) or dwend_part.stride(0) != dwend_part.shape[1] * dwend_part.stride(1):
        raise RuntimeError("linattn_fold_bwd: dweff / dwend_part images must be packed")
    _lib.check(_lib.load().segmif_linattn_fold_bwd_f32(
        ktv.data_ptr(), wend.data_ptr(), wend.stride(0), wofs, dweff.data_ptr(), dweff.stride(1), kofs, float(scale), dktv.data_ptr(),
        dwend_part.data_ptr(), dwend_part.stride(1), B, wend.shape[0], heads, d, _stream()), "segmif_linattn_fold_bwd_f32")
    return dktv, dwend_part


class LazySeg:
    """The segmentation feature CrossPath consumes, NOT yet resized: `low` = (B, ih, iw, 64) contiguous NHWC (conv3 / conv4 already
    applied), to be read as bilinear(low -> H x W) (align_corners = False; core/mix_transformer.py:364-373).  The Gram-form
    CrossPath reads it through segmif_crosspath_gram_lazy_f32 / SegmifCrossTail.x3_ih - the (B, H, W, 64) tensor (5 GB at 64 x 480
    x 640, written once and read three times per interaction) never exists; any other consumer calls materialise()."""

    def __init__(self, low, H, W):
        _req(low, "low")
        if low.dim() != 4 or low.shape[-1] != 64 or not low.is_contiguous():
            raise RuntimeError("LazySeg expects a contiguous (B, ih, iw, 64) map")
        self.low, self.H, self.W = low, int(H), int(W)
        self._full = None

    @property
    def shape(self):
        return torch.Size((self.low.shape[0], self.H, self.W, 64))

    requires_grad = False

    def fits(self):
        """segmif_crosspath_gram_lazy_f32's geometry: aligned groups of four pixels in one row, an enlargement by three or more."""
        return self.W % 4 == 0 and 3 * self.low.shape[2] <= self.W

    def materialise(self):
        if self._full is None:
            self._full = bilinear(self.low, self.H, self.W)
        return self._full


def crosspath_gram_lazy(s_low, H, W):
    """Gram partials of relu(bilinear(s_low -> H x W)): s_low (B, ih, iw, 64) rows view (a channel slice of the projected low-
    resolution map: pitch = its last stride) -> (B, nblk, 3072) fp64, as crosspath_gram gives on the resized tensor."""
    _req(s_low, "s_low")
    if s_low.dim() != 4 or s_low.shape[3] != 64 or s_low.stride(3) != 1 or s_low.stride(1) != s_low.shape[2] * s_low.stride(2) \
            or s_low.stride(0) != s_low.shape[1] * s_low.stride(1):
        raise RuntimeError("crosspath_gram_lazy expects a (B, ih, iw, 64) rows view")
    B, ih, iw, _ = s_low.shape
    lib = _lib.load()
    nblk = lib.segmif_crosspath_gram_blocks(H * W)
    part = torch.empty((B, nblk, 3072), device=s_low.device, dtype=torch.float64)
    _side("cp_gram_lazy", lambda: _lib.check(lib.segmif_crosspath_gram_lazy_f32(
        s_low.data_ptr(), s_low.stride(2), ih, iw, H, W, part.data_ptr(), B, _stream()), "segmif_crosspath_gram_lazy_f32"),
        256.0 * B * ih * iw)
    return _gram_total(part)


def _gram_total(part):
    """(r6) (B, nblk, 3072) Gram partials -> (B, 1, 3072): their fixed-order sum by segmif_crosspath_gram_sum_f64 (12 workgroups per
    image), so that crosspath_fold's one workgroup per image reads 24 KB instead of 1.5 - 3 MB."""
    B, nblk, _ = part.shape
    if nblk <= 2:
        return part
    total = torch.empty((B, 1, 3072), device=part.device, dtype=torch.float64)
    _lib.check(_lib.load().segmif_crosspath_gram_sum_f64(part.data_ptr(), nblk, total.data_ptr(), B, _stream()), "segmif_crosspath_gram_sum_f64")
    return total


def crosspath_gram(x, w_half, b_half):
    """Per-image Gram partials of relu(x @ w_half^T + b_half): x (B, N, 64) rows view, w_half a contiguous (64, 64) slice
    of a channel_proj weight -> (B, nblk, 3072) fp64 (segmif_crosspath_gram_f32)."""
    _req(x, "x"), _req(w_half, "w_half")
    if x.dim() != 3 or x.shape[2] != 64 or x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        raise RuntimeError("crosspath_gram expects a (B, N, 64) rows view")
    if tuple(w_half.shape) != (64, 64) or not w_half.is_contiguous():
        raise RuntimeError("crosspath_gram expects a contiguous (64, 64) weight slice")
    B, N, _ = x.shape
    lib = _lib.load()
    nblk = lib.segmif_crosspath_gram_blocks(N)
    part = torch.empty((B, nblk, 3072), device=x.device, dtype=torch.float64)
    _side("cp_gram", lambda: _lib.check(lib.segmif_crosspath_gram_f32(
        x.data_ptr(), x.stride(1), w_half.data_ptr(), _req(b_half, "bias").data_ptr() if b_half is not None else None,
        part.data_ptr(), B, N, _stream()), "segmif_crosspath_gram_f32"), 256.0 * B * N)
    return _gram_total(part)


def crosspath_fold(part, wkv, wend, weff, wofs, kofs, scale):
    """softmax((Wk G Wv^T) * scale) per head from Gram partials, folded into end_proj: writes weff[:, :, kofs:kofs+64]."""
    B, nblk, _ = part.shape
    if tuple(_req(wkv, "wkv").shape) != (128, 64) or not wkv.is_contiguous():
        raise RuntimeError("crosspath_fold expects the raw contiguous (128, 64) kv weight")
    Nout = wend.shape[0]
    guard = active_guard()
    cond = guard.cond_slot(B) if guard is not None else None  # (r5) the softmax's conditioning figure, per image
    _lib.check(_lib.load().segmif_crosspath_fold_f32(part.data_ptr(), nblk, wkv.data_ptr(), _req(wend).data_ptr(),
                                                     _req(weff).data_ptr(), B, Nout, wend.stride(0), wofs, weff.stride(1), kofs,
                                                     float(scale), cond, _stream()), "segmif_crosspath_fold_f32")
    return weff


def crosspath_tail(x3, xi, w3, b3, wi, bi, weff, bend, ln, out=None, planes=None, hw=None, planes_only=False, lazy=False):
    """out = LN(x_i + weff_b @ [relu(w3 x_3 + b3) | relu(wi x_i + bi)] + bend): x3, xi (B, N, 64) rows views, w3 / wi
    contiguous (64, 64) slices, weff (B, 64, 128), ln = (gamma, beta, eps).  planes: optional ops.Planes that receives
    out as chunks 0..3 (hw = (H, W) with H * W == N); planes_only: write nothing else (the fp32 tensor has no reader:
    the second interaction of Fusion_Network3_ac, whose consumers are the planes convs) and return None.
    lazy=True: x3 is the (B, ih, iw, 64) rows view of the LOW-resolution map of channel_proj3's y half already applied (w3 / b3
    unused); the kernel reads bilinear(x3 -> hw) (SegmifCrossTail.x3_ih)."""
    for t, nm in ((xi, "xi"),) if lazy else ((x3, "x3"), (xi, "xi")):
        _req(t, nm)
        if t.dim() != 3 or t.shape[2] != 64 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError(f"crosspath_tail: {nm} must be a (B, N, 64) rows view")
    B, N, _ = xi.shape
    if lazy:
        _req(x3, "x3")
        if x3.dim() != 4 or x3.shape[0] != B or x3.shape[3] != 64 or x3.stride(3) != 1 or x3.stride(1) != x3.shape[2] * x3.stride(2) \
                or x3.stride(0) != x3.shape[1] * x3.stride(1) or hw is None or hw[0] * hw[1] != N:
            raise RuntimeError("crosspath_tail: lazy x3 must be a (B, ih, iw, 64) rows view, with hw = (H, W) of the tokens")
    if planes_only:
        if planes is None or out is not None:
            raise RuntimeError("crosspath_tail: planes_only needs a planes buffer and no fp32 output")
    else:
        if out is None:
            out = torch.empty((B, N, 64), device=xi.device, dtype=torch.float32)
        if tuple(out.shape) != (B, N, 64) or out.stride(2) != 1 or out.stride(0) != N * out.stride(1):
            raise RuntimeError("crosspath_tail: out must be a (B, N, 64) rows view")
    for t in (wi,) if lazy else (w3, wi):
        if tuple(_req(t, "w").shape) != (64, 64) or not t.is_contiguous():
            raise RuntimeError("crosspath_tail expects contiguous (64, 64) weight slices")
    if tuple(_req(weff, "weff").shape) != (B, 64, 128) or not weff.is_contiguous():
        raise RuntimeError("crosspath_tail expects a contiguous (B, 64, 128) folded weight")
    d = _lib.SegmifCrossTail()
    d.x3, d.xi, d.ld3, d.ldi = x3.data_ptr(), xi.data_ptr(), x3.stride(2 if lazy else 1), xi.stride(1)
    d.w3, d.wi, d.weff = None if lazy else w3.data_ptr(), wi.data_ptr(), weff.data_ptr()
    d.b3 = _req(b3).data_ptr() if b3 is not None and not lazy else None
    if lazy:
        d.x3_ih, d.x3_iw, d.H, d.W = x3.shape[1], x3.shape[2], hw[0], hw[1]
    d.bi = _req(bi).data_ptr() if bi is not None else None
    d.bend = _req(bend).data_ptr() if bend is not None else None
    d.ln_gamma, d.ln_beta, d.ln_eps = _req(ln[0]).data_ptr(), _req(ln[1]).data_ptr(), float(ln[2])
    d.out, d.ldo, d.B, d.N = (None, 64, B, N) if planes_only else (out.data_ptr(), out.stride(1), B, N)
    if planes is not None:
        if hw is None or hw[0] * hw[1] != N or (planes.B, planes.H, planes.W) != (B, hw[0], hw[1]):
            raise RuntimeError("crosspath_tail: planes geometry does not match the tokens")
        planes.need(4, "crosspath_tail planes output")
        d.planes_out, d.H, d.W, d.planes_chunks = planes.data.data_ptr(), hw[0], hw[1], planes.chunks
        if planes.f16:
            d.planes_f16 = 1
            d.planes_amax, d.planes_amax_images = planes.guard.slot(B)
            if lazy and planes_only and _mode("crosspath_arith") == "f16x3":
                # (r6) the kernel's own contractions on half pairs: its operands' range goes to a slot of its own
                d.arith_f16 = 1
                d.arith_amax, d.arith_amax_images = planes.guard.slot(B)
    _side("cp_tail", lambda: _lib.check(_lib.load().segmif_crosspath_tail_f32(ctypes.byref(d), _stream()),
                                        "segmif_crosspath_tail_f32"),
          ((512.0 if planes_only else 768.0) - (256.0 if lazy else 0.0) + (0.0 if planes is None else 256.0 if planes.f16 else 384.0)) * B * N)  # + the planes copy: 4 | 6 B per element
    return out


def seg_normalize(x):
    """(B,3,H,W) NCHW contiguous -> normalised NHWC (B,H,W,3)."""
    _req(x, "x")
    x = x.contiguous()
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError("seg_normalize expects 3 channels")
    out = torch.empty((B, H, W, 3), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_seg_normalize_f32(x.data_ptr(), out.data_ptr(), B, H, W, _stream()),
               "segmif_seg_normalize_f32")
    return out


def to_nhwc(x):
    """Logical NCHW tensor (any strides) -> contiguous NHWC (B,H,W,C) tensor, zero-copy when the
    input is already channels-last in memory."""
    _req(x, "x")
    B, C, H, W = x.shape
    p = x.permute(0, 2, 3, 1)
    if p.is_contiguous():
        return p
    if torch.is_grad_enabled() and x.requires_grad:
        return p.contiguous()  # keep the layout change inside the autograd graph
    x = x.contiguous()
    out = torch.empty((B, H, W, C), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_nchw_to_nhwc_f32(x.data_ptr(), out.data_ptr(), B, C, H * W, C, _stream()),
               "segmif_nchw_to_nhwc_f32")
    return out


def as_nchw(x_nhwc):
    """NHWC storage presented with the reference's logical (B, C, H, W) shape (channels_last strides)."""
    return x_nhwc.permute(0, 3, 1, 2)


def to_nchw_contiguous(x_nhwc):
    _req(x_nhwc, "x")
    B, H, W, C = x_nhwc.shape
    _, _, ldx = rows_view(x_nhwc, "x")
    out = torch.empty((B, C, H, W), device=x_nhwc.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_nhwc_to_nchw_f32(x_nhwc.data_ptr(), out.data_ptr(), B, C, H * W, ldx, _stream()),
               "segmif_nhwc_to_nchw_f32")
    return out


def fuse_ycrcb(vis, yf):
    """vis (B,3,H,W) RGB NCHW, yf (B,1,H,W) -> clamp01(YCrCb2RGB([yf, Cr(vis), Cb(vis)])) NCHW."""
    vis = _req(vis, "vis").contiguous()
    yf = _req(yf, "yf").contiguous()
    B, _, H, W = vis.shape
    out = torch.empty_like(vis)
    _lib.check(_lib.load().segmif_fuse_ycrcb_f32(vis.data_ptr(), yf.data_ptr(), out.data_ptr(), B, H * W, _stream()),
               "segmif_fuse_ycrcb_f32")
    return out


def bilinear_argmax(x, OH, OW):
    """(r6) argmax over channels of bilinear(x -> OH x OW) for NHWC logits x (B, IH, IW, C) rows view -> int32 labels (B, OH, OW); the
    resized logits are never formed (one kernel instead of bilinear + argmax_nhwc)."""
    if x.dim() != 4:
        raise RuntimeError("bilinear_argmax expects (B, H, W, C)")
    _, C, ldx = rows_view(x, "x")
    B, IH, IW = x.shape[0], x.shape[1], x.shape[2]
    labels = torch.empty((B, OH, OW), device=x.device, dtype=torch.int32)
    _side("bilinear", lambda: _lib.check(_lib.load().segmif_bilinear_argmax_i32(
        x.data_ptr(), labels.data_ptr(), B, IH, IW, OH, OW, C, ldx, _stream()), "segmif_bilinear_argmax_i32"),
        4.0 * B * (C * IH * IW + OH * OW))
    return labels


PSEUDO_BELOW = ("keep", "ignore")


def pseudo_label(logits_nhwc, OH, OW, tau=0.968, below="keep", ignore_index=255, return_conf=False):
    """Pseudo-labels of a teacher's NHWC logits (B, IH, IW, C) rows view, C <= 32, in one pass (csrc/pseudo_label.hip; the rule:
    include/segmif_hip.h, segmif_pseudo_label_f32): labels (B, OH, OW) int64 = argmax of the bilinear resize (bilinear_argmax's
    labels), count (B,) int64 = the pixels whose softmax maximum is > tau, and with return_conf the maximum itself (B, OH, OW)
    float32.  below="keep" leaves the argmax everywhere (DAFormer: the weight carries the confidence), "ignore" writes ignore_index
    where the maximum is not above tau.  tau = 0.968 is DAFormer's default.  The resized logits are never formed; no
    synchronisation.  -> (labels, count) or (labels, count, conf).  NOT the reference's training."""
    if logits_nhwc.dim() != 4:
        raise RuntimeError("pseudo_label expects (B, H, W, C)")
    if below not in PSEUDO_BELOW:
        raise ValueError(f"pseudo_label: below must be one of {', '.join(PSEUDO_BELOW)}, got {below!r}")
    tau = float(tau)
    _, C, ldx = rows_view(logits_nhwc, "logits")
    B, IH, IW = logits_nhwc.shape[0], logits_nhwc.shape[1], logits_nhwc.shape[2]
    if min(B, IH, IW, int(OH), int(OW)) < 1 or not 1 <= C <= 32 or not 0.0 <= tau <= 1.0:  # (NaN fails the comparison)
        raise ValueError(f"pseudo_label: sizes must be >= 1, C in 1..32 and tau in [0, 1]; got {tuple(logits_nhwc.shape)} -> "
                         f"{OH} x {OW}, tau {tau} (SEGMIF_EINVAL)")
    dev = logits_nhwc.device
    labels = torch.empty((B, OH, OW), device=dev, dtype=torch.int64)
    count = torch.empty((B,), device=dev, dtype=torch.int64)
    conf = torch.empty((B, OH, OW), device=dev, dtype=torch.float32) if return_conf else None
    _side("bilinear", lambda: _lib.check(_lib.load().segmif_pseudo_label_f32(
        logits_nhwc.data_ptr(), labels.data_ptr(), conf.data_ptr() if return_conf else None, count.data_ptr(), B, IH, IW, int(OH),
        int(OW), C, ldx, tau, int(below == "ignore"), int(ignore_index), _stream()), "segmif_pseudo_label_f32"),
        4.0 * B * C * IH * IW + (12.0 if return_conf else 8.0) * B * OH * OW)
    return (labels, count, conf) if return_conf else (labels, count)


def pseudo_weight(count, OH, OW):
    """DAFormer's pseudo_weight: q_b = count_b / (OH OW), the share of a sample's pixels above tau, as (B,) float32 on the device
    (count: pseudo_label's; formed in double, no readback)."""
    if not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int64 or count.dim() != 1:
        raise RuntimeError("pseudo_weight: count must be pseudo_label's (B,) int64 device tensor")
    return (count.double() / float(int(OH) * int(OW))).float()


def tta_vote(views, flips, OH, OW, want_probs=False):
    """Multi-scale + flip vote (csrc/tta.hip): views - up to 16 NHWC logit maps (B, ih, iw, C) rows views, C <= 32, as
    bilinear_argmax takes them; flips - one flag per view (the view's input was mirrored).  Every view is resized to OH x OW
    (bilinear_argmax's arithmetic, a mirrored one read at the mirrored column), soft-maxed and averaged in list order ->
    int32 labels (B, OH, OW) = argmax of the mean, or (labels, probs (B, OH, OW, C)) with want_probs.  Neither the resized
    logits nor, unless asked for, the probabilities are ever formed."""
    views, flips = list(views), list(flips)
    if not 1 <= len(views) <= 16 or len(flips) != len(views):
        raise RuntimeError(f"tta_vote takes 1..16 views and one flip flag per view, got {len(views)} and {len(flips)}")
    if views[0].dim() != 4:
        raise RuntimeError("tta_vote expects (B, H, W, C) views")
    B, C = views[0].shape[0], views[0].shape[3]
    tab = (_lib.SegmifTtaView * len(views))()
    nbytes = 4.0 * B * OH * OW * (1 + (C if want_probs else 0))
    for i, (x, f) in enumerate(zip(views, flips)):
        if x.dim() != 4 or x.shape[0] != B or x.shape[3] != C or x.device != views[0].device:
            raise RuntimeError(f"tta_vote: view {i} is {tuple(x.shape)}, expected ({B}, ih, iw, {C}) on one device")
        _, _, ldx = rows_view(x, f"views[{i}]")
        tab[i].x, tab[i].ih, tab[i].iw, tab[i].ldx, tab[i].flip = x.data_ptr(), x.shape[1], x.shape[2], ldx, int(bool(f))
        nbytes += 4.0 * x.numel()
    labels = torch.empty((B, OH, OW), device=views[0].device, dtype=torch.int32)
    probs = torch.empty((B, OH, OW, C), device=views[0].device, dtype=torch.float32) if want_probs else None
    _side("bilinear", lambda: _lib.check(_lib.load().segmif_tta_vote_f32(
        tab, len(views), labels.data_ptr(), probs.data_ptr() if want_probs else None, B, OH, OW, C, _stream()),
        "segmif_tta_vote_f32"), nbytes)
    return (labels, probs) if want_probs else labels


def resize_flip_nchw(x, OH, OW, flip):
    """x (B, C, IH, IW) contiguous NCHW -> flip?(F.interpolate(x, (OH, OW), mode='bilinear', align_corners=False)) in one pass
    (flip mirrors the width): the network input of one multi-scale view."""
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError("resize_flip_nchw expects a contiguous (B, C, H, W) tensor")
    B, C, IH, IW = x.shape
    out = torch.empty((B, C, OH, OW), device=x.device, dtype=torch.float32)
    _side("bilinear", lambda: _lib.check(_lib.load().segmif_resize_flip_nchw_f32(
        x.data_ptr(), out.data_ptr(), B * C, IH, IW, OH, OW, int(bool(flip)), _stream()), "segmif_resize_flip_nchw_f32"),
        4.0 * B * C * (IH * IW + OH * OW))
    return out


def pointwise2(a, b, mode, out=None):
    """(r6) y = a + b (mode 0), silu(a) + silu(b) (mode 1), silu(a) (mode 2; b None) over rows views of equal shape."""
    rows, C, lda = rows_view(a, "a")
    ldb = 0
    if b is not None:
        rb, cb, ldb = rows_view(b, "b")
        if (rb, cb) != (rows, C):
            raise RuntimeError("pointwise2: a and b differ in shape")
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=torch.float32)
    ro, co, ldo = rows_view(out, "out")
    if (ro, co) != (rows, C):
        raise RuntimeError("pointwise2: out shape mismatch")
    _lib.check(_lib.load().segmif_pointwise2_f32(a.data_ptr(), lda, b.data_ptr() if b is not None else None, ldb, out.data_ptr(), ldo,
                                                 rows, C, mode, _stream()), "segmif_pointwise2_f32")
    return out


def pointwise2_bwd(dy, a, b, mode, da=None, db=None):
    """Backward of pointwise2 modes 1 (silu(a) + silu(b)) and 2 (silu(a)) from the pre-activations a, b: -> (da, db) with
    da = dy silu'(a), db = dy silu'(b) (None in mode 2).  da / db: optional rows views (channel slices of wider buffers)."""
    if mode not in (1, 2) or (mode == 1) != (b is not None):
        raise RuntimeError("pointwise2_bwd: mode 1 takes a and b, mode 2 a only")
    rows, C, ldy = rows_view(dy, "dy")
    outs, lds = [], []
    for src, o, n in ((a, da, "a"), (b, db, "b")):
        if src is None:
            outs.append(None)
            lds += [0, 0]
            continue
        rs, cs, lds_ = rows_view(src, n)
        if (rs, cs) != (rows, C):
            raise RuntimeError(f"pointwise2_bwd: {n} and dy differ in shape")
        o = torch.empty(src.shape, device=src.device, dtype=torch.float32) if o is None else o
        ro, co, ldo = rows_view(o, "d" + n)
        if (ro, co) != (rows, C):
            raise RuntimeError(f"pointwise2_bwd: d{n} shape mismatch")
        outs.append(o)
        lds += [lds_, ldo]
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_lib.load().segmif_pointwise2_bwd_f32(dy.data_ptr(), ldy, a.data_ptr(), lds[0], ptr(b), lds[2], outs[0].data_ptr(), lds[1],
                                                     ptr(outs[1]), lds[3], rows, C, mode, _stream()), "segmif_pointwise2_bwd_f32")
    return outs[0], outs[1]


def argmax_nhwc(x):
    rows, C, ldx = rows_view(x, "x")
    out = torch.empty(x.shape[:-1], device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().segmif_argmax_nhwc_i32(x.data_ptr(), out.data_ptr(), rows, C, ldx, _stream()),
               "segmif_argmax_nhwc_i32")
    return out


AUGMENT_REC_WORDS = ctypes.sizeof(_lib.SegmifAugmentRec) // 4


def _req_u8(t, name, shape=None, dtype=torch.uint8):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"segmif_amd: {name} must be a tensor on the MI355X device (the HIP path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"segmif_amd: {name} must be a contiguous {dtype} tensor, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"segmif_amd: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _augment_args(label, rec, tab, crop_h, crop_w):
    _req_u8(label, "label")
    if label.dim() != 3:
        raise RuntimeError("augment: label must be (N, h, w) uint8")
    _req_u8(rec, "rec", dtype=torch.int32)
    _req_u8(tab, "tab", dtype=torch.int32)
    if rec.dim() != 2 or rec.shape[1] != AUGMENT_REC_WORDS or rec.shape[0] < 1:
        raise RuntimeError(f"augment: rec must be (B, {AUGMENT_REC_WORDS}) int32 (one SegmifAugmentRec per sample)")
    if crop_h < 1 or crop_w < 1 or crop_w % 4:
        raise RuntimeError(f"augment: the crop must be positive and its width a multiple of 4, got {crop_h} x {crop_w}")
    return label.shape


def augment_pick(label, rec, tab, crop_h, crop_w):
    """segmif_augment_pick_u8: chooses each sample's crop box among its ten candidates (imutils.py:223-238) and writes it
    into `rec` (B, AUGMENT_REC_WORDS) int32 on the device.  label: the resident (N, h, w) uint8 label maps."""
    N, h, w = _augment_args(label, rec, tab, crop_h, crop_w)
    _lib.check(_lib.load().segmif_augment_pick_u8(label.data_ptr(), N, h, w, rec.data_ptr(), tab.data_ptr(), tab.numel(), rec.shape[0],
                                                  crop_h, crop_w, _stream()), "segmif_augment_pick_u8")
    return rec


def augment_apply(ir, vis, mask, label, rec, tab, crop_h, crop_w):
    """segmif_augment_apply_u8: the augmented batch of the records' boxes -> ir3, vis3, mask3 (B, 3, crop_h, crop_w) fp32 and
    label (B, crop_h, crop_w) int64.  ir, mask, label (N, h, w) and vis (N, h, w, 3) are the resident uint8 frames."""
    N, h, w = _augment_args(label, rec, tab, crop_h, crop_w)
    _req_u8(ir, "ir", (N, h, w)), _req_u8(mask, "mask", (N, h, w)), _req_u8(vis, "vis", (N, h, w, 3))
    B = rec.shape[0]
    ir3, vis3, mask3 = (torch.empty((B, 3, crop_h, crop_w), device=label.device, dtype=torch.float32) for _ in range(3))
    out = torch.empty((B, crop_h, crop_w), device=label.device, dtype=torch.int64)
    _lib.check(_lib.load().segmif_augment_apply_u8(ir.data_ptr(), vis.data_ptr(), mask.data_ptr(), label.data_ptr(), N, h, w,
                                                   rec.data_ptr(), tab.data_ptr(), tab.numel(), B, crop_h, crop_w, ir3.data_ptr(),
                                                   vis3.data_ptr(), mask3.data_ptr(), out.data_ptr(), _stream()),
               "segmif_augment_apply_u8")
    return ir3, vis3, mask3, out


def check_want(want, B=None):
    """Host-side check of a pick_class `want` table (it lives on the device when the kernel reads it): (B, 2) integers, the
    class -1 (any negative value: the reference's rule) or 0..254, the threshold >= 0 -> (B, 2) int32 numpy array."""
    import numpy as np
    w = np.asarray(want)
    if w.ndim != 2 or w.shape[1] != 2 or w.shape[0] < 1 or (B is not None and w.shape[0] != B) or w.dtype.kind not in "iu":
        raise ValueError(f"augment_pick_class: want must be (B, 2) integers (class or -1, threshold), got {w.dtype} {w.shape}")
    if (w[:, 0] > 254).any() or (w[:, 1] < 0).any() or (w > 2 ** 31 - 1).any() or (w < -2 ** 31).any():
        raise ValueError("augment_pick_class: a wanted class lies in 0..254 (or is -1) and a threshold is >= 0 "
                         f"(SEGMIF_EINVAL), got {w.tolist()}")
    return np.ascontiguousarray(w, dtype=np.int32)


def augment_pick_class(label, rec, tab, crop_h, crop_w, want, tally=None):
    """segmif_augment_pick_class_u8: augment_pick with a second rule per sample.  want: (B, 2) (class or -1, threshold), either a
    host array / list, which is checked and uploaded here, or an int32 device tensor whose values the caller has passed through
    check_want.  tally: None or an (n_class, 2) int64 device tensor that accumulates (drawn, hit) per class.  -> got (B,) int32
    on the device: the chosen window's pixels of the wanted class, -1 for a sample without one."""
    N, h, w = _augment_args(label, rec, tab, crop_h, crop_w)
    B = rec.shape[0]
    if not isinstance(want, torch.Tensor) or not want.is_cuda:
        want = torch.from_numpy(check_want(want.numpy() if isinstance(want, torch.Tensor) else want, B)).to(label.device)
    _req_u8(want, "want", (B, 2), dtype=torch.int32)
    if tally is not None:
        _req_u8(tally, "tally", dtype=torch.int64)
        if tally.dim() != 2 or tally.shape[1] != 2 or tally.shape[0] < 1:
            raise RuntimeError("augment_pick_class: tally must be (n_class, 2) int64")
    got = torch.empty(B, device=label.device, dtype=torch.int32)
    _lib.check(_lib.load().segmif_augment_pick_class_u8(label.data_ptr(), N, h, w, rec.data_ptr(), tab.data_ptr(), tab.numel(), B, crop_h,
                                                        crop_w, want.data_ptr(), got.data_ptr(),
                                                        tally.data_ptr() if tally is not None else None,
                                                        tally.shape[0] if tally is not None else 0, _stream()),
               "segmif_augment_pick_class_u8")
    return got


def label_stats(label):
    """segmif_label_stats_u8 / _i64: per-frame class counts of uint8 (N, H, W) or int64 (B, H, W) label maps -> (N, 257) int64 on
    the device; column v < 256 counts the pixels equal to v, column 256 the values outside 0..255 (int64 maps only)."""
    if not isinstance(label, torch.Tensor) or not label.is_cuda:
        raise RuntimeError("segmif_amd: label_stats needs a tensor on the MI355X device (the HIP path has no CPU fallback)")
    if label.dtype not in (torch.uint8, torch.int64) or label.dim() != 3 or not label.is_contiguous() or label.numel() < 1:
        raise RuntimeError(f"label_stats: label must be a contiguous, non-empty (N, H, W) uint8 or int64 tensor, got {label.dtype} "
                           f"{tuple(label.shape)}")
    N = label.shape[0]
    counts = torch.empty((N, 257), device=label.device, dtype=torch.int64)
    fn = "segmif_label_stats_u8" if label.dtype == torch.uint8 else "segmif_label_stats_i64"
    _lib.check(getattr(_lib.load(), fn)(label.data_ptr(), N, label.shape[1] * label.shape[2], counts.data_ptr(), _stream()), fn)
    return counts


MIX_SEL_WORDS = 8


def check_mix_table(table, B, n_class):
    """Host-side check of a ClassMix table (it lives on the device when the kernels read it): (B, 2 + n_class) integers, rows
    (donor, force, key[0..n_class-1]) with the donor in 0..B-1, force in -1..n_class-1 and the keys a permutation of
    0..n_class-1 -> (B, 2 + n_class) int32 numpy array."""
    import numpy as np
    if not 1 <= n_class <= 255 or B < 1:
        raise ValueError(f"class_mix: n_class {n_class} outside 1..255 or B {B} < 1 (SEGMIF_EINVAL)")
    t = np.asarray(table)
    if t.ndim != 2 or t.shape != (B, 2 + n_class) or t.dtype.kind not in "iu":
        raise ValueError(f"class_mix: the table must be ({B}, {2 + n_class}) integers (donor, force, {n_class} keys), got {t.dtype} {t.shape}")
    if (t[:, 0] < 0).any() or (t[:, 0] >= B).any():
        raise ValueError(f"class_mix: a donor lies in 0..{B - 1}, got {t[:, 0].tolist()}")
    if (t[:, 1] < -1).any() or (t[:, 1] >= n_class).any():
        raise ValueError(f"class_mix: force is -1 (half of the present classes) or a class in 0..{n_class - 1}, got {t[:, 1].tolist()}")
    if not (np.sort(t[:, 2:], axis=1) == np.arange(n_class)).all():
        raise ValueError(f"class_mix: the keys of a row must be a permutation of 0..{n_class - 1}")
    return np.ascontiguousarray(t, dtype=np.int32)


def class_mix(ir3, vis3, mask3, label, table, n_class=9, min_pixels=0, tally=None):
    """ClassMix on an augmented batch (the rule: include/segmif_hip.h, segmif_class_mix_select): receiver b takes, from crop
    donor[b] of the SAME, unmixed batch, the pixels of the selected classes - half of the classes present in the donor (those
    with more than min_pixels pixels), the ones with the smallest keys, or the one class `force` - in every plane and in the
    label, bit for bit.  ir3, vis3, mask3 (B, 3, h, w) fp32, label (B, h, w) int64, w % 4 == 0.  table: (B, 2 + n_class) rows
    (donor, force, keys), either a host array / list, which is checked and uploaded here, or an int32 device tensor whose values
    the caller has passed through check_mix_table.  tally: None or an (n_class, 2) int64 device tensor that accumulates (samples
    that selected the class, pixels pasted).  Three launches on the current stream (label_stats, select, apply), no
    synchronisation.  -> (ir3', vis3', mask3', label', sel (B, 8) int32, pasted (B,) int64), new tensors.  NOT the reference's
    loader."""
    _req_u8(label, "label", dtype=torch.int64)
    if label.dim() != 3 or label.numel() < 1:
        raise RuntimeError(f"class_mix: label must be a non-empty (B, h, w) int64 tensor, got {tuple(label.shape)}")
    B, h, w = label.shape
    if w % 4:
        raise RuntimeError(f"class_mix: the width must be a multiple of 4 (16-byte accesses), got {w}")
    if not 1 <= n_class <= 255 or min_pixels < 0:
        raise ValueError(f"class_mix: n_class {n_class} outside 1..255 or min_pixels {min_pixels} < 0 (SEGMIF_EINVAL)")
    for t, name in ((ir3, "ir3"), (vis3, "vis3"), (mask3, "mask3")):
        _req_u8(t, name, (B, 3, h, w), dtype=torch.float32)
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        table = torch.from_numpy(check_mix_table(table.numpy() if isinstance(table, torch.Tensor) else table, B, n_class)).to(label.device)
    _req_u8(table, "table", (B, 2 + n_class), dtype=torch.int32)
    if tally is not None:
        _req_u8(tally, "tally", (n_class, 2), dtype=torch.int64)
    lib = _lib.load()
    counts = label_stats(label)
    sel = torch.empty((B, MIX_SEL_WORDS), device=label.device, dtype=torch.int32)
    pasted = torch.empty(B, device=label.device, dtype=torch.int64)
    _lib.check(lib.segmif_class_mix_select(counts.data_ptr(), table.data_ptr(), B, n_class, int(min_pixels), sel.data_ptr(), pasted.data_ptr(),
                                           tally.data_ptr() if tally is not None else None, _stream()), "segmif_class_mix_select")
    out = tuple(torch.empty_like(t) for t in (ir3, vis3, mask3, label))
    _lib.check(lib.segmif_class_mix_apply_f32(ir3.data_ptr(), vis3.data_ptr(), mask3.data_ptr(), label.data_ptr(), table.data_ptr(),
                                              sel.data_ptr(), B, h, w, n_class, *(t.data_ptr() for t in out), _stream()),
               "segmif_class_mix_apply_f32")
    return out + (sel, pasted)


STRONG_MAX_RADIUS = 8
STRONG_TILE = (32, 64)  # SEGMIF_STRONG_TILE_H, SEGMIF_STRONG_TILE_W
STRONG_REC_WORDS = 16


def strong_rec_dtype():
    """numpy's view of SegmifStrongAugRec (64 bytes): what a host table of strong_augment is made of"""
    import numpy as np
    return np.dtype([("jitter_on", np.int32), ("fb", np.float32), ("fc", np.float32), ("fs", np.float32), ("fh", np.float32),
                     ("radius", np.int32), ("taps", np.float32, (STRONG_MAX_RADIUS + 1,)), ("reserved", np.int32)])


def strong_taps(sigma):
    """The blur's taps for a Gaussian of standard deviation sigma in (0, 2]: R = min(8, ceil(4 sigma)),
    w_k = exp(-k^2 / (2 sigma^2)) over -R..R normalised in double, rounded to float32 -> (R, taps (9,) float32, zero past R)."""
    import math
    import numpy as np
    sigma = float(sigma)
    if not 0.0 < sigma <= 2.0:  # (NaN fails too)
        raise ValueError(f"strong_taps: sigma {sigma} outside (0, 2]")
    R = min(STRONG_MAX_RADIUS, math.ceil(4.0 * sigma))
    k = np.arange(-R, R + 1, dtype=np.float64)
    wk = np.exp(-k * k / (2.0 * sigma * sigma))
    wk /= wk.sum()
    taps = np.zeros(STRONG_MAX_RADIUS + 1, dtype=np.float32)
    taps[:R + 1] = wk[R:]
    return R, taps


def check_strong_table(table, B):
    """Host-side check of a strong-augmentation table (it lives on the device when the kernels read it): (B,) records of
    strong_rec_dtype() with fb, fc, fs finite and >= 0, |fh| <= 0.5, radius in 0..8, finite taps and reserved == 0
    -> a contiguous (B,) array of that dtype."""
    import numpy as np
    dt = strong_rec_dtype()
    t = np.asarray(table)
    if B < 1 or t.dtype != dt or t.shape != (B,):
        raise ValueError(f"strong_augment: the table must be ({B},) records of ops.strong_rec_dtype(), B >= 1, got {t.dtype} {t.shape}")
    for name in ("fb", "fc", "fs"):
        if not (np.isfinite(t[name]) & (t[name] >= 0)).all():
            raise ValueError(f"strong_augment: {name} must be finite and >= 0, got {t[name].tolist()}")
    if not (np.abs(t["fh"]) <= 0.5).all():  # (NaN fails too)
        raise ValueError(f"strong_augment: |fh| <= 0.5 is required, got {t['fh'].tolist()}")
    if ((t["radius"] < 0) | (t["radius"] > STRONG_MAX_RADIUS)).any():
        raise ValueError(f"strong_augment: radius lies in 0..{STRONG_MAX_RADIUS}, got {t['radius'].tolist()}")
    if not np.isfinite(t["taps"]).all():
        raise ValueError("strong_augment: the taps must be finite")
    if t["reserved"].any():
        raise ValueError("strong_augment: reserved must be zero")
    return np.ascontiguousarray(t)


def strong_augment(x, table, return_mean=False):
    """Colour jitter, then a Gaussian blur, per sample of a batch (the rule: include/segmif_hip.h, segmif_strong_augment_f32;
    DAFormer's strong_transform for the student of self-training).  x (B, 3, h, w) fp32 in [0, 1], w % 4 == 0.  table: (B,)
    records of strong_rec_dtype(), either a host array, which check_strong_table checks and this call uploads, or a (B, 16) int32
    device tensor of the same bytes whose values the caller has checked.  Two launches on the current stream, no synchronisation.
    No gradient is taken: an x that requires grad is refused.  -> y, a new tensor (with return_mean: (y, mean (B,) fp32), the
    luma mean the contrast step used, 0 for a sample without jitter).  NOT the reference's training."""
    _req_u8(x, "x", dtype=torch.float32)
    if x.requires_grad:
        raise RuntimeError("strong_augment: no gradient is taken through the augmentation; detach x")
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() < 1:
        raise RuntimeError(f"strong_augment: x must be a non-empty (B, 3, h, w) fp32 tensor, got {tuple(x.shape)}")
    B, _, h, w = x.shape
    if w % 4:
        raise RuntimeError(f"strong_augment: the width must be a multiple of 4 (16-byte accesses), got {w}")
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        import numpy as np
        host = check_strong_table(table, B)
        table = torch.from_numpy(host.view(np.int32).reshape(B, STRONG_REC_WORDS)).to(x.device)
    _req_u8(table, "table", (B, STRONG_REC_WORDS), dtype=torch.int32)
    lib = _lib.load()
    n = lib.segmif_strong_augment_blocks(h, w)
    if n < 1:
        raise RuntimeError(f"strong_augment: segmif_strong_augment_blocks({h}, {w}) failed with code {n}")
    partial = torch.empty((B, n), device=x.device, dtype=torch.float64)
    y, mean = torch.empty_like(x), torch.empty(B, device=x.device, dtype=torch.float32)
    _lib.check(lib.segmif_strong_augment_f32(x.data_ptr(), y.data_ptr(), table.data_ptr(), partial.data_ptr(), mean.data_ptr(), B, h, w,
                                             _stream()), "segmif_strong_augment_f32")
    return (y, mean) if return_mean else y


PASTE_WORDS, PASTE_MAX_SLOTS, PASTE_MAX_SIZE, PASTE_MAX_STEP = (_lib.PASTE_RECORD_WORDS, _lib.PASTE_MAX_SLOTS, _lib.PASTE_MAX_SIZE,
                                                                  _lib.PASTE_MAX_STEP)


def object_boxes(root, label, n_class, class_mask, min_area, max_box, records, counter, frame0=0, workspace=None):
    """segmif_object_boxes_i32 (the rule: include/segmif_paste.h): appends one record {frame0 + frame, root, cls, area, x0, y0, bw, bh}
    per connected component of `root` (n, H, W) int32 (utils.objects.connected_components' roots of `label` (n, H, W) uint8) whose
    class is below n_class and in the 32-bit class_mask, whose area is >= min_area and whose tight box holds <= max_box pixels.
    records (capacity, 8) int32 and counter (1,) int32 are device tensors: the caller zeroes the counter, which rises past the
    capacity when the list is too short (those records are not written).  The append order is arrival order: sort by (frame, root).
    Three launches, no synchronisation.  -> the workspace used (pass it back to spare the allocation)."""
    _req_u8(root, "root", dtype=torch.int32)
    if root.dim() != 3 or root.numel() < 1:
        raise RuntimeError(f"object_boxes: root must be a non-empty (n, H, W) int32 tensor, got {tuple(root.shape)}")
    n, H, W = (int(v) for v in root.shape)
    _req_u8(label, "label", (n, H, W))
    _req_u8(records, "records", dtype=torch.int32)
    _req_u8(counter, "counter", (1,), dtype=torch.int32)
    if records.dim() != 2 or records.shape[1] != PASTE_WORDS:
        raise RuntimeError(f"object_boxes: records must be (capacity, {PASTE_WORDS}) int32, got {tuple(records.shape)}")
    if not 1 <= n_class <= 32 or min_area < 1 or max_box < 1 or frame0 < 0 or not 0 <= class_mask < 2 ** 32:
        raise ValueError(f"object_boxes: n_class {n_class} in 1..32, min_area {min_area} >= 1, max_box {max_box} >= 1, frame0 {frame0} >= 0 "
                         f"and a 32-bit class_mask are required (SEGMIF_EINVAL)")
    lib = _lib.load()
    need = int(lib.segmif_object_boxes_workspace_bytes(n, H, W))
    if need <= 0:
        raise ValueError(f"object_boxes: at most {_lib.PASTE_MAX_FRAMES} frames of fewer than 2^31 pixels, got {tuple(root.shape)} (SEGMIF_EINVAL)")
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty(need // 4, device=root.device, dtype=torch.int32)
    _lib.check(lib.segmif_object_boxes_i32(root.data_ptr(), label.data_ptr(), n, H, W, int(n_class), int(class_mask), int(min_area),
                                           int(max_box), int(frame0), records.data_ptr() if records.shape[0] else None,
                                           records.shape[0], counter.data_ptr(), workspace.data_ptr(), _stream()),
               "segmif_object_boxes_i32")
    return workspace


def object_pack(records, offsets, patches, root, ir, vis, mask, frame0=0):
    """segmif_object_pack_u8: fills the patch store of the objects among `records` (M, 8) int32 (sorted, on the device) that lie in
    frames frame0 .. frame0 + n - 1, whose root maps `root` (n, H, W) int32 and uint8 frames ir, mask (n, H, W), vis (n, H, W, 3) are
    given.  offsets (M + 1,) int64: the objects' first pixels in patches (store_pixels, 8) uint8.  A pixel of an object's box is
    {ir, v0, v1, v2, mask, 1, 0, 0} where the frame's root is the object's, else eight zero bytes.  One launch."""
    _req_u8(records, "records", dtype=torch.int32)
    if records.dim() != 2 or records.shape[1] != PASTE_WORDS or records.shape[0] < 1:
        raise RuntimeError(f"object_pack: records must be (M, {PASTE_WORDS}) int32 with M >= 1, got {tuple(records.shape)}")
    M = records.shape[0]
    _req_u8(offsets, "offsets", (M + 1,), dtype=torch.int64)
    _req_u8(patches, "patches")
    if patches.dim() != 2 or patches.shape[1] != PASTE_WORDS:
        raise RuntimeError(f"object_pack: patches must be (pixels, {PASTE_WORDS}) uint8, got {tuple(patches.shape)}")
    _req_u8(root, "root", dtype=torch.int32)
    if root.dim() != 3 or root.numel() < 1:
        raise RuntimeError(f"object_pack: root must be a non-empty (n, H, W) int32 tensor, got {tuple(root.shape)}")
    n, H, W = (int(v) for v in root.shape)
    _req_u8(ir, "ir", (n, H, W)), _req_u8(mask, "mask", (n, H, W)), _req_u8(vis, "vis", (n, H, W, 3))
    _lib.check(_lib.load().segmif_object_pack_u8(records.data_ptr(), offsets.data_ptr(), M, patches.shape[0], root.data_ptr(),
                                                 ir.data_ptr(), vis.data_ptr(), mask.data_ptr(), int(frame0), n, H, W, patches.data_ptr(),
                                                 _stream()), "segmif_object_pack_u8")
    return patches


def check_paste_table(table, B, P=None):
    """Host-side check of a copy-paste table (it lives on the device when the kernel reads it): (B, P, 8) integers that fit int32,
    P in 0..8 (and equal to P when given) -> (B, P, 8) int32 numpy array.  The VALUES are not checked: a slot outside the kernel's
    domain is an empty slot by the rule."""
    import numpy as np
    t = np.asarray(table)
    if t.ndim != 3 or t.shape[0] != B or B < 1 or t.shape[2] != PASTE_WORDS or t.dtype.kind not in "iu":
        raise ValueError(f"copy_paste: the table must be ({B}, P, {PASTE_WORDS}) integers (obj, dx, dy, ow, oh, sx, sy, flip), got {t.dtype} {t.shape}")
    if t.shape[1] > PASTE_MAX_SLOTS or (P is not None and t.shape[1] != P):
        raise ValueError(f"copy_paste: P = {t.shape[1]} slots per sample, the kernel takes 0..{PASTE_MAX_SLOTS}" + (f" and {P} were announced" if P is not None else "")
                         + " (SEGMIF_EINVAL)")
    if t.size and ((t > 2 ** 31 - 1).any() or (t < -2 ** 31).any()):
        raise ValueError("copy_paste: a table value does not fit int32")
    return np.ascontiguousarray(t, dtype=np.int32)


def copy_paste(ir3, vis3, mask3, label, bank, table, n_class=9, tally=None):
    """Instance copy-paste on an augmented batch (the rule: include/segmif_paste.h, segmif_copy_paste_f32): every pixel takes the values
    of the LAST slot of its sample's table whose rectangle covers it and whose patch pixel belongs to the object (alpha = 1) - ir and
    mask in all three channels, vis per channel, each byte / 255 as augment_apply forms it WITHOUT photometric distortion, the label
    the object's class - and is the receiver's, bit for bit, where no slot does.  ir3, vis3, mask3 (B, 3, h, w) fp32, label (B, h, w)
    int64, w % 4 == 0.  bank: an object with records (M, 8) int32, offsets (M + 1,) int64 and patches (pixels, 8) uint8 device tensors
    (data.ObjectBank).  table: (B, P, 8) slots (obj, dx, dy, ow, oh, sx, sy, flip), either a host array / list, which is checked
    and uploaded here, or an int32 device tensor.  tally: None or an (n_class, 2) int64 device tensor that accumulates (non-empty
    slots, pixels pasted) per class.  One launch on the current stream, no synchronisation.  -> (ir3', vis3', mask3', label',
    pasted (B,) int64), new tensors.  NOT the reference's loader."""
    _req_u8(label, "label", dtype=torch.int64)
    if label.dim() != 3 or label.numel() < 1:
        raise RuntimeError(f"copy_paste: label must be a non-empty (B, h, w) int64 tensor, got {tuple(label.shape)}")
    B, h, w = label.shape
    if w % 4:
        raise RuntimeError(f"copy_paste: the width must be a multiple of 4 (16-byte accesses), got {w}")
    if not 1 <= n_class <= 255:
        raise ValueError(f"copy_paste: n_class {n_class} outside 1..255 (SEGMIF_EINVAL)")
    for t, name in ((ir3, "ir3"), (vis3, "vis3"), (mask3, "mask3")):
        _req_u8(t, name, (B, 3, h, w), dtype=torch.float32)
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        table = torch.from_numpy(check_paste_table(table.numpy() if isinstance(table, torch.Tensor) else table, B)).to(label.device)
    _req_u8(table, "table", dtype=torch.int32)
    if table.dim() != 3 or table.shape[0] != B or table.shape[2] != PASTE_WORDS or table.shape[1] > PASTE_MAX_SLOTS:
        raise RuntimeError(f"copy_paste: table must be ({B}, P <= {PASTE_MAX_SLOTS}, {PASTE_WORDS}) int32, got {tuple(table.shape)}")
    records, offsets, patches = bank.records, bank.offsets, bank.patches
    _req_u8(records, "bank.records", dtype=torch.int32)
    M = records.shape[0]
    if records.dim() != 2 or records.shape[1] != PASTE_WORDS or M < 1:
        raise RuntimeError(f"copy_paste: bank.records must be (M, {PASTE_WORDS}) int32 with M >= 1, got {tuple(records.shape)}")
    _req_u8(offsets, "bank.offsets", (M + 1,), dtype=torch.int64)
    _req_u8(patches, "bank.patches")
    if patches.dim() != 2 or patches.shape[1] != PASTE_WORDS or patches.shape[0] < 1:
        raise RuntimeError(f"copy_paste: bank.patches must be (pixels >= 1, {PASTE_WORDS}) uint8, got {tuple(patches.shape)}")
    if tally is not None:
        _req_u8(tally, "tally", (n_class, 2), dtype=torch.int64)
    P = table.shape[1]
    out = tuple(torch.empty_like(t) for t in (ir3, vis3, mask3, label))
    pasted = torch.empty(B, device=label.device, dtype=torch.int64)
    _lib.check(_lib.load().segmif_copy_paste_f32(ir3.data_ptr(), vis3.data_ptr(), mask3.data_ptr(), label.data_ptr(), B, h, w,
                                                 records.data_ptr(), offsets.data_ptr(), patches.data_ptr(), M, patches.shape[0],
                                                 table.data_ptr() if P else None, P, n_class, *(t.data_ptr() for t in out),
                                                 pasted.data_ptr(), tally.data_ptr() if tally is not None else None, _stream()),
               "segmif_copy_paste_f32")
    return out + (pasted,)
