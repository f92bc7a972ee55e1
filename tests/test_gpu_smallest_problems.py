"""GPU tests of the SMALLEST problems the C entry points accept: shorter than the kernels' pipelines, smaller than their tiles.
The Python dispatchers send such problems to the fp32 tiles (ops.PAIRS_MIN_ROWS, ops.GEMM_SPLIT_MIN_ROWS, N >= 128), so the
pipelined kernels behind them are called through the C ABI directly here.

Every family is compared with the fp64 CPU statement its existing test uses and is held to that test's bar - no tolerance is new:
    gemm_pairs              2e-6 of each output's conditioning sum |a||w| + |bias| + |res|     (tests/test_gpu_round5.py)
    gemm_split bf16x6/f16x3 TOL = 2e-5 of max |ref|, e <= 3 e32 + 1e-7 against the exact-fp32 igemm on the same problem, and 1e-6
                            of the conditioning for the plain product           (tests/test_gpu_kernels.py, tests/test_gpu_planes16.py)
    LayerNorm (three forms) TOL = 2e-5 of max |ref|; the PAIRS form decoded equals the fp32 kernel within one half-pair rounding,
                            2^-21 relative (2^-14 floor)                        (tests/test_gpu_kernels.py, tests/test_gpu_round5.py)
    depthwise conv, bilinear, upsum_act   TOL; the PAIRS depthwise conv: the two bounds of tests/test_gpu_round5.py, unchanged;
                            bilinear_argmax: the labels of the fp64 argmax (the sources have no ties)
    linear attention        1e-6 / 2e-6 of max |K^T V| (partial / fused with the kv projection), TOL and 1e-5 for the fold at 8 x 8 and
                            at the generic geometry, 5e-5 for its backward  (tests/test_gpu_kernels.py, test_gpu_round6.py, test_gpu_backward.py)
Every output goes into a NaN-filled buffer wider and longer than the result, which must stay NaN outside it - except where the
entry point takes no output pitch (the depthwise convs, conv3x3_c1 / c32to1, mixffn, the fp64 partial sums): those buffers are
only longer; and of a PAIRS result only the padding is looked at (its bytes are not floats).  The inputs come from
the existing rnd helper; a case's seed is the one of SEEDS whose fp64 reference has the largest positive entry against its own
conditioning (a property of the reference alone), and every compared reference is asserted to be non-zero.  The worst error of a family is recorded
through tests/_observed.py as smallest_*.

The bars of the remaining families:
    igemm                   TOL; tile 14 also within 2x of tile 10's error + 1e-7        (tests/test_gpu_kernels.py)
    planes convs            TOL of the arithmetic's own test file, e <= 2 e32 + 1e-7 against tile 10, 2e-6 of the conditioning for the
                            fused tail; conv3x3_c1 1e-6, conv3x3_c32to1 2e-6   (test_gpu_kernels.py, test_gpu_planes16.py, round6, round3)
    mixffn                  tests/test_gpu_round4.py's TOL and e <= 3 e32 + 2e-7 against the exact-fp32 chain
    attention               TOL forward, 2e-5 of each gradient's range backward   (tests/test_gpu_kernels.py, tests/test_gpu_round5.py)
    weight gradients        5e-5 (exact fp32), 2e-6 (both split arithmetics), 1e-5 for the fused bias sum; colsum 5e-5
    CrossPath               1e-6 / 2e-6 of max |G| (Gram / lazy Gram), TOL for fold and tails, the planes copy byte for byte"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _observed import observed
from test_gpu_kernels import TOL, act_ref, err, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEEDS = range(4)
ACTS = (0, 1, 2, 3)
SLOPE = 0.25
WORST = {}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import _lib, ops
    return _lib.load(), ops, _lib


def note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), float(value))
    observed("smallest_" + family, WORST[family])


def nan_out(rows, cols):
    """a NaN-filled buffer two rows longer and eight floats wider than the rows x cols result that is written at its start"""
    return torch.full((rows + 2, cols + 8), NAN, device="cuda")


def only_result_written(buf, rows, cols):
    return bool(torch.isfinite(buf[:rows, :cols]).all()) and bool(torch.isnan(buf[rows:]).all()) and bool(torch.isnan(buf[:rows, cols:]).all())


def pitched(t, extra):
    """a copy of the 2-D tensor t on the device as a view of rows `extra` floats wider (the rest NaN: nothing may read it)"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), NAN, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf, buf[:, :t.shape[1]]


def pick_seed(make):
    """make(seed) -> (inputs, ref, yard); the seed of SEEDS whose reference has the largest POSITIVE entry against its conditioning
    (positive: a ReLU of it is then not all zero either)"""
    best = None
    for s in SEEDS:
        inputs, ref, yard = make(s)
        score = float(ref.max() / yard.max())
        if best is None or score > best[0]:
            best = (score, inputs, ref, yard)
    assert best[0] > 0.0
    return best[1:]


def act64(y, act):
    return act_ref(y, act, SLOPE)


# ------------------------------------------------------------------------------------------------------------------ gemm_pairs
def pairs_encode(lib, ops, x):
    """fp32 (M, K) -> (pitched PAIRS buffer, its row pitch in bytes, the decoded values on the CPU: the truth's input)"""
    M, K = x.shape
    xd = x.cuda().contiguous()
    buf = torch.zeros((M, K + 16), device="cuda")
    st = ops._stream()
    assert lib.segmif_pairs_from_f32(xd.data_ptr(), K, buf.data_ptr(), 4 * (K + 16), M, K, None, 1, st) == 0
    back = torch.empty((M, K), device="cuda")
    assert lib.segmif_pairs_to_f32(buf.data_ptr(), 4 * (K + 16), back.data_ptr(), K, M, K, st) == 0
    return buf, 4 * (K + 16), back.cpu()


def pairs_weight(lib, ops, w):
    N, K = w.shape
    img = torch.empty((lib.segmif_gemm_pairs_weight_bytes(N, K),), device="cuda", dtype=torch.uint8)
    assert img.numel() > 0
    assert lib.segmif_gemm_pairs_pack(w.cuda().contiguous().data_ptr(), N, K, K, img.data_ptr(), ops._stream()) == 0
    return img


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("K", [16, 32, 48])
def test_gemm_pairs_below_one_tile_and_one_ring(env, K, tile):
    """K = 16, 32, 48: one, two and three steps of a ring issued two steps ahead; M = 1, 63, 129 and N = 4, 68, 132 around the
    64-row wave tile and the 128-column tile; every activation with and without the residual; A, out and res pitched."""
    lib, ops, L = env
    slope = torch.tensor([SLOPE], device="cuda")
    for M in (1, 63, 129):
        for N in (4, 68, 132):
            def make(s):
                x, w, b, r = rnd(M, K, seed=10 + s), rnd(N, K, seed=20 + s) * 0.1, rnd(N, seed=30 + s), rnd(M, N, seed=40 + s)
                lin = x.double() @ w.double().t() + b.double()
                return (x, w, b, r), lin, x.double().abs() @ w.double().abs().t() + b.double().abs()
            (x, w, b, r), _, _ = pick_seed(make)
            abuf, lda_bytes, back = pairs_encode(lib, ops, x)
            img, bd = pairs_weight(lib, ops, w), b.cuda()
            rbuf = pitched(r, 4)[0]
            lin = back.double() @ w.double().t() + b.double()
            yard0 = back.double().abs() @ w.double().abs().t() + b.double().abs()
            for act in ACTS:
                for use_res in (False, True):
                    buf = nan_out(M, N)
                    d = L.SegmifGemmPairs()
                    d.a, d.w, d.bias, d.out, d.prelu = abuf.data_ptr(), img.data_ptr(), bd.data_ptr(), buf.data_ptr(), slope.data_ptr()
                    d.M, d.lda_bytes, d.N, d.K, d.ldo, d.act, d.tile_rows = M, lda_bytes, N, K, buf.stride(0), act, tile
                    if use_res:
                        d.res, d.ldr = rbuf.data_ptr(), rbuf.stride(0)
                    assert lib.segmif_gemm_pairs_f32(ctypes.byref(d), ops._stream()) == 0
                    ref = act64(lin, act) + (r.double() if use_res else 0.0)
                    yard = yard0 + (r.double().abs() if use_res else 0.0)
                    assert float(ref.abs().max()) > 0.0  # (no case is judged on an all-zero reference)
                    got = buf.cpu()
                    e = float(((got[:M, :N].double() - ref).abs() / yard).max())
                    print(f"gemm_pairs M{M} N{N} K{K} tile{tile} act{act} res{int(use_res)}: {e:.3e}")
                    note("gemm_pairs", e)
                    assert only_result_written(got, M, N), (M, N, K, tile, act, use_res)
                    assert e < 2e-6, (M, N, K, tile, act, use_res, e)


@pytest.mark.parametrize("k,st,pad", [(3, 2, 1), (2, 2, 0)])
def test_gemm_pairs_patch_mode_on_an_image_smaller_than_the_kernel(env, k, st, pad):
    """Patch mode on 2 x 2 images of 16 channels: one output pixel per image, most taps of the 3 x 3 patch outside the image."""
    lib, ops, L = env
    B, H, W, C, N = 3, 2, 2, 16, 68
    K = k * k * C

    def make(s):
        x, w, b = rnd(B, H, W, C, seed=50 + s), rnd(N, C, k, k, seed=60 + s) * 0.1, rnd(N, seed=70 + s)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=st, padding=pad)
        yard = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs(), b.double().abs(), stride=st, padding=pad)
        return (x, w, b), ref, yard
    (x, w, b), _, _ = pick_seed(make)
    xd = x.cuda().view(B * H * W, C).contiguous()
    img_a, back = torch.zeros_like(xd), torch.empty_like(xd)
    st_ = ops._stream()
    assert lib.segmif_pairs_from_f32(xd.data_ptr(), C, img_a.data_ptr(), 4 * C, B * H * W, C, None, 1, st_) == 0
    assert lib.segmif_pairs_to_f32(img_a.data_ptr(), 4 * C, back.data_ptr(), C, B * H * W, C, st_) == 0
    back = back.cpu().view(B, H, W, C)
    wk = w.permute(0, 2, 3, 1).reshape(N, K).contiguous()  # (ky, kx, c) order
    img, bd = pairs_weight(lib, ops, wk), b.cuda()
    OH, OW = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    assert (OH, OW) == (1, 1)
    ref = F.conv2d(back.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=st, padding=pad).permute(0, 2, 3, 1).reshape(B, N)
    yard = F.conv2d(back.double().abs().permute(0, 3, 1, 2), w.double().abs(), b.double().abs(), stride=st, padding=pad).permute(0, 2, 3, 1).reshape(B, N)
    for tile in (128, 256):
        buf = nan_out(B, N)
        d = L.SegmifGemmPairs()
        d.a, d.w, d.bias, d.out = img_a.data_ptr(), img.data_ptr(), bd.data_ptr(), buf.data_ptr()
        d.M, d.lda_bytes, d.N, d.K, d.ldo, d.tile_rows = B, 4 * C, N, K, buf.stride(0), tile
        d.patch_k, d.patch_st, d.patch_pad, d.patch_H, d.patch_W, d.patch_C = k, st, pad, H, W, C
        assert lib.segmif_gemm_pairs_f32(ctypes.byref(d), st_) == 0
        got = buf.cpu()
        e = float(((got[:B, :N].double() - ref).abs() / yard).max())
        print(f"gemm_pairs patch k{k} s{st} p{pad} tile{tile}: {e:.3e}")
        note("gemm_pairs_patch", e)
        assert only_result_written(got, B, N) and e < 2e-6, (tile, e)


# ------------------------------------------------------------------------------------------------------------------ gemm_split
def split_weight(lib, ops, w, f16):
    N, K = w.shape
    size = (lib.segmif_gemm_split16_weight_bytes if f16 else lib.segmif_gemm_split_weight_bytes)(N, K)
    img = torch.empty((size,), device="cuda", dtype=torch.uint8)
    pack = lib.segmif_gemm_split16_pack if f16 else lib.segmif_gemm_split_pack
    assert size > 0 and pack(w.cuda().contiguous().data_ptr(), N, K, K, img.data_ptr(), ops._stream()) == 0
    return img


def run_split(lib, ops, d, f16):
    if f16:
        return lib.segmif_gemm_split16_f32(ctypes.byref(d), None, 1, ops._stream())
    return lib.segmif_gemm_split_f32(ctypes.byref(d), ops._stream())


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16x6", "f16x3"])
def test_gemm_split_below_one_tile(env, f16, K):
    """K = 32, 64: one and two steps; M = 1, 127, 129 and N = 4, 132 around the 128 x 128 tile; every activation with and without
    the residual; A, out and res pitched.  e32: the exact-fp32 igemm (ops.linear) on the same operands."""
    lib, ops, L = env
    name = "gemm_split_f16x3" if f16 else "gemm_split_bf16x6"
    slope = torch.tensor([SLOPE], device="cuda")
    for M in (1, 127, 129):
        for N in (4, 132):
            def make(s):
                x, w, b, r = rnd(M, K, seed=110 + s), rnd(N, K, seed=120 + s) * 0.1, rnd(N, seed=130 + s), rnd(M, N, seed=140 + s)
                lin = x.double() @ w.double().t() + b.double()
                return (x, w, b, r), lin, x.double().abs() @ w.double().abs().t() + b.double().abs()
            (x, w, b, r), lin, cond = pick_seed(make)
            abuf, av = pitched(x, 32)
            rbuf, rv = pitched(r, 4)
            img, bd, wt = split_weight(lib, ops, w, f16), b.cuda(), ops.pack_weight(w.cuda())
            for act in ACTS:
                for use_res in (False, True):
                    buf = nan_out(M, N)
                    d = L.SegmifGemmSplit()
                    d.a, d.w, d.bias, d.out, d.prelu = abuf.data_ptr(), img.data_ptr(), bd.data_ptr(), buf.data_ptr(), slope.data_ptr()
                    d.M, d.N, d.K, d.lda, d.ldo, d.act = M, N, K, abuf.stride(0), buf.stride(0), act
                    if use_res:
                        d.res, d.ldr = rbuf.data_ptr(), rbuf.stride(0)
                    assert run_split(lib, ops, d, f16) == 0
                    y32 = ops.linear(av, wt, N, bias=bd, act=act, prelu=slope if act == 2 else None, res=rv if use_res else None)
                    ref = act64(lin, act) + (r.double() if use_res else 0.0)
                    assert float(ref.abs().max()) > 0.0  # (no case is judged on an all-zero reference)
                    got = buf.cpu()
                    e, e32 = err(got[:M, :N], ref), err(y32, ref)
                    print(f"{name} M{M} N{N} K{K} act{act} res{int(use_res)}: e {e:.3e} e32 {e32:.3e}")
                    note(name, e)
                    assert only_result_written(got, M, N), (M, N, K, act, use_res)
                    assert e < TOL and e <= 3.0 * e32 + 1e-7, (M, N, K, act, use_res, e, e32)
                    if act == 0 and not use_res:
                        ec = float(((got[:M, :N].double() - lin).abs() / cond).max())
                        print(f"{name} M{M} N{N} K{K} conditioning-relative: {ec:.3e}")
                        note(name + "_cond", ec)
                        assert ec < 1e-6, (M, N, K, ec)


@pytest.mark.parametrize("k,st,pad", [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16x6", "f16x3"])
def test_gemm_split_patch_mode_on_an_image_smaller_than_the_kernel(env, f16, k, st, pad):
    """Patch mode on 2 x 2 images of 32 channels: one output pixel per image (see the gemm_pairs test of the same name)."""
    lib, ops, L = env
    B, H, W, C, N = 3, 2, 2, 32, 132
    K = k * k * C

    def make(s):
        x, w, b = rnd(B, H, W, C, seed=150 + s), rnd(N, C, k, k, seed=160 + s) * 0.1, rnd(N, seed=170 + s)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=st, padding=pad)
        yard = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs(), b.double().abs(), stride=st, padding=pad)
        return (x, w, b), ref.permute(0, 2, 3, 1).reshape(B, N), yard.permute(0, 2, 3, 1).reshape(B, N)
    (x, w, b), ref, yard = pick_seed(make)
    xd, bd = x.cuda().contiguous(), b.cuda()
    img = split_weight(lib, ops, w.permute(0, 2, 3, 1).reshape(N, K).contiguous(), f16)
    buf = nan_out(B, N)
    d = L.SegmifGemmSplit()
    d.a, d.w, d.bias, d.out = xd.data_ptr(), img.data_ptr(), bd.data_ptr(), buf.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldo = B, N, K, C, buf.stride(0)
    d.patch_k, d.patch_st, d.patch_pad, d.patch_H, d.patch_W = k, st, pad, H, W
    assert run_split(lib, ops, d, f16) == 0
    got = buf.cpu()
    e, ec = err(got[:B, :N], ref), float(((got[:B, :N].double() - ref).abs() / yard).max())
    name = "gemm_split_patch_f16x3" if f16 else "gemm_split_patch_bf16x6"
    print(f"{name} k{k} s{st} p{pad}: e {e:.3e} conditioning-relative {ec:.3e}")
    note(name, e)
    assert only_result_written(got, B, N) and e < TOL and ec < 1e-6, (e, ec)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def ln_inputs(rows, C):
    return rnd(rows, C, seed=19, lo=-3, hi=5), rnd(C, seed=20), rnd(C, seed=21)


@pytest.mark.parametrize("C", [4, 36, 1024])
@pytest.mark.parametrize("rows", [1, 3])
def test_layernorm_and_add_layernorm_on_one_and_three_rows(env, rows, C):
    """One and three rows (a block holds 256 / G of them), C = 4 (one vector), 36 (a ragged group) and 1024 (the widest form);
    every operand pitched.  add_layernorm: with and without the per-image scale, the sum held to the same bar."""
    lib, ops, L = env
    x, g, b = ln_inputs(rows, C)
    br, sc = rnd(rows, C, seed=22), rnd(rows, seed=23, lo=0.5, hi=1.5)
    gd, bd, scd = g.cuda(), b.cuda(), sc.cuda()
    xbuf, _ = pitched(x, 4)
    bbuf, _ = pitched(br, 8)
    st = ops._stream()
    for eps in (1e-6, 1e-5):
        buf = nan_out(rows, C)
        assert lib.segmif_layernorm_f32(xbuf.data_ptr(), gd.data_ptr(), bd.data_ptr(), buf.data_ptr(), rows, C, xbuf.stride(0), buf.stride(0), eps, st) == 0
        got = buf.cpu()
        e = err(got[:rows, :C], F.layer_norm(x.double(), (C,), g.double(), b.double(), eps))
        print(f"layernorm rows{rows} C{C} eps{eps}: {e:.3e}")
        note("layernorm", e)
        assert only_result_written(got, rows, C) and e < TOL, e
    for scaled in (False, True):
        buf = nan_out(rows, C)
        sbuf = nan_out(rows, C)
        rc = lib.segmif_add_layernorm_f32(xbuf.data_ptr(), bbuf.data_ptr(), scd.data_ptr() if scaled else None, 1, gd.data_ptr(), bd.data_ptr(),
                                          sbuf.data_ptr(), buf.data_ptr(), rows, C, xbuf.stride(0), bbuf.stride(0), sbuf.stride(0), buf.stride(0), 1e-5, st)
        assert rc == 0
        total = x.double() + (sc.double()[:, None] if scaled else 1.0) * br.double()
        got, gsum = buf.cpu(), sbuf.cpu()
        e, es = err(got[:rows, :C], F.layer_norm(total, (C,), g.double(), b.double(), 1e-5)), err(gsum[:rows, :C], total)
        print(f"add_layernorm rows{rows} C{C} scaled{int(scaled)}: y {e:.3e} sum {es:.3e}")
        note("add_layernorm", max(e, es))
        assert only_result_written(got, rows, C) and only_result_written(gsum, rows, C) and e < TOL and es < TOL, (e, es)


@pytest.mark.parametrize("C", [16, 48, 1024])
@pytest.mark.parametrize("rows", [1, 3])
def test_layernorm_pairs_on_one_and_three_rows(env, rows, C):
    """The PAIRS form: decoded, it is the fp32 kernel's result within one half-pair rounding and the fp64 LayerNorm within TOL; its
    rows are C * 4 bytes of a pitched buffer whose padding stays NaN."""
    lib, ops, L = env
    x, g, b = ln_inputs(rows, C)
    gd, bd = g.cuda(), b.cuda()
    xbuf, _ = pitched(x, 4)
    st = ops._stream()
    buf = nan_out(rows, C)
    rc = lib.segmif_layernorm_pairs_f32(xbuf.data_ptr(), gd.data_ptr(), bd.data_ptr(), buf.data_ptr(), rows, C, xbuf.stride(0), buf.stride(0), 1e-5,
                                        None, 1, 1, 1, st)
    assert rc == 0
    raw = buf.cpu()
    assert bool(torch.isnan(raw[rows:]).all()) and bool(torch.isnan(raw[:rows, C:]).all())  # (the pairs bytes themselves are not floats)
    dec = torch.empty((rows, C), device="cuda")
    assert lib.segmif_pairs_to_f32(buf.data_ptr(), 4 * buf.stride(0), dec.data_ptr(), C, rows, C, st) == 0
    y32 = torch.empty((rows, C), device="cuda")
    assert lib.segmif_layernorm_f32(xbuf.data_ptr(), gd.data_ptr(), bd.data_ptr(), y32.data_ptr(), rows, C, xbuf.stride(0), C, 1e-5, st) == 0
    a, r32 = dec.double().cpu(), y32.double().cpu()
    half = float(((a - r32).abs() / (r32.abs() + 2.0 ** -14)).max())
    e = err(dec, F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5))
    print(f"layernorm_pairs rows{rows} C{C}: vs fp32 kernel {half:.3e}, vs fp64 {e:.3e}")
    note("layernorm_pairs", e)
    assert half < 2.0 ** -21 and e < TOL, (half, e)


# ------------------------------------------------------------------------------------------------- the other row kernels
DW_SHAPES = [(1, 1), (1, 17), (17, 1), (2, 16)]  # one pixel; one row / one column around the 16-wide switch to the two-column kernel


def dw_case(B, H, W, C):
    x, w, b = rnd(B, H * W, C, seed=22, lo=-2, hi=2), rnd(C, 1, 3, 3, seed=23), rnd(C, seed=24)
    img = x.double().transpose(1, 2).reshape(B, C, H, W)
    pre = F.conv2d(img, w.double(), b.double(), padding=1, groups=C).flatten(2).transpose(1, 2).reshape(B * H * W, C)
    cond = F.conv2d(img.abs(), w.double().abs(), b.double().abs(), padding=1, groups=C).flatten(2).transpose(1, 2).reshape(B * H * W, C)
    return x, w, b, pre, cond


def dense_nan(rows, C):
    return torch.full((rows + 2, C), NAN, device="cuda")


@pytest.mark.parametrize("H,W", DW_SHAPES)
def test_depthwise_conv_on_images_of_one_row_or_column(env, H, W):
    """Depthwise 3 x 3 with GELU, with bias only, and the PAIRS form (C = 16) on images where most taps fall outside; two images."""
    lib, ops, L = env
    B, st = 2, ops._stream()
    rows = B * H * W
    x, w, b, pre, _ = dw_case(B, H, W, 4)
    xd, w9, bd = x.cuda().contiguous(), ops.pack_dw_weight(w.cuda()), b.cuda()
    for name, fn, ref in (("dwconv_gelu", lib.segmif_dwconv3x3_gelu_f32, F.gelu(pre)), ("dwconv_bias", lib.segmif_dwconv3x3_bias_f32, pre)):
        buf = dense_nan(rows, 4)
        assert fn(xd.data_ptr(), w9.data_ptr(), bd.data_ptr(), buf.data_ptr(), B, H, W, 4, st) == 0
        got = buf.cpu()
        e = err(got[:rows], ref)
        print(f"{name} {H}x{W}: {e:.3e}")
        note(name, e)
        assert bool(torch.isnan(got[rows:]).all()) and e < TOL, (name, e)
    C = 16
    x, w, b, pre, cond = dw_case(B, H, W, C)
    xd, w9, bd = x.cuda().contiguous(), ops.pack_dw_weight(w.cuda()), b.cuda()
    buf, y32, dec = dense_nan(rows, C), torch.empty((rows, C), device="cuda"), torch.empty((rows, C), device="cuda")
    assert lib.segmif_dwconv3x3_gelu_pairs_f32(xd.data_ptr(), w9.data_ptr(), bd.data_ptr(), buf.data_ptr(), B, H, W, C, None, 1, st) == 0
    assert lib.segmif_dwconv3x3_gelu_f32(xd.data_ptr(), w9.data_ptr(), bd.data_ptr(), y32.data_ptr(), B, H, W, C, st) == 0
    assert lib.segmif_pairs_to_f32(buf.data_ptr(), 4 * C, dec.data_ptr(), C, rows, C, st) == 0
    assert bool(torch.isnan(buf.cpu()[rows:]).all())
    got, r32 = dec.double().cpu(), y32.double().cpu()
    ref64 = 0.5 * pre * (1.0 + torch.erf(pre * 0.70710678118654752440))
    # the two bounds of tests/test_gpu_round5.py::test_pairs_producers_match_their_fp32_kernels_and_report_ranges
    w32 = float(((got - r32).abs() / (2.0 ** -21 * r32.abs() + 1.0e-7 * pre.abs() + 2.0 ** -35)).max())
    w64 = float(((got - ref64).abs() / (2.0 ** -20 * ref64.abs() + 4.0e-7 * cond + 2.0 ** -30)).max())
    print(f"dwconv_gelu_pairs {H}x{W}: against the fp32 kernel {w32:.3f} of its bound, against fp64 {w64:.3f} of its bound")
    note("dwconv_gelu_pairs_of_bound", max(w32, w64))
    assert w32 < 1.0 and w64 < 1.0, (w32, w64)


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("IH,IW,OH,OW", [(1, 1, 5, 7), (5, 7, 1, 1)])
def test_bilinear_from_and_to_a_single_pixel(env, IH, IW, OH, OW, C):
    """1 x 1 -> 5 x 7 (every tap clamps to the one source pixel) and 5 x 7 -> 1 x 1; C = 1 (scalar path) and 4 (16-byte path); pitched."""
    lib, ops, L = env
    B = 2
    x = rnd(B, IH, IW, C, seed=25)
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), size=[OH, OW], mode="bilinear", align_corners=False).permute(0, 2, 3, 1).reshape(B * OH * OW, C)
    xbuf, _ = pitched(x.view(B * IH * IW, C), 4)
    buf = nan_out(B * OH * OW, C)
    assert lib.segmif_bilinear_nhwc_f32(xbuf.data_ptr(), buf.data_ptr(), B, IH, IW, OH, OW, C, xbuf.stride(0), buf.stride(0), ops._stream()) == 0
    got = buf.cpu()
    e = err(got[:B * OH * OW, :C], ref)
    print(f"bilinear {IH}x{IW}->{OH}x{OW} C{C}: {e:.3e}")
    note("bilinear", e)
    assert only_result_written(got, B * OH * OW, C) and e < TOL, e


def test_upsum_act_and_bilinear_argmax_with_single_pixel_sources(env):
    """upsum_act over three 1 x 1 sources (plus a pitched base, the bias and the ReLU) and bilinear_argmax of a 1 x 1 map."""
    lib, ops, L = env
    B, OH, OW, C, st = 2, 3, 5, 4, ops._stream()
    rows = B * OH * OW
    srcs = [rnd(B, 1, 1, C, seed=81 + i) for i in range(3)]
    base, bias = rnd(rows, C, seed=84), rnd(C, seed=85)
    ref = F.relu(base.double().view(B, OH * OW, C) + bias.double() + sum(s.double().view(B, 1, C) for s in srcs)).reshape(rows, C)
    bbuf, _ = pitched(base, 4)
    sd, bd = [s.cuda().contiguous() for s in srcs], bias.cuda()
    buf = nan_out(rows, C)
    rc = lib.segmif_upsum_act_nhwc_f32(bbuf.data_ptr(), bbuf.stride(0), sd[0].data_ptr(), 1, 1, sd[1].data_ptr(), 1, 1, sd[2].data_ptr(), 1, 1, bd.data_ptr(),
                                       buf.data_ptr(), buf.stride(0), B, OH, OW, C, 1, st)
    assert rc == 0
    got = buf.cpu()
    e = err(got[:rows, :C], ref)
    print(f"upsum_act 1x1 sources: {e:.3e}")
    note("upsum_act", e)
    assert only_result_written(got, rows, C) and e < TOL, e
    Cl = 9
    x = rnd(B, Cl, seed=86)
    xbuf, _ = pitched(x, 4)
    labels = torch.full((rows + 2,), -7, device="cuda", dtype=torch.int32)
    assert lib.segmif_bilinear_argmax_i32(xbuf.data_ptr(), labels.data_ptr(), B, 1, 1, OH, OW, Cl, xbuf.stride(0), st) == 0
    lab = labels.cpu()
    assert bool((lab[rows:] == -7).all())
    assert torch.equal(lab[:rows].view(B, OH * OW).long(), x.double().argmax(1)[:, None].expand(B, OH * OW))


# ------------------------------------------------------------------------------------------------------------ linear attention
BWD_TOL = 5e-5  # tests/test_gpu_backward.py


def f64_nan(n):
    return torch.full((n,), NAN, device="cuda", dtype=torch.float64)


@pytest.mark.parametrize("heads,d", [(8, 8), (8, 4)])
@pytest.mark.parametrize("N", [1, 31, 32, 33])
def test_linear_attention_on_less_than_two_runs_of_rows(env, N, heads, d):
    """partial / kvpartial / fold / fold_bwd with N = 1, 31, 32, 33 tokens (the kernels sum in fp32 inside a 32-row run and in fp64
    across runs: one row, one short of a run, one run, one over) at 8 heads of 8 (16-byte loads) and 8 heads of 4 (the generic kernels).
    Bars: 1e-6 of max |K^T V| for the partial sums (2e-6 fused with the kv projection), TOL / 1e-5 for the fold (the 8 x 8 / the
    generic test's), 5e-5 for its backward."""
    lib, ops, L = env
    B, C, st = 2, heads * d, ops._stream()
    E, scale = C * d, d ** -0.5
    tag = f"{heads}x{d} N{N}"
    kv = rnd(B, N, 2 * C, seed=30 + N)
    kbuf, _ = pitched(kv.view(B * N, 2 * C), 4)
    k = kv[..., :C].double().view(B, N, heads, d).permute(0, 2, 1, 3)
    v = kv[..., C:].double().view(B, N, heads, d).permute(0, 2, 1, 3)
    ktv = k.transpose(-2, -1) @ v  # (B, heads, d, d)
    assert lib.segmif_linattn_num_blocks(N) == 1
    part = f64_nan(B * E + 8)
    assert lib.segmif_linattn_partial_f32(kbuf.data_ptr(), part.data_ptr(), B, N, heads, d, kbuf.stride(0), st) == 0
    got = part.cpu()
    e = err(got[:B * E].view(B, heads, d, d), ktv)
    print(f"linattn_partial {tag}: {e:.3e}")
    note("linattn_partial", e)
    assert bool(torch.isnan(got[B * E:]).all()) and e < 1e-6, e
    if (heads, d) == (8, 8):  # the fused kv projection exists at this geometry only
        p = rnd(B, N, 2 * C, seed=40 + N, lo=0.0, hi=1.0)
        wkv = rnd(2 * C, C, seed=41, lo=-0.3, hi=0.3)
        pd, wd = p.cuda(), wkv.cuda()
        kvp = (p[..., :C].double() @ wkv.double().t()).reshape(B, N, 2, 8, 8)
        raw = kvp[:, :, 0].permute(0, 2, 1, 3).transpose(-2, -1) @ kvp[:, :, 1].permute(0, 2, 1, 3)
        part2 = f64_nan(B * 512 + 8)
        assert lib.segmif_linattn_kvpartial_f32(pd.data_ptr(), wd.data_ptr(), part2.data_ptr(), B, N, 8, 8, 2 * C, st) == 0
        got = part2.cpu()
        e = err(got[:B * 512].view(B, 8, 8, 8), raw)
        print(f"linattn_kvpartial {tag}: {e:.3e}")
        note("linattn_kvpartial", e)
        assert bool(torch.isnan(got[B * 512:]).all()) and e < 2e-6, e
    # the fold and its backward on the fp64 K^T V of these N rows (one partial per image)
    Nout = 48
    wend, dweff = rnd(Nout, 2 * C, seed=7), rnd(B, Nout, 2 * C, seed=8)
    wd_, ktv_d = wend.cuda(), ktv.contiguous().cuda()
    ctx = torch.softmax(ktv * scale, dim=-2)
    we = wend.double()[:, C:].view(Nout, heads, d)
    want = torch.einsum("bhij,nhj->bnhi", ctx, we).reshape(B * Nout, C)
    buf = torch.full((B * Nout + 2, 2 * C + 8), NAN, device="cuda")
    assert lib.segmif_linattn_fold_f32(ktv_d.data_ptr(), wd_.data_ptr(), buf.data_ptr(), B, 1, heads, d, Nout, 2 * C, C, buf.stride(0), C, scale, st) == 0
    got = buf.cpu()
    e = err(got[:B * Nout, C:2 * C], want)
    print(f"linattn_fold {tag}: {e:.3e}")
    note("linattn_fold", e)
    outside = got.clone()
    outside[:B * Nout, C:2 * C] = NAN
    assert bool(torch.isnan(outside).all()) and e < (TOL if (heads, d) == (8, 8) else 1e-5), e
    dw = dweff.double()[..., C:].view(B, Nout, heads, d)                                  # dWeff[b][n][kofs + h d + i]
    dctx = torch.einsum("bnhi,nhj->bhij", dw, we)
    want_dktv = scale * ctx * (dctx - (ctx * dctx).sum(dim=-2, keepdim=True))
    want_dwend = torch.einsum("bnhi,bhij->bnhj", dw, ctx).reshape(B * Nout, C)
    dktv = f64_nan(B * E + 8)
    pbuf = torch.full((B * Nout + 2, 2 * C + 8), NAN, device="cuda")
    dd = dweff.cuda()
    rc = lib.segmif_linattn_fold_bwd_f32(ktv_d.data_ptr(), wd_.data_ptr(), 2 * C, C, dd.data_ptr(), 2 * C, C, scale, dktv.data_ptr(), pbuf.data_ptr(),
                                         pbuf.stride(0), B, Nout, heads, d, st)
    assert rc == 0
    gk, gp = dktv.cpu(), pbuf.cpu()
    e1, e2 = err(gk[:B * E].view(B, heads, d, d), want_dktv), err(gp[:B * Nout, C:2 * C], want_dwend)
    print(f"linattn_fold_bwd {tag}: dktv {e1:.3e} dwend {e2:.3e}")
    note("linattn_fold_bwd", max(e1, e2))
    outside = gp.clone()
    outside[:B * Nout, C:2 * C] = NAN
    assert bool(torch.isnan(gk[B * E:]).all()) and bool(torch.isnan(outside).all()) and e1 < BWD_TOL and e2 < BWD_TOL, (e1, e2)


# ----------------------------------------------------------------------------------------------------------------------- igemm
from test_gpu_kernels import TILES_ALL, _planes_decode  # noqa: E402


def nhwc(x):
    """NCHW on the CPU -> a contiguous NHWC device tensor with canonical strides (torch keeps the permuted strides of size-1
    dimensions through .contiguous(), which ops.rows_view does not take for a rows view)"""
    B, C, H, W = x.shape
    t = torch.empty((B, H, W, C), device="cuda")
    t.copy_(x.permute(0, 2, 3, 1))
    return t


def view4(buf, B, OH, OW, N):
    """the (B, OH, OW, N) rows view at the start of a NaN buffer of nan_out(B * OH * OW, N)"""
    ld = buf.stride(0)
    return torch.as_strided(buf, (B, OH, OW, N), (OH * OW * ld, OW * ld, ld, 1))


def test_igemm_one_row_one_column_and_three_deep(env):
    """M = 1 on every tile of TILES_ALL (every activation path the existing test takes), N = 1 on every tile, K = 3 (the generic
    gather); pitched A and res, NaN-padded out."""
    lib, ops, L = env
    for M, N, K, tiles in ((1, 64, 64, TILES_ALL), (33, 1, 64, TILES_ALL), (1, 1, 64, TILES_ALL), (33, 8, 3, [-1]), (1, 4, 3, [-1])):
        def make(s):
            x, w, b, r = rnd(M, K, seed=1 + s), rnd(N, K, seed=2 + s), rnd(N, seed=3 + s), rnd(M, N, seed=4 + s)
            lin = x.double() @ w.double().t() + b.double()
            return (x, w, b, r), lin, x.double().abs() @ w.double().abs().t() + b.double().abs()
        (x, w, b, r), lin, _ = pick_seed(make)
        av, rv = pitched(x, 4)[1], pitched(r, 4)[1]
        wt, bd = ops.pack_weight(w.cuda()), b.cuda()
        for tile in tiles:
            for act, use_res in ((0, False), (1, True), (3, False)):
                ref = act64(lin, act) + (r.double() if use_res else 0.0)
                assert float(ref.abs().max()) > 0.0
                buf = nan_out(M, N)
                ops.linear(av, wt, N, bias=bd, act=act, res=rv if use_res else None, tile=tile, out=buf[:M, :N])
                got = buf.cpu()
                e = err(got[:M, :N], ref)
                note("igemm_dense", e)
                assert only_result_written(got, M, N) and e < TOL, (M, N, K, tile, act, use_res, e)
    print("igemm dense worst:", WORST["igemm_dense"])


@pytest.mark.parametrize("H,W", [(1, 1), (2, 1)])
@pytest.mark.parametrize("Cin,k,s,p", [(16, 3, 1, 1), (3, 7, 4, 3)])
def test_igemm_conv_on_images_smaller_than_the_kernel(env, Cin, k, s, p, H, W):
    """3 x 3 pad 1 and the stage-1 patch embed (7 x 7, stride 4, pad 3; scalar gather) on 1 x 1 and 2 x 1 images."""
    lib, ops, L = env
    B, N = 2, 32
    x, w, b = rnd(B, Cin, H, W, seed=13), rnd(N, Cin, k, k, seed=14), rnd(N, seed=15)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p).permute(0, 2, 3, 1)
    OH, OW = ref.shape[1], ref.shape[2]
    xh, wt = nhwc(x), ops.pack_weight(w.cuda())
    for tile in ([-1] if Cin % 16 else list(TILES_ALL)):
        if tile in (1, 3, 5, 8, 11) and Cin % 32:
            continue
        buf = nan_out(B * OH * OW, N)
        ops.conv2d(xh, wt, N, k, stride=s, pad=p, bias=b.cuda(), tile=tile, out=view4(buf, B, OH, OW, N))
        got = buf.cpu()
        e = err(got[:B * OH * OW, :N], ref.reshape(B * OH * OW, N))
        print(f"igemm conv k{k} s{s} p{p} {H}x{W} tile{tile}: {e:.3e}")
        note("igemm_conv", e)
        assert only_result_written(got, B * OH * OW, N) and e < TOL, (tile, e)


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
def test_halo_and_split_tiles_on_images_smaller_than_one_patch(env, H, W, dil):
    """Tiles 9, 10 (halo-tiled fp32) and 14 (split bf16x6) work on 8 x 32 patches: a 1 x 1 and a 3 x 5 image at dilation 1 and 2.
    Tile 14's bar: TOL and within 2x of tile 10's error (+1e-7), as tests/test_gpu_kernels.py::test_conv3x3_split_bf16x6."""
    lib, ops, L = env
    B, Cin, N = 2, 16, 32
    x, w, b = rnd(B, Cin, H, W, seed=13), rnd(N, Cin, 3, 3, seed=14), rnd(N, seed=15)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil).permute(0, 2, 3, 1).reshape(B * H * W, N)
    xh = nhwc(x)
    errs = {}
    for tile, wt in ((9, ops.pack_weight(w.cuda())), (10, ops.pack_weight(w.cuda())), (14, ops.pack_weight_split(w.cuda()))):
        buf = nan_out(B * H * W, N)
        ops.conv2d(xh, wt, N, 3, pad=dil, dil=dil, bias=b.cuda(), tile=tile, out=view4(buf, B, H, W, N))
        got = buf.cpu()
        errs[tile] = err(got[:B * H * W, :N], ref)
        print(f"tile {tile} {H}x{W} dil{dil}: {errs[tile]:.3e}")
        note("igemm_halo_tiles", errs[tile])
        assert only_result_written(got, B * H * W, N) and errs[tile] < TOL, (tile, errs[tile])
    assert errs[14] <= 2.0 * errs[10] + 1e-7, errs


def test_igemm_at_the_split_k_threshold(env):
    """The smallest K at which the split-K plan engages for a 64 x 64 output (found from segmif_igemm_workspace_floats, a host query) and
    one K step of 16 below it."""
    lib, ops, L = env
    M, N = 64, 64

    def need(K):
        x, wt, out = torch.empty(M, K, device="cuda"), torch.empty(N, K, device="cuda"), torch.empty(M, N, device="cuda")
        d = L.SegmifIgemm()
        d.in_, d.wt, d.out = x.data_ptr(), wt.data_ptr(), out.data_ptr()
        d.M, d.N, d.K, d.lda, d.ldo, d.Cin = M, N, K, K, N, K
        d.H = d.W = d.OH = d.OW = d.KH = d.KW = d.stride = d.dil = 1
        d.tile = -1
        return lib.segmif_igemm_workspace_floats(ctypes.byref(d))
    K0 = next(K for K in range(16, 2049, 16) if need(K) > 0)
    assert K0 > 16 and need(K0 - 16) == 0
    for K in (K0 - 16, K0):
        x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3)
        ref = x.double() @ w.double().t() + b.double()
        buf = nan_out(M, N)
        ops.linear(x.cuda(), ops.pack_weight(w.cuda()), N, bias=b.cuda(), out=buf[:M, :N])
        got = buf.cpu()
        e = err(got[:M, :N], ref)
        print(f"igemm split-K threshold K{K} (workspace {need(K)} floats): {e:.3e}")
        note("igemm_splitk", e)
        assert only_result_written(got, M, N) and e < TOL, (K, e)


# ---------------------------------------------------------------------------------------------------------------- planes convs
PLANE_SIZES = [(1, 1), (3, 5), (7, 31), (9, 33)]  # one pixel, inside one 8 x 32 patch, one short of it, one over in both directions


@pytest.mark.parametrize("f16", [False, True], ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("H,W", PLANE_SIZES)
def test_planes_convs_on_images_around_one_patch(env, H, W, f16):
    """conv3x3_planes (both arithmetics) with cin 16 and 64 at dilation 1 and 2: the plain conv (fp32 rows into a NaN-padded buffer
    and two more planes chunks, nothing outside the interior) and the fused DRDB tail.  Bars of the existing tests: TOL of the
    arithmetic's own test file, e <= 2 e32 + 1e-7 against tile 10 (plain), 2e-6 of the conditioning (fused tail)."""
    lib, ops, L = env
    import test_gpu_planes16 as t16
    tol = t16.TOL if f16 else TOL
    B, name = 2, "planes_f16x3" if f16 else "planes_bf16x6"
    pack = ops.pack_weight_planes16 if f16 else ops.pack_weight_planes
    for Cin in (16, 64):
        for dil in (1, 2):
            x, w, b = rnd(B, Cin, H, W, seed=13), rnd(32, Cin, 3, 3, seed=14), rnd(32, seed=15)
            ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil)).permute(0, 2, 3, 1)
            assert float(ref.abs().max()) > 0.0
            xh = nhwc(x)
            y32 = ops.conv2d(xh, ops.pack_weight(w.cuda()), 32, 3, pad=dil, dil=dil, bias=b.cuda(), act=1, tile=10)
            guard = ops.Planes16Guard("cuda") if f16 else None
            pl = ops.Planes(B, H, W, Cin // 16 + 2, "cuda", guard).load_f32(xh)
            buf = nan_out(B * H * W, 32)
            ops.conv3x3_planes(pl, Cin, pack(w.cuda()), dil=dil, bias=b.cuda(), act=1, out_chunk0=Cin // 16, out=view4(buf, B, H, W, 32))
            got = buf.cpu()
            e, e32 = err(got[:B * H * W, :32], ref.reshape(B * H * W, 32)), err(y32, ref)
            print(f"{name} {H}x{W} cin{Cin} dil{dil}: e {e:.3e} e32 {e32:.3e}")
            note(name, e)
            assert only_result_written(got, B * H * W, 32) and e < tol and e <= 2.0 * e32 + 1e-7, (Cin, dil, e, e32)
            dec, raw = (t16._decode if f16 else _planes_decode)(pl, Cin // 16, 2)
            assert float((dec - ref).abs().max() / ref.abs().max()) < tol
            mask = torch.ones_like(raw, dtype=torch.bool)
            mask[:, :, 2:2 + H, 2:2 + W] = False
            assert float(raw[mask].abs().max()) == 0.0  # nothing written outside the H x W interior
            # the fused tail: out1 = res + relu(W1 . [in | relu(conv)] + b1)
            w1, b1, res = rnd(64, Cin + 32, seed=33) * 0.1, rnd(64, seed=34), rnd(B, H, W, 64, seed=35)
            xd = x.double()
            mid = F.relu(F.conv2d(xd, w.double(), b.double(), padding=dil, dilation=dil))
            pre = F.conv2d(torch.cat((xd, mid), dim=1), w1.double()[:, :, None, None], b1.double())
            ref1 = (res.double().permute(0, 3, 1, 2) + F.relu(pre)).permute(0, 2, 3, 1).reshape(B * H * W, 64)
            cond = (F.conv2d(torch.cat((xd.abs(), mid.abs()), dim=1), w1.double().abs()[:, :, None, None]).permute(0, 2, 3, 1)
                    + res.double().abs()).reshape(B * H * W, 64)
            pl2 = ops.Planes(B, H, W, Cin // 16, "cuda", guard).load_f32(xh)
            rbuf = pitched(res.view(B * H * W, 64), 4)[0]
            buf1 = nan_out(B * H * W, 64)
            ops.conv3x3_planes(pl2, Cin, pack(w.cuda()), dil=dil, bias=b.cuda(), act=1,
                               tail=(pack(w1.cuda()), b1.cuda(), view4(rbuf, B, H, W, 64), view4(buf1, B, H, W, 64), 1))
            got = buf1.cpu()
            e1 = err(got[:B * H * W, :64], ref1)
            ec = float(((got[:B * H * W, :64].double() - ref1).abs() / (cond + 1e-30)).max())
            print(f"{name} fused tail {H}x{W} cin{Cin} dil{dil}: e {e1:.3e} conditioning-relative {ec:.3e}")
            note(name + "_fused_tail", e1)
            assert only_result_written(got, B * H * W, 64) and e1 < tol and ec < 2e-6, (Cin, dil, e1, ec)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3)])
def test_one_channel_stencils_on_tiny_images(env, H, W):
    """conv3x3_c1 (1 -> 64, fp32 rows and the f16x3 planes copy) and conv3x3_c32to1 (32 -> 1) on 1 x 1 and 2 x 3 images; bars 1e-6 and
    2e-6 of max |ref| (tests/test_gpu_round6.py, tests/test_gpu_round3.py).  Their outputs take no pitch: the buffers are only longer."""
    lib, ops, L = env
    B, st = 2, ops._stream()
    rows = B * H * W
    x, w, bias = rnd(B, H, W, 1, seed=61), rnd(64, 1, 3, 3, seed=62) * 0.5, rnd(64, seed=63)
    slope = torch.tensor([SLOPE], device="cuda")
    want = F.prelu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), padding=1), torch.tensor([SLOPE], dtype=torch.float64))
    want = want.permute(0, 2, 3, 1).reshape(rows, 64)
    guard = ops.Planes16Guard("cuda", B)
    pl, ref_pl = ops.Planes(B, H, W, 8, "cuda", guard), ops.Planes(B, H, W, 8, "cuda", guard)
    xd, wd, bd = x.cuda().contiguous(), w.cuda().contiguous(), bias.cuda()
    buf = torch.full((rows + 2, 64), NAN, device="cuda")
    amax, nimg = guard.slot(B)
    rc = lib.segmif_conv3x3_c1_f16x3(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), slope.data_ptr(), 2, pl.data.data_ptr(), 8, 4, buf.data_ptr(), 64,
                                     B, H, W, amax, nimg, st)
    assert rc == 0
    got = buf.cpu()
    e = err(got[:rows], want)
    print(f"conv3x3_c1 {H}x{W}: {e:.3e}")
    note("conv3x3_c1", e)
    assert bool(torch.isnan(got[rows:]).all()) and e < 1e-6, e
    ref_pl.load_f32(buf[:rows].view(B, H, W, 64), 4)  # the planes copy is bit for bit what planes16_from_f32 makes of the rows
    cb = pl.data.numel() // (B * 8)
    assert torch.equal(pl.data.view(B, 8, cb)[:, 4:8], ref_pl.data.view(B, 8, cb)[:, 4:8])
    x2, w2, b2 = rnd(B, H, W, 32, seed=64), rnd(1, 32, 3, 3, seed=65) * 0.3, torch.tensor([0.07])
    ref0 = F.conv2d(x2.double().permute(0, 3, 1, 2), w2.double(), b2.double(), padding=1).reshape(rows)
    xbuf = pitched(x2.view(rows, 32), 16)[0]
    wt2, b2d = ops.pack_weight(w2.cuda()), b2.cuda()
    for act, ref in ((2, torch.where(ref0 >= 0, ref0, SLOPE * ref0)), (1, ref0.clamp(min=0)), (0, ref0)):
        out = torch.full((rows + 8,), NAN, device="cuda")
        rc = lib.segmif_conv3x3_c32to1_f32(xbuf.data_ptr(), xbuf.stride(0), wt2.data_ptr(), b2d.data_ptr(), slope.data_ptr(), act, out.data_ptr(),
                                           B, H, W, st)
        assert rc == 0
        got = out.cpu()
        e = float((got[:rows].double() - ref).abs().max() / (ref0.abs().max() + 1e-30))
        print(f"conv3x3_c32to1 {H}x{W} act{act}: {e:.3e}")
        note("conv3x3_c32to1", e)
        assert bool(torch.isnan(got[rows:]).all()) and bool(torch.isfinite(got[:rows]).all()) and e < 2e-6, (act, e)


# ---------------------------------------------------------------------------------------------------------------------- mixffn
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H,W", [(1, 1), (11, 15), (12, 16), (13, 17)])
def test_mixffn_around_one_tile(env, H, W, C):
    """The fused Mix-FFN's tiles are 12 x 16: one pixel, one short of a tile, one tile, one over.  Bars of
    tests/test_gpu_round4.py::test_mixffn_fused_kernel: its TOL and e <= 3 e32 + 2e-7 against the exact-fp32 chain.  The output takes
    no pitch: the buffer is only longer; x must be left untouched."""
    lib, ops, L = env
    import test_gpu_round4 as t4
    B, hid, eps = 2, 4 * C, 1e-6
    x = rnd(B, H * W, C, seed=C + H) * 10.0 ** rnd(B, H * W, 1, seed=3, lo=-1, hi=1)
    gamma, beta = rnd(C, seed=4, lo=0.5, hi=1.5), rnd(C, seed=5) * 0.2
    w1, b1 = rnd(hid, C, seed=6) * 0.2 * 10.0 ** rnd(hid, 1, seed=7, lo=-1, hi=0.5), rnd(hid, seed=8) * 0.3
    wd, bd = rnd(hid, 1, 3, 3, seed=9) * 0.5, rnd(hid, seed=10) * 0.2
    w2, b2 = rnd(C, hid, seed=11) * 0.1 * 10.0 ** rnd(C, 1, seed=12, lo=-1, hi=0.5), rnd(C, seed=13) * 0.3
    xd = x.double()
    n = F.layer_norm(xd, (C,), gamma.double(), beta.double(), eps)
    img = (n @ w1.double().t() + b1.double()).transpose(1, 2).reshape(B, hid, H, W)
    g = F.gelu(F.conv2d(img, wd.double(), bd.double(), padding=1, groups=hid).flatten(2).transpose(1, 2))
    ref = (xd + g @ w2.double().t() + b2.double()).reshape(B * H * W, C)
    xc = x.cuda().contiguous()
    keep = xc.clone()
    gm, bt, b2d = gamma.cuda(), beta.cuda(), b2.cuda()
    dw9 = ops.pack_dw_weight(wd.cuda())
    wimg = ops.pack_mixffn(w1.cuda(), b1.cuda(), dw9, bd.cuda(), w2.cuda())
    guard = ops.Planes16Guard("cuda", B)
    buf = torch.full((B * H * W + 2, C), NAN, device="cuda")
    d = L.SegmifMixFfn()
    d.x, d.out, d.wimg = xc.data_ptr(), buf.data_ptr(), wimg.data_ptr()
    d.ln_gamma, d.ln_beta, d.ln_eps, d.b2 = gm.data_ptr(), bt.data_ptr(), eps, b2d.data_ptr()
    d.B, d.H, d.W, d.C = B, H, W, C
    d.amax_a, n1 = guard.slot(B)
    d.amax_g, _n2 = guard.slot(B)
    d.amax_images = n1
    assert lib.segmif_mixffn_f16x3(ctypes.byref(d), ops._stream()) == 0
    got = buf.cpu()
    assert torch.equal(xc, keep) and bool(torch.isnan(got[B * H * W:]).all())
    xn = ops.layernorm(xc, gm, bt, eps)
    hh = ops.dwconv3x3_gelu(ops.linear(xn, ops.pack_weight(w1.cuda()), hid, bias=b1.cuda()), dw9, bd.cuda(), H, W)
    chain = ops.linear(hh, ops.pack_weight(w2.cuda()), C, bias=b2d, res=xc)
    e, e32 = err(got[:B * H * W], ref), err(chain.view(B * H * W, C), ref)
    print(f"mixffn C{C} {H}x{W}: e {e:.3e} e32 {e32:.3e}")
    note("mixffn", e)
    assert e < t4.TOL and e <= 3.0 * e32 + 2e-7 and guard.ok(), (e, e32)


# ------------------------------------------------------------------------------------------------------------------- attention
def attention_case(N, Nk, hd):
    C = hd
    q, kv, do = rnd(1, N, C, seed=26 + N, lo=-2, hi=2), rnd(1, Nk, 2 * C, seed=27 + Nk, lo=-2, hi=2), rnd(1, N, C, seed=53)
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    ref = torch.softmax(qd @ kvd[..., :C].transpose(-1, -2) * hd ** -0.5, dim=-1) @ kvd[..., C:]
    ref.backward(do.double())
    return q, kv, do, ref.detach().view(N, C), qd.grad.view(N, C), kvd.grad.view(Nk, 2 * C)


@pytest.mark.parametrize("Nk", [1, 2, 31, 33])
@pytest.mark.parametrize("N", [1, 31, 33])
def test_attention_with_fewer_queries_and_keys_than_a_tile(env, N, Nk):
    """One head, one image, N = 1, 31, 33 queries and Nk = 1, 2, 31, 33 keys (tiles of 32): the fp32 kernel at head_dim 32 and 64,
    the bf16x6 and f16x3 kernels, the f16x3 kernel's PAIRS output (decoded) and the fused backward.  Bars: TOL of max |ref|
    (tests/test_gpu_kernels.py::test_sr_attention) and 2e-5 of each gradient's range for dq / dkv
    (tests/test_gpu_round5.py::test_fused_attention_backward_vs_fp64_autograd).  q, kv and out are pitched; dq / dkv take no pitch."""
    lib, ops, L = env
    st = ops._stream()
    for hd in (32, 64):
        C, scale = hd, hd ** -0.5
        q, kv, do, ref, dq_ref, dkv_ref = attention_case(N, Nk, hd)
        assert float(ref.abs().max()) > 0.0
        qb, kb = pitched(q.view(N, C), 4)[0], pitched(kv.view(Nk, 2 * C), 4)[0]
        kptr = kb.data_ptr()
        buf = nan_out(N, C)
        rc = lib.segmif_sr_attention_f32(qb.data_ptr(), kptr, kptr + 4 * C, buf.data_ptr(), 1, 1, N, Nk, hd, qb.stride(0), kb.stride(0), buf.stride(0), scale, st)
        assert rc == 0
        got = buf.cpu()
        e = err(got[:N, :C], ref)
        print(f"sr_attention fp32 hd{hd} N{N} Nk{Nk}: {e:.3e}")
        note("attention_fp32", e)
        assert only_result_written(got, N, C) and e < TOL, e
        if hd != 64:
            continue
        y32 = buf[:N, :C].contiguous()
        ws = torch.empty((lib.segmif_sr_attention_split_workspace(1, 1, Nk),), device="cuda", dtype=torch.uint8)
        for name in ("bf16x6", "f16x3", "f16x3_pairs"):
            buf = nan_out(N, C)
            args = (qb.data_ptr(), kptr, kptr + 4 * C, buf.data_ptr(), ws.data_ptr(), 1, 1, N, Nk, 64, qb.stride(0), kb.stride(0), buf.stride(0), scale)
            if name == "bf16x6":
                rc = lib.segmif_sr_attention_split_f32(*args, st)
            elif name == "f16x3":
                rc = lib.segmif_sr_attention_split16_f32(*args, None, 1, st)
            else:
                rc = lib.segmif_sr_attention_split16_pairs_f32(*args, None, None, 1, st)
            assert rc == 0
            raw = buf.cpu()
            assert bool(torch.isnan(raw[N:]).all()) and bool(torch.isnan(raw[:N, C:]).all())
            if name == "f16x3_pairs":
                dec = torch.empty((N, C), device="cuda")
                assert lib.segmif_pairs_to_f32(buf.data_ptr(), 4 * buf.stride(0), dec.data_ptr(), C, N, C, st) == 0
                y = dec.cpu()
            else:
                y = raw[:N, :C]
            e = err(y, ref)
            print(f"sr_attention {name} N{N} Nk{Nk}: {e:.3e}")
            note("attention_" + name, e)
            assert e < TOL, (name, e)
        dod = do.cuda().view(N, C).contiguous()
        qd_, kvd_ = q.cuda().view(N, C).contiguous(), kv.cuda().view(Nk, 2 * C).contiguous()
        dq = torch.full((N + 2, C), NAN, device="cuda")
        dkv = torch.full((Nk + 2, 2 * C), NAN, device="cuda")
        wsf = torch.empty((lib.segmif_sr_attention_bwd_workspace_floats(1, 1, N, Nk, C),), device="cuda")
        rc = lib.segmif_sr_attention_bwd_f32(qd_.data_ptr(), kvd_.data_ptr(), kvd_.data_ptr() + 4 * C, y32.data_ptr(), dod.data_ptr(), dq.data_ptr(),
                                             dkv.data_ptr(), wsf.data_ptr(), 1, 1, N, Nk, 64, 2 * C, scale, st)
        assert rc == 0
        gq, gkv = dq.cpu(), dkv.cpu()
        if Nk == 1:
            # one key: softmax = 1 and dq = 0 EXACTLY in the reference, so there is no range to be relative to.  The kernel forms
            # dq = scale (P o (dP - D)) K with dP = dO V^T and D = dO . O from differently ordered sums: the bar is the same 2e-5
            # of the expression's conditioning scale (|dO| |V|^T) |K| instead
            assert float(dq_ref.abs().max()) == 0.0
            yard = scale * float(((do.double().view(N, C).abs() @ kv.double().view(Nk, 2 * C)[:, C:].abs().t()) @ kv.double().view(Nk, 2 * C)[:, :C].abs()).max())
            e1 = float(gq[:N].double().abs().max()) / yard
        else:
            e1 = err(gq[:N], dq_ref)
        e2 = err(gkv[:Nk], dkv_ref)
        print(f"sr_attention_bwd N{N} Nk{Nk}: dq {e1:.3e} dkv {e2:.3e}")
        note("attention_bwd", max(e1, e2))
        assert bool(torch.isnan(gq[N:]).all()) and bool(torch.isnan(gkv[Nk:]).all()) and e1 < 2e-5 and e2 < 2e-5, (e1, e2)


# ------------------------------------------------------------------------------------------------------------ weight gradients
def wgrad_call(lib, ops, L, d, dy, ldy, N, K_elems, want_bias=True):
    """segmif_wgrad_f32 into NaN buffers eight elements longer than dW and db (neither takes a pitch here) -> (dW buffer, db buffer)"""
    dw = torch.full((N * K_elems + 8,), NAN, device="cuda")
    db = torch.full((N + 8,), NAN, device="cuda")
    ws = torch.empty((lib.segmif_wgrad_workspace_size(d.M, d.N, d.K),), device="cuda")
    rc = lib.segmif_wgrad_f32(ctypes.byref(d), dy.data_ptr(), ldy, 0, dw.data_ptr(), K_elems, 1, db.data_ptr() if want_bias else None, ws.data_ptr(), 0,
                              ops._stream())
    assert rc == 0
    return dw.cpu(), db.cpu()


@pytest.mark.parametrize("M", [1, 33])
def test_dense_weight_gradient_and_column_sums_on_one_row(env, M):
    """dW = dY^T X with M = 1 and 33 rows (a chunk holds at least 1024) on the fast (N, K multiples of the tile) and the general path,
    pitched X and dY; and segmif_colsum_f32 over ONE row on its vector and scalar kernels.  Bar: 5e-5 of max |ref|
    (tests/test_gpu_backward.py::test_linear_backward, tests/test_gpu_autograd_nodes.py::test_colsum)."""
    lib, ops, L = env
    for N, K in ((64, 64), (12, 20)):
        x, dy = rnd(M, K, seed=1), rnd(M, N, seed=4)
        ref, bref = dy.double().t() @ x.double(), dy.double().sum(0)
        xb, yb = pitched(x, 4)[0], pitched(dy, 4)[0]
        d = L.SegmifIgemm()
        d.in_ = xb.data_ptr()
        d.M, d.N, d.K, d.lda, d.Cin = M, N, K, xb.stride(0), K
        d.H = d.W = d.OH = d.OW = d.KH = d.KW = d.stride = d.dil = 1
        dw, db = wgrad_call(lib, ops, L, d, yb, yb.stride(0), N, K)
        e, eb = err(dw[:N * K].view(N, K), ref), err(db[:N], bref)
        print(f"wgrad dense M{M} N{N} K{K}: dW {e:.3e} db {eb:.3e}")
        note("wgrad_dense", max(e, eb))
        assert bool(torch.isnan(dw[N * K:]).all()) and bool(torch.isnan(db[N:]).all()) and e < BWD_TOL and eb < BWD_TOL, (e, eb)
    if M == 1:
        for N, extra in ((64, 4), (9, 3), (1280, 0)):
            x = rnd(1, N, seed=80, lo=-3, hi=5)
            xb = pitched(x, extra)[0] if extra else x.cuda()
            out = torch.full((N + 8,), NAN, device="cuda")
            ws = torch.empty((lib.segmif_colsum_blocks(1) * N,), device="cuda", dtype=torch.float64)
            assert lib.segmif_colsum_f32(xb.data_ptr(), out.data_ptr(), ws.data_ptr(), 1, N, xb.stride(0), 0, ops._stream()) == 0
            got = out.cpu()
            e = err(got[:N], x.double().view(N))
            print(f"colsum one row N{N}: {e:.3e}")
            note("colsum_one_row", e)
            assert bool(torch.isnan(got[N:]).all()) and e < BWD_TOL, e


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
def test_conv3x3_weight_gradient_on_images_smaller_than_one_tile(env, H, W, dil):
    """The 3 x 3 stride-1 weight gradient works on 8 x 32 (halo, exact fp32: N = 16) and 4 x 32 (two-team split kernel, bf16x6 and
    f16x3: N = 32) pixel tiles: a 1 x 1 and a 3 x 5 image.  Bars: 5e-5 for the fp32 kernel (tests/test_gpu_backward.py), 2e-6 of
    max |ref| for both split arithmetics and 1e-5 for the fused bias gradient
    (tests/test_gpu_round4.py::test_conv_wgrad_on_f16x3_with_device_ranges)."""
    lib, ops, L = env
    B, Cin = 2, 32
    for N, form in ((16, "halo_fp32"), (32, "split_bf16x6"), (32, "split_f16x3")):
        x, dy = rnd(B, H, W, Cin, seed=1), rnd(B, H, W, N, seed=2)
        ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (N, Cin, 3, 3), dy.double().permute(0, 3, 1, 2), padding=dil, dilation=dil)
        bref = dy.double().sum((0, 1, 2))
        assert float(ref.abs().max()) > 0.0
        xd, yd = x.cuda().view(B * H * W, Cin).contiguous(), dy.cuda().view(B * H * W, N).contiguous()
        d = L.SegmifIgemm()
        d.in_ = xd.data_ptr()
        d.M, d.N, d.K, d.lda = B * H * W, N, 9 * Cin, Cin
        d.H, d.W, d.Cin, d.KH, d.KW, d.stride, d.pad, d.dil, d.OH, d.OW = H, W, Cin, 3, 3, 1, dil, dil, H, W
        if form == "split_f16x3":
            xs, ys = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.amax_rows(xd, xs)
            ops.amax_rows(yd, ys)
            d.split_f16, d.split_in_amax, d.split_in_amax_n, d.wgrad_dy_amax, d.wgrad_dy_amax_n = 1, xs.data_ptr(), 1, ys.data_ptr(), 1
        dw, db = wgrad_call(lib, ops, L, d, yd, N, N, 9 * Cin)
        e, eb = err(dw[:N * 9 * Cin].view(N, Cin, 3, 3), ref), err(db[:N], bref)
        print(f"wgrad3x3 {form} {H}x{W} dil{dil}: dW {e:.3e} db {eb:.3e}")
        note("wgrad3x3_" + form, e)
        assert bool(torch.isnan(dw[N * 9 * Cin:]).all()) and bool(torch.isnan(db[N:]).all()), form
        assert (e < BWD_TOL and eb < BWD_TOL) if form == "halo_fp32" else (e < 2e-6 and eb < 1e-5), (form, e, eb)


# ------------------------------------------------------------------------------------------------------------------- CrossPath
from test_gpu_kernels import _gram_from_partials  # noqa: E402


def rows3(buf, B, N, C):
    """the (B, N, C) rows view at the start of a pitched 2-D buffer"""
    ld = buf.stride(0)
    return torch.as_strided(buf, (B, N, C), (N * ld, ld, 1))


@pytest.mark.parametrize("N", [1, 31, 33, 255])
def test_crosspath_gram_sum_and_fold_on_less_than_a_workgroup_of_pixels(env, N):
    """The Gram kernel sums inside 32-pixel runs: N = 1, 31, 33 and 255 pixels (one partial per image), then gram_sum and fold on
    that single partial (nblk = 1).  Bars: 1e-6 of max |G| and TOL for the folded weight (tests/test_gpu_kernels.py::
    test_crosspath_gram_and_fold); the fp64 outputs take no pitch (longer buffers only)."""
    lib, ops, L = env
    B, st, scale = 2, ops._stream(), 8 ** -0.5
    x, w, b = rnd(B, N, 64, seed=61), rnd(64, 64, seed=62) * 0.3, rnd(64, seed=63) * 0.1
    wkv, wend = rnd(128, 64, seed=64) * 0.05, rnd(64, 128, seed=65)
    y = F.relu(x.double() @ w.double().t() + b.double())
    Gref = torch.einsum("bni,bnj->bij", y, y)
    assert float(Gref.abs().max()) > 0.0
    xb = pitched(x.view(B * N, 64), 4)[0]
    wd, bd = w.cuda(), b.cuda()
    nblk = lib.segmif_crosspath_gram_blocks(N)
    assert nblk == 1
    part = f64_nan(B * 3072 + 8)
    assert lib.segmif_crosspath_gram_f32(xb.data_ptr(), xb.stride(0), wd.data_ptr(), bd.data_ptr(), part.data_ptr(), B, N, st) == 0
    got = part.cpu()
    e = float((_gram_from_partials(got[:B * 3072].view(B, 1, 3072)) - Gref).abs().max() / Gref.abs().max())
    print(f"crosspath_gram N{N}: {e:.3e}")
    note("crosspath_gram", e)
    assert bool(torch.isnan(got[B * 3072:]).all()) and e < 1e-6, e
    total = f64_nan(B * 3072 + 8)
    assert lib.segmif_crosspath_gram_sum_f64(part.data_ptr(), 1, total.data_ptr(), B, st) == 0
    tot = total.cpu()
    assert torch.equal(tot[:B * 3072], got[:B * 3072]) and bool(torch.isnan(tot[B * 3072:]).all())  # the sum of one partial is that partial
    kd, ed = wkv.cuda(), wend.cuda()
    buf = torch.full((B * 64 + 2, 128 + 8), NAN, device="cuda")
    rc = lib.segmif_crosspath_fold_f32(total.data_ptr(), 1, kd.data_ptr(), ed.data_ptr(), buf.data_ptr(), B, 64, 128, 64, buf.stride(0), 64, scale, None, st)
    assert rc == 0
    kv = y @ wkv.double().t()
    k, v = kv[..., :64].view(B, N, 8, 8), kv[..., 64:].view(B, N, 8, 8)
    ctx = torch.softmax(torch.einsum("bnhi,bnhj->bhij", k, v) * scale, dim=-2)
    ref = torch.einsum("bhij,nhj->bnhi", ctx, wend.double()[:, 64:].view(64, 8, 8)).reshape(B * 64, 64)
    gw = buf.cpu()
    e = err(gw[:B * 64, 64:128], ref)
    print(f"crosspath_fold nblk 1, N{N}: {e:.3e}")
    note("crosspath_fold", e)
    outside = gw.clone()
    outside[:B * 64, 64:128] = NAN
    assert bool(torch.isnan(outside).all()) and e < TOL, e


def test_crosspath_lazy_gram_and_tails_at_their_smallest_geometry(env):
    """gram_lazy at its smallest legal geometry (a 1 x 1 source enlarged to 1 x 4: W % 4 == 0, 3 iw <= W), the tail on ONE token, and the
    lazy tail with that 1 x 1 source plus the f16x3 planes copy.  Bars: 2e-6 of max |G| (tests/test_gpu_round5.py), TOL against fp64 for
    the tails (tests/test_gpu_kernels.py::test_crosspath_tail), the planes copy byte for byte planes16_from_f32 of the fp32 output
    (tests/test_gpu_planes16.py::test_crosspath_tail_f16x3_planes_copy)."""
    lib, ops, L = env
    import test_gpu_planes16  # noqa: F401  (the bar's home)
    B, st = 2, ops._stream()
    low = rnd(B, 1, 1, 64, seed=3, lo=-2.0, hi=2.0)   # the projected low-resolution map: a resize of one pixel repeats it
    lb = pitched(low.view(B, 64), 4)[0]
    part = f64_nan(B * 3072 + 8)
    assert lib.segmif_crosspath_gram_blocks(4) == 1
    assert lib.segmif_crosspath_gram_lazy_f32(lb.data_ptr(), lb.stride(0), 1, 1, 1, 4, part.data_ptr(), B, st) == 0
    up = low.double().view(B, 1, 64).relu().expand(B, 4, 64)
    g64 = torch.einsum("bni,bnj->bij", up, up)
    got = part.cpu()
    e = float((_gram_from_partials(got[:B * 3072].view(B, 1, 3072)) - g64).abs().max() / g64.abs().max())
    print(f"crosspath_gram_lazy 1x1 -> 1x4: {e:.3e}")
    note("crosspath_gram_lazy", e)
    assert bool(torch.isnan(got[B * 3072:]).all()) and e < 2e-6, e

    w3, b3, wi, bi = rnd(64, 64, seed=73) * 0.3, rnd(64, seed=74) * 0.1, rnd(64, 64, seed=75) * 0.3, rnd(64, seed=76) * 0.1
    weff, bend = rnd(B, 64, 128, seed=77) * 0.2, rnd(64, seed=78) * 0.1
    gm, bt = rnd(64, seed=79, lo=0.5, hi=1.5), rnd(64, seed=80)
    ln = (gm.cuda(), bt.cuda(), 1e-5)

    def tail_ref(y3, xi):
        t = torch.cat((y3, F.relu(xi.double() @ wi.double().t() + bi.double())), dim=-1)
        return F.layer_norm(xi.double() + torch.einsum("bnk,bok->bno", t, weff.double()) + bend.double(), (64,), gm.double(), bt.double(), 1e-5)

    # one token per image
    x3, xi = rnd(B, 1, 64, seed=71), rnd(B, 1, 64, seed=72)
    ref = tail_ref(F.relu(x3.double() @ w3.double().t() + b3.double()), xi).reshape(B, 64)
    buf = nan_out(B, 64)
    ops.crosspath_tail(rows3(pitched(x3.view(B, 64), 4)[0], B, 1, 64), rows3(pitched(xi.view(B, 64), 8)[0], B, 1, 64), w3.cuda(), b3.cuda(), wi.cuda(),
                       bi.cuda(), weff.cuda(), bend.cuda(), ln, out=rows3(buf, B, 1, 64))
    got = buf.cpu()
    e = err(got[:B, :64], ref)
    print(f"crosspath_tail N1: {e:.3e}")
    note("crosspath_tail", e)
    assert only_result_written(got, B, 64) and e < TOL, e
    # the lazy tail: x3 = the 1 x 1 projected map, tokens 1 x 4, fp32 rows and the f16x3 planes copy
    N = 4
    xi = rnd(B, N, 64, seed=9, lo=-1.5, hi=1.5)
    ref = tail_ref(low.double().view(B, 1, 64).relu().expand(B, N, 64), xi).reshape(B * N, 64)
    guard = ops.Planes16Guard("cuda", B)
    pl = ops.Planes(B, 1, 4, 4, "cuda", guard)
    pl.data.zero_()
    buf = nan_out(B * N, 64)
    x3l = torch.as_strided(lb, (B, 1, 1, 64), (lb.stride(0), lb.stride(0), lb.stride(0), 1))
    ops.crosspath_tail(x3l, rows3(pitched(xi.view(B * N, 64), 4)[0], B, N, 64), None, None, wi.cuda(), bi.cuda(), weff.cuda(), bend.cuda(), ln,
                       out=rows3(buf, B, N, 64), planes=pl, hw=(1, 4), lazy=True)
    got = buf.cpu()
    e = err(got[:B * N, :64], ref)
    print(f"crosspath_tail lazy 1x1 -> 1x4 with planes: {e:.3e}")
    note("crosspath_tail_lazy", e)
    assert only_result_written(got, B * N, 64) and e < TOL, e
    want = ops.Planes(B, 1, 4, 4, "cuda", ops.Planes16Guard("cuda", B))
    want.data.zero_()
    want.load_f32(buf[:B * N, :64].contiguous().view(B, 1, 4, 64), chunk0=0)
    assert torch.equal(pl.data, want.data)
