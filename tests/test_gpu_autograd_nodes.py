"""Every torch.autograd.Function node of segmif_amd/autograd.py ALONE against float64 aten on the CPU, at the shapes where its
kernels change path: ragged tails, pitched operands, placed outputs (ag.Out), sliced cotangents and the dispatch branches no
network takes (tests/test_gpu_backward.py holds the network-sized cases of the same nodes).

Bars: TOL = 5e-5 on max|got - ref| / max|ref| (the fp32-kernel-against-float64 bar of test_gpu_backward.py), 1e-6 for the SiLU
nodes (the bar of test_gpu_variant_train.py::test_pointwise2_bwd_vs_fp64); no case needs more.
Placed outputs and sliced gradients live in NaN-filled buffers that must stay NaN outside the view.
The worst error of every test is recorded under the names nodes_* through tests/_observed.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import segmif_oracle as so
from _observed import observed
from test_gpu_backward import TOL, err, leaf, rnd

pytestmark = pytest.mark.gpu

SILU_TOL = 1e-6
NAN = float("nan")


@pytest.fixture(scope="module")
def ag():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import autograd as _ag
    return _ag


class Track:
    """err() of every compared tensor of one test: printed and recorded (the running worst) BEFORE it is asserted."""

    def __init__(self, name):
        self.name, self.worst = name, 0.0

    def __call__(self, what, got, ref, tol=TOL):
        e = err(got, ref)
        self.worst = max(self.worst, e)
        observed(self.name, self.worst)
        print(f"{self.name} {what}: {e:.3e}")
        assert e < tol, (self.name, what, e, tol)
        return e


def nan_buf(*shape):
    return torch.full(shape, NAN, device="cuda")


def only_view_written(buf, c0, c1):
    """The channel slice [c0, c1) of a NaN-filled buffer is finite, everything else still NaN."""
    return bool(torch.isfinite(buf[..., c0:c1]).all()) and bool(torch.isnan(buf[..., :c0]).all()) \
        and bool(torch.isnan(buf[..., c1:]).all())


def sliced_cotangent(y, G, before):
    """Back-propagate G (..., before + C) through cat([pad, y]): autograd hands y's node the channel slice G[..., before:], a
    view with pitch before + C > C (no copy is made on the way)."""
    pad = torch.zeros(y.shape[:-1] + (before,), device=y.device)
    torch.cat([pad, y], dim=-1).backward(G)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. conv input gradient: every dispatch branch of ConvFn.backward
# ------------------------------------------------------------------------------------------------------------------------------
CONV_STRIDED_DILATED = [  # the last `else`: segmif_conv_dgrad_strided_dil_f32
    (2, 13, 17, 8, 16, 3, 2, 2, 2, 0),
    (1, 11, 14, 5, 7, 3, 2, 2, 2, 1),
    (1, 15, 15, 8, 8, 3, 3, 2, 2, 0),
]
CONV_COL2IM = [  # overlapping / general strided at dilation 1: GEMM + col2im
    (2, 10, 13, 16, 24, 1, 2, 0, 1, 0),  # k = 1
    (1, 11, 16, 8, 16, 2, 3, 0, 1, 0),   # stride > k: input pixels without a tap, gradient exactly 0
    (1, 12, 9, 6, 16, 3, 2, 0, 1, 0),    # Cin % 4 != 0: col2im_kernel<1>
    (1, 9, 9, 4, 8, 5, 2, 2, 1, 0),
]
CONV_PATCHES = [  # stride == k, pad 0: one dense GEMM + patch -> image gather
    (1, 9, 13, 32, 24, 2, 2, 0, 1, 0),   # N % 16 != 0: the pack_weight form of wt
    (2, 8, 8, 4, 16, 4, 4, 0, 1, 0),
]
CONV_STRIDE1 = [  # stride 1 but not "same": full correlation with the rotated kernel at pad' = dil (k - 1) - pad
    (1, 9, 12, 16, 16, 3, 1, 0, 1, 0),   # valid conv
    (1, 9, 12, 16, 8, 1, 1, 0, 1, 1),    # 1x1: a dense problem to the weight-gradient kernel, written at the (N, Cin) pitch
    (1, 10, 11, 8, 16, 2, 1, 0, 1, 0),   # even kernel
    (1, 12, 12, 16, 16, 3, 1, 1, 2, 0),  # pad < dil
]
CONV_NEGATIVE_PAD = (1, 9, 12, 16, 8, 1, 1, 1, 1, 0)  # pad > dil (k - 1): the transposed conv's padding is -1
CONV_ALL = CONV_STRIDED_DILATED + CONV_COL2IM + CONV_PATCHES + CONV_STRIDE1
CONV_ONE_PER_BRANCH = [CONV_STRIDED_DILATED[0], CONV_COL2IM[2], CONV_PATCHES[0], CONV_STRIDE1[0]]


@functools.lru_cache(maxsize=None)
def conv_reference(case):
    """fp32 inputs and the float64 results of F.conv2d (+ ReLU): computed once per case, shared, never modified."""
    B, H, W, Cin, N, k, s, p, d, act = case
    x, w, b = rnd(B, Cin, H, W, seed=5), rnd(N, Cin, k, k, seed=6), rnd(N, seed=7)
    xr, wr, br = leaf(x, double=True), leaf(w, double=True), leaf(b, double=True)
    y = F.conv2d(xr, wr, br, stride=s, padding=p, dilation=d)
    y = F.relu(y) if act == 1 else y
    g = rnd(*y.shape, seed=8)
    y.backward(g.double())
    return dict(x=x, w=w, b=b, g=g, y=y.detach().permute(0, 2, 3, 1), dx=xr.grad.permute(0, 2, 3, 1), dw=wr.grad, db=br.grad)


def run_conv(ag, case, want=(True, True, True)):
    """ag.conv2d forward + backward with gradients wanted for (x, w, b) as flagged -> (y, x, w, b) device tensors."""
    B, H, W, Cin, N, k, s, p, d, act = case
    r = conv_reference(case)
    dev = [r["x"].permute(0, 2, 3, 1).contiguous().cuda(), r["w"].cuda(), r["b"].cuda()]
    xg, wg, bg = [t.requires_grad_(True) if f else t for t, f in zip(dev, want)]
    yg = ag.conv2d(xg, wg, bg, k=k, stride=s, pad=p, dil=d, act=act)
    yg.backward(r["g"].permute(0, 2, 3, 1).contiguous().cuda())
    return yg, xg, wg, bg


@pytest.mark.parametrize("case", CONV_ALL)
def test_conv_every_dgrad_branch(ag, case):
    """Two defects this test found, both fixed in the commit that added it.  Strided + dilated: the gather kernel had no dilation
    argument - err(dx) 1.31 / 1.00 / 1.48 on the three cases, y / dw / db within TOL.  The 1x1 stride-1 case: the weight-gradient
    kernel treats it as a dense problem and was handed a row pitch of 0 for dw - err(dw) 0.97, y / dx / db within TOL."""
    r = conv_reference(case)
    t = Track(f"nodes_conv[{'-'.join(map(str, case))}]")
    yg, xg, wg, bg = run_conv(ag, case)
    t("y", yg, r["y"])
    t("dx", xg.grad, r["dx"])
    t("dw", wg.grad, r["dw"])
    t("db", bg.grad, r["db"])
    # input pixels no tap reaches (stride > k, rows / columns the conv dropped) have a gradient of exactly zero
    assert bool((xg.grad.cpu()[r["dx"] == 0] == 0).all())


def test_conv_stride1_padding_beyond_the_kernel(ag):
    """k = 1, pad = 1: the input gradient is the rotated conv at padding dil (k - 1) - pad = -1, which the implicit-GEMM gather
    takes as it is (every tap is bounds-checked) - so the gradient has to be right, not refused."""
    case = CONV_NEGATIVE_PAD
    r = conv_reference(case)
    t = Track("nodes_conv_negative_pad")
    yg, xg, wg, bg = run_conv(ag, case)
    t("y", yg, r["y"])
    t("dx", xg.grad, r["dx"])
    t("dw", wg.grad, r["dw"])
    t("db", bg.grad, r["db"])


@pytest.mark.parametrize("only", ["x", "w", "b"])
@pytest.mark.parametrize("case", CONV_ONE_PER_BRANCH)
def test_conv_one_gradient_wanted(ag, case, only):
    """only b: the bias gradient is colsum(dz), no weight-gradient launch to fuse it into."""
    r = conv_reference(case)
    t = Track(f"nodes_conv_only[{only}-{'-'.join(map(str, case))}]")
    _, xg, wg, bg = run_conv(ag, case, want=(only == "x", only == "w", only == "b"))
    got = dict(x=xg, w=wg, b=bg)
    for name, ten in got.items():
        if name == only:
            t("d" + name, ten.grad, r["d" + name])
        else:
            assert ten.grad is None, name


# ------------------------------------------------------------------------------------------------------------------------------
# 2. ag.dwconv (DwconvFn): dwconv_gelu_bwd_kernel<false> + dwconv3x3_plain_kernel with flipped taps
# ------------------------------------------------------------------------------------------------------------------------------
def dwconv_reference(h, w, b, g, H, W, wgrad=True):
    B, _, C = h.shape
    hr = leaf(h, double=True)
    wr, br = (leaf(w, double=True), leaf(b, double=True)) if wgrad else (w.double(), b.double())
    y = F.conv2d(hr.transpose(1, 2).reshape(B, C, H, W), wr, br, padding=1, groups=C).flatten(2).transpose(1, 2)
    y.backward(g.double())
    return y.detach(), hr.grad, (wr.grad if wgrad else None), (br.grad if wgrad else None)


def dwconv_inputs(B, H, W, C):
    return (rnd(B, H * W, C, seed=13, lo=-2, hi=2), rnd(C, 1, 3, 3, seed=14), rnd(C, seed=15), rnd(B, H * W, C, seed=16))


@pytest.mark.parametrize("B,H,W,C", [(2, 9, 13, 128),
                                     (1, 5, 3, 256),    # W < 8 and H < 8
                                     (1, 1, 1, 128),
                                     (2, 17, 8, 384),   # three channel tiles, exactly one x tile, two strips plus one row
                                     (1, 8, 9, 640)])
def test_dwconv_node(ag, B, H, W, C):
    h, w, b, g = dwconv_inputs(B, H, W, C)
    y, dh, dw, db = dwconv_reference(h, w, b, g, H, W)
    t = Track(f"nodes_dwconv[{B}-{H}-{W}-{C}]")
    hg, wg, bg = leaf(h, "cuda"), leaf(w, "cuda"), leaf(b, "cuda")
    yg = ag.dwconv(hg, wg, bg, H, W)
    t("y", yg, y)
    yg.backward(g.cuda())
    t("dh", hg.grad, dh)
    t("dw", wg.grad, dw)
    t("db", bg.grad, db)


def test_dwconv_input_gradient_only_at_36_channels(ag):
    """Frozen weights: only dwconv3x3_plain_kernel runs, which takes any C % 4 == 0."""
    B, H, W, C = 2, 9, 13, 36
    h, w, b, g = dwconv_inputs(B, H, W, C)
    y, dh, _, _ = dwconv_reference(h, w, b, g, H, W, wgrad=False)
    t = Track("nodes_dwconv_frozen[36]")
    hg = leaf(h, "cuda")
    yg = ag.dwconv(hg, w.cuda(), b.cuda(), H, W)
    t("y", yg, y)
    yg.backward(g.cuda())
    t("dh", hg.grad, dh)


def test_dwconv_refuses_parameter_gradients_at_36_channels(ag):
    B, H, W, C = 2, 9, 13, 36
    h, w, b, _ = dwconv_inputs(B, H, W, C)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ag.dwconv(leaf(h, "cuda"), leaf(w, "cuda"), leaf(b, "cuda"), H, W)


def test_dwconv_parameter_gradients_are_deterministic(ag):
    B, H, W, C = 2, 17, 8, 384
    h, w, b, g = dwconv_inputs(B, H, W, C)
    runs = []
    for _ in range(2):
        hg, wg, bg = leaf(h, "cuda"), leaf(w, "cuda"), leaf(b, "cuda")
        ag.dwconv(hg, wg, bg, H, W).backward(g.cuda())
        runs.append((wg.grad.clone(), bg.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------------------------------------
# 3. per-image linear nodes
# ------------------------------------------------------------------------------------------------------------------------------
def batched_linear_reference(x, w, b, g):
    xr, wr = leaf(x, double=True), leaf(w, double=True)
    br = leaf(b, double=True) if b is not None else None
    y = torch.bmm(xr, wr.transpose(1, 2))
    y = y + br if br is not None else y
    y.backward(g.double())
    return y.detach(), xr.grad, wr.grad, (br.grad if br is not None else None)


def batched_linear_inputs(B, n, K, N):
    return rnd(B, n, K, seed=70), rnd(B, N, K, seed=71), rnd(N, seed=72), rnd(B, n, N, seed=73)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,n,K,N", [(2, 37, 64, 64),
                                     (3, 130, 128, 9),  # N % 16 != 0: the transposed per-image weights are padded
                                     (1, 5, 16, 1)])
def test_batched_linear(ag, B, n, K, N, bias):
    x, w, b, g = batched_linear_inputs(B, n, K, N)
    b = b if bias else None
    y, dx, dw, db = batched_linear_reference(x, w, b, g)
    t = Track(f"nodes_batched_linear[{B}-{n}-{K}-{N}-{'bias' if bias else 'nobias'}]")
    xg, wg = leaf(x, "cuda"), leaf(w, "cuda")
    bg = leaf(b, "cuda") if bias else None
    yg = ag.batched_linear(xg, wg, bg)
    t("y", yg, y)
    yg.backward(g.cuda())
    t("dx", xg.grad, dx)
    t("dw", wg.grad, dw)
    if bias:
        t("db", bg.grad, db)


def test_batched_linear_pitched_input(ag):
    """x = a channel slice of a wider tensor: the forward GEMM and the weight gradient read it at its pitch (lda = x.stride(1))."""
    B, n, K, N = 3, 130, 128, 9
    x, w, b, g = batched_linear_inputs(B, n, K, N)
    y, dx, dw, db = batched_linear_reference(x, w, b, g)
    t = Track("nodes_batched_linear_pitched")
    wide = rnd(B, n, K + 16, seed=74)
    wide[..., 8:8 + K] = x
    wideg, wg, bg = leaf(wide, "cuda"), leaf(w, "cuda"), leaf(b, "cuda")
    yg = ag.batched_linear(wideg[..., 8:8 + K], wg, bg)
    t("y", yg, y)
    yg.backward(g.cuda())
    t("dx", wideg.grad[..., 8:8 + K], dx)
    assert float(wideg.grad[..., :8].abs().max()) == 0.0 and float(wideg.grad[..., 8 + K:].abs().max()) == 0.0
    t("dw", wg.grad, dw)
    t("db", bg.grad, db)


def test_batched_linear_bias_gradient_only(ag):
    """Frozen weights and input: db = colsum(dy) (no weight-gradient launch to fuse it into)."""
    B, n, K, N = 2, 37, 64, 64
    x, w, b, g = batched_linear_inputs(B, n, K, N)
    y, _, _, db = batched_linear_reference(x, w, b, g)
    t = Track("nodes_batched_linear_bias_only")
    bg = leaf(b, "cuda")
    yg = ag.batched_linear(x.cuda(), w.cuda(), bg)
    t("y", yg, y)
    yg.backward(g.cuda())
    t("db", bg.grad, db)


def batched_linear2_run(ag, Ka, Kb, N, n, B=2):
    """xa | xb = two channel slices of ONE wider buffer; res requires grad.  -> (Track, reference tuple, device tensors)"""
    K = Ka + Kb
    wide = rnd(B, n, K + 8, seed=75)
    w, b, res, g = rnd(B, N, K, seed=76), rnd(N, seed=77), rnd(B, n, N, seed=78), rnd(B, n, N, seed=79)
    xr, wr, br, rr = leaf(wide[..., 4:4 + K], double=True), leaf(w, double=True), leaf(b, double=True), leaf(res, double=True)
    y = rr + torch.bmm(xr, wr.transpose(1, 2)) + br
    y.backward(g.double())
    wideg, wg, bg, rg = leaf(wide, "cuda"), leaf(w, "cuda"), leaf(b, "cuda"), leaf(res, "cuda")
    gd = g.cuda()
    yg = ag.batched_linear2(wideg[..., 4:4 + Ka], wideg[..., 4 + Ka:4 + K], wg, bg, rg)
    return (y.detach(), xr.grad, wr.grad, br.grad), (yg, wideg, wg, bg, rg, gd)


@pytest.mark.parametrize("n", [37, 407])
@pytest.mark.parametrize("Ka,Kb,N", [(64, 64, 64), (32, 96, 48),
                                     (32, 48, 64)])  # in place of (16, 48): the two-source GEMM wants Ka % 32 == 0 (see below)
def test_batched_linear2(ag, Ka, Kb, N, n):
    K = Ka + Kb
    t = Track(f"nodes_batched_linear2[{Ka}-{Kb}-{N}-{n}]")
    (y, dx, dw, db), (yg, wideg, wg, bg, rg, gd) = batched_linear2_run(ag, Ka, Kb, N, n)
    t("y", yg, y)
    yg.backward(gd)
    t("dxa|dxb", wideg.grad[..., 4:4 + K], dx)
    assert float(wideg.grad[..., :4].abs().max()) == 0.0 and float(wideg.grad[..., 4 + K:].abs().max()) == 0.0
    t("dw", wg.grad, dw)  # both column blocks: dw[:, :, Ka:] is written through sn = K
    t("db", bg.grad, db)
    assert torch.equal(rg.grad, gd)  # the residual's gradient IS the cotangent


def test_batched_linear2_refuses_a_first_source_of_16_channels(ag):
    """(Ka, Kb) = (16, 48): the two-source GEMM tiles its first source in 32-column steps and says so instead of computing."""
    B, n, Ka, Kb, N = 2, 37, 16, 48, 64
    wide = rnd(B, n, Ka + Kb + 8, seed=75).cuda()
    with pytest.raises(RuntimeError):
        ag.batched_linear2(wide[..., 4:4 + Ka], wide[..., 4 + Ka:4 + Ka + Kb], rnd(B, N, Ka + Kb, seed=76).cuda(), None,
                           rnd(B, n, N, seed=78).cuda())


# ------------------------------------------------------------------------------------------------------------------------------
# 4. ag.colsum: scalar kernel + the four vector instantiations, pitched views, accumulate, the rows-per-block rule
# ------------------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [
    # rows, N, form        rows per block: 16 up to 8192 rows, 32 at 9000, 144 at 70001
    (1, 1280, "dense"),      # quads 320 > 64 lanes: five trips of the q0 loop
    (15, 260, "dense"),      # 65 quads: two trips, the second with one live lane
    (16, 256, "pitch4"),     # QPR 64, pitched on the vector path
    (17, 128, "accumulate"),  # QPR 32; two blocks, the second with one row
    (1003, 64, "dense"),     # QPR 16
    (1003, 260, "pitch4"),
    (9000, 32, "dense"),     # QPR 8
    (9000, 9, "dense"),      # scalar kernel
    (70001, 1, "dense"),
    (1003, 64, "pitch_odd"),  # N % 4 == 0 but ld % 4 != 0: scalar kernel
    (17, 1280, "accumulate"),
    (16, 1, "pitch_odd"),
    (15, 9, "accumulate"),
]


@pytest.mark.parametrize("rows,N,form", COLSUM_CASES)
def test_colsum(ag, rows, N, form):
    left, right = {"dense": (0, 0), "accumulate": (0, 0), "pitch4": (4, 4), "pitch_odd": (0, 3)}[form]
    wide = rnd(rows, left + N + right, seed=80, lo=-3, hi=5)  # sums that do not hover at zero
    ref = wide[:, left:left + N].double().sum(0)
    x = wide.cuda()[:, left:left + N]
    t = Track(f"nodes_colsum[{rows}-{N}-{form}]")
    if form == "accumulate":
        base = rnd(N, seed=81, lo=-3, hi=5)
        outs = [ag.colsum(x, out=base.clone().cuda(), accumulate=True) for _ in range(2)]
        ref = ref + base.double()
    else:
        outs = [ag.colsum(x) for _ in range(2)]
    t("sum", outs[0], ref)
    assert torch.equal(outs[0], outs[1])  # fixed-order two-stage reduction


# ------------------------------------------------------------------------------------------------------------------------------
# 5. attention backward over materialised scores (row_softmax / row_softmax_bwd / segmif_wgrad_batched2_f32)
# ------------------------------------------------------------------------------------------------------------------------------
def attention_inputs(B, heads, N, Nk, hd, big=False):
    C = heads * hd
    r = 8 if big else 2
    q, k = rnd(B, N, C, seed=19, lo=-r, hi=r), rnd(B, Nk, C, seed=20, lo=-r, hi=r)
    v, g = rnd(B, Nk, C, seed=22, lo=-2, hi=2), rnd(B, N, C, seed=21)
    return q, torch.cat([k, v], dim=2), g


def attention_reference(q, kv, g, heads, hd):
    """The float64 graph of test_sr_attention_backward."""
    B, N, C = q.shape
    Nk = kv.shape[1]
    qr, kvr = leaf(q, double=True), leaf(kv, double=True)
    qh = qr.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    kvh = kvr.reshape(B, Nk, 2, heads, hd)
    k, v = kvh[:, :, 0].permute(0, 2, 1, 3), kvh[:, :, 1].permute(0, 2, 1, 3)
    y = (torch.softmax(qh @ k.transpose(-2, -1) * hd ** -0.5, -1) @ v).transpose(1, 2).reshape(B, N, C)
    y.backward(g.double())
    return y.detach(), qr.grad, kvr.grad


@pytest.mark.parametrize("B,heads,N,Nk,big", [
    (1, 1, 131, 1, False),    # rows not a multiple of the 4 per block; one key: softmax == 1, dq == 0
    (2, 2, 70, 6, False),
    (1, 3, 65, 33, False),    # Nk % 4 != 0: contraction over the padded pitch, rows >= Nk sliced away
    (1, 2, 96, 300, False),
    (1, 1, 64, 1024, False),  # the last register slot (lane + 64 * 15)
    (2, 2, 70, 6, True),      # q, k in [-8, 8]: logits of +-20 and beyond, the max subtraction matters (observed 2.8e-6; the
                              # same graph in float32 on the CPU: 1.7e-6)
])
def test_attention_backward_materialised_head32(ag, B, heads, N, Nk, big):
    hd = 32
    q, kv, g = attention_inputs(B, heads, N, Nk, hd, big)
    y, dq, dkv = attention_reference(q, kv, g, heads, hd)
    t = Track(f"nodes_attention32[{B}-{heads}-{N}-{Nk}{'-big' if big else ''}]")
    qg, kvg = leaf(q, "cuda"), leaf(kv, "cuda")
    yg = ag.sr_attention(qg, kvg, heads, hd ** -0.5)
    t("y", yg, y)
    yg.backward(g.cuda())
    assert kvg.grad.shape == kv.shape
    t("dq", qg.grad, dq)
    t("dkv", kvg.grad, dkv)


def test_attention_backward_refuses_more_than_1024_keys_at_head32(ag):
    """Score pitch 1040 > 1024: the row kernels hold a row in 16 registers per lane and refuse; no numbers come back."""
    q, kv, g = attention_inputs(1, 1, 8, 1025, 32)
    qg, kvg = leaf(q, "cuda"), leaf(kv, "cuda")
    with pytest.raises(RuntimeError):
        ag.sr_attention(qg, kvg, 1, 32 ** -0.5).backward(g.cuda())
    assert qg.grad is None and kvg.grad is None


def test_attention_backward_materialised_head64_without_the_switch(ag, monkeypatch):
    """Head size 64 reaches the materialising path without SEGMIF_ATTN_BWD through storage the fused kernel cannot take.
    A non-contiguous q (a channel slice of a wider tensor) never gets that far: the FORWARD refuses it.  What does get there is
    a cotangent that is contiguous but not on a 16-byte boundary (a slice of a wider flat tensor)."""
    B, heads, N, Nk, hd = 1, 2, 70, 35, 64
    q, kv, g = attention_inputs(B, heads, N, Nk, hd)
    y, dq, dkv = attention_reference(q, kv, g, heads, hd)
    t = Track("nodes_attention64_unaligned_cotangent")
    wide = rnd(B, N, heads * hd + 8, seed=23).cuda()
    with pytest.raises(RuntimeError):
        ag.sr_attention(wide[..., 4:4 + heads * hd], kv.cuda(), heads, hd ** -0.5)

    def fused(*a, **k):
        raise AssertionError("the fused backward ran: the cotangent was expected to be refused by its alignment test")

    monkeypatch.setattr(ag.ops, "sr_attention_bwd", fused)
    flat = torch.empty(g.numel() + 1, device="cuda")
    gd = flat[1:].view(g.shape)
    gd.copy_(g)
    assert gd.is_contiguous() and gd.data_ptr() % 16 == 4
    qg, kvg = leaf(q, "cuda"), leaf(kv, "cuda")
    yg = ag.sr_attention(qg, kvg, heads, hd ** -0.5)
    t("y", yg, y)
    yg.backward(gd)
    t("dq", qg.grad, dq)
    t("dkv", kvg.grad, dkv)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. glue and colour nodes
# ------------------------------------------------------------------------------------------------------------------------------
def silu(z):
    return z * torch.sigmoid(z)


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("C", [32, 36])
def test_silu_sum_node(ag, C, two):
    """Inputs = channel slices of wider leaves, the output placed into a NaN-filled buffer (two inputs) or fresh (one input),
    the cotangent a channel slice of a wider gradient."""
    rows, before = 1001, 8
    abuf, bbuf = rnd(rows, C + 16, seed=3, lo=-30.0, hi=30.0), rnd(rows, C + 8, seed=4, lo=-30.0, hi=30.0)
    abuf[::7, 8:8 + C:5] = 0.0
    G = rnd(rows, before + C, seed=5)
    ar, br = leaf(abuf[:, 8:8 + C], double=True), leaf(bbuf[:, 4:4 + C], double=True)
    y = silu(ar) + silu(br) if two else silu(ar)
    y.backward(G[:, before:].double())
    t = Track(f"nodes_silu_sum[{C}-{'two' if two else 'one'}]")
    ag_, bg_ = leaf(abuf, "cuda"), leaf(bbuf, "cuda")
    a, b = ag_[:, 8:8 + C], bg_[:, 4:4 + C]
    if two:
        buf = nan_buf(rows, C + 24)
        yg = ag.silu_sum(a, b, out=ag.Out(buf[:, 16:16 + C]))
        assert yg.data_ptr() == buf[:, 16:].data_ptr() and only_view_written(buf, 16, 16 + C)
    else:
        yg = ag.silu_sum(a)
    t("y", yg, y.detach(), SILU_TOL)
    sliced_cotangent(yg, G.cuda(), before)
    t("da", ag_.grad[:, 8:8 + C], ar.grad, SILU_TOL)
    assert float(ag_.grad[:, :8].abs().max()) == 0.0 and float(ag_.grad[:, 8 + C:].abs().max()) == 0.0
    if two:
        t("db", bg_.grad[:, 4:4 + C], br.grad, SILU_TOL)
        assert float(bg_.grad[:, :4].abs().max()) == 0.0 and float(bg_.grad[:, 4 + C:].abs().max()) == 0.0
        assert only_view_written(buf, 16, 16 + C)
    else:
        assert bg_.grad is None


@pytest.mark.parametrize("s_grad", [True, False])
def test_add_shared_node(ag, s_grad):
    shape = (3, 333, 36)
    a1, a2, s, g1, g2 = (rnd(*shape, seed=90 + i) for i in range(5))
    t = Track(f"nodes_add_shared[{'s' if s_grad else 'frozen_s'}]")
    a1g, a2g = leaf(a1, "cuda"), leaf(a2, "cuda")
    sg = leaf(s, "cuda") if s_grad else s.cuda()
    y1, y2 = ag.add_shared(a1g, a2g, sg)
    t("y1", y1, a1.double() + s.double())
    t("y2", y2, a2.double() + s.double())
    torch.autograd.backward([y1, y2], [g1.cuda(), g2.cuda()])
    t("da1", a1g.grad, g1.double())
    t("da2", a2g.grad, g2.double())
    if s_grad:
        t("ds", sg.grad, g1.double() + g2.double())
    else:
        assert sg.grad is None


def test_join_node(ag):
    """Two producers write their results into the two channel blocks of one buffer (out= placements); ag.join returns the buffer
    and hands each producer the matching slice of the whole's gradient - compared with cat(LayerNorm(x1), Linear(x2)) in float64."""
    rows, C1, C2, K = 517, 32, 16, 64
    x1, gm, bt = rnd(rows, C1, seed=100, lo=-3, hi=5), rnd(C1, seed=101), rnd(C1, seed=102)
    x2, w, b, G = rnd(rows, K, seed=103), rnd(C2, K, seed=104), rnd(C2, seed=105), rnd(rows, C1 + C2, seed=106)
    r1, rg, rb, r2, rw, rbias = (leaf(v, double=True) for v in (x1, gm, bt, x2, w, b))
    y = torch.cat([F.layer_norm(r1, (C1,), rg, rb, 1e-6), F.linear(r2, rw, rbias)], dim=1)
    y.backward(G.double())
    t = Track("nodes_join")
    d1, dg, db_, d2, dw_, dbias = (leaf(v, "cuda") for v in (x1, gm, bt, x2, w, b))
    buf = nan_buf(rows, C1 + C2)
    p1 = ag.layernorm(d1, dg, db_, 1e-6, out=ag.Out(buf[:, :C1]))
    p2 = ag.linear(d2, dw_, dbias, out=ag.Out(buf[:, C1:]))
    seen = {}
    p1.register_hook(lambda gr: seen.__setitem__("p1", gr.clone()))
    p2.register_hook(lambda gr: seen.__setitem__("p2", gr.clone()))
    whole = ag.join(ag.Out(buf), p1, p2)
    assert whole.data_ptr() == buf.data_ptr() and whole.shape == buf.shape
    t("whole", whole, y.detach())
    Gd = G.cuda()
    whole.backward(Gd)
    assert torch.equal(seen["p1"], Gd[:, :C1]) and torch.equal(seen["p2"], Gd[:, C1:])
    for name, got, ref in (("dx1", d1, r1), ("dgamma", dg, rg), ("dbeta", db_, rb), ("dx2", d2, r2), ("dw", dw_, rw),
                           ("dbias", dbias, rbias)):
        t(name, got.grad, ref.grad)
    with pytest.raises(RuntimeError):  # parts that are not the buffer's slices are refused
        ag.join(ag.Out(buf), p2, p1)


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 5, 7),     # smaller than the window
                                     (2, 3, 32, 32), (1, 2, 33, 65), (1, 1, 11, 100)])
def test_gauss_blur11_node(ag, B, C, H, W):
    x, g = rnd(B, C, H, W, seed=110, lo=0, hi=1), rnd(B, C, H, W, seed=111)
    taps = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    taps = taps / taps.sum()
    window = torch.outer(taps, taps).expand(C, 1, 11, 11).contiguous()
    xr = leaf(x, double=True)
    y = F.conv2d(xr, window, padding=5, groups=C)
    y.backward(g.double())
    t = Track(f"nodes_gauss_blur11[{B}-{C}-{H}-{W}]")
    xg = leaf(x, "cuda")
    yg = ag.gauss_blur11(xg)
    t("y", yg, y.detach())
    yg.backward(g.cuda())
    t("dx", xg.grad, xr.grad)


def test_colour_nodes(ag):
    B, H, W = 2, 11, 17
    rgb, ycc, yl = rnd(B, 3, H, W, seed=120, lo=0, hi=1), rnd(B, 3, H, W, seed=121, lo=0, hi=1), rnd(B, 1, H, W, seed=122, lo=0, hi=1)
    g = rnd(B, 3, H, W, seed=123)
    t = Track("nodes_colour")
    # rgb -> YCrCb
    rr = leaf(rgb, double=True)
    y = so.rgb2ycrcb(rr)
    y.backward(g.double())
    rg = leaf(rgb, "cuda")
    yg = ag.rgb2ycrcb(rg)
    t("rgb2ycrcb y", yg, y.detach())
    yg.backward(g.cuda())
    t("rgb2ycrcb dx", rg.grad, rr.grad)
    # YCrCb -> rgb
    cr = leaf(ycc, double=True)
    y = so.ycrcb2rgb(cr)
    y.backward(g.double())
    cg = leaf(ycc, "cuda")
    yg = ag.ycrcb2rgb(cg)
    t("ycrcb2rgb y", yg, y.detach())
    yg.backward(g.cuda())
    t("ycrcb2rgb dx", cg.grad, cr.grad)
    # YCrCb -> rgb with the luminance taken from another tensor: channel 0 of ycc is not read
    cr, lr = leaf(ycc, double=True), leaf(yl, double=True)
    y = so.ycrcb2rgb(torch.cat((lr, cr[:, 1:2], cr[:, 2:3]), dim=1))
    y.backward(g.double())
    cg, lg = leaf(ycc, "cuda"), leaf(yl, "cuda")
    yg = ag.ycrcb2rgb(cg, lg)
    t("ycrcb2rgb(y) y", yg, y.detach())
    yg.backward(g.cuda())
    t("ycrcb2rgb(y) dycc", cg.grad, cr.grad)
    assert float(cg.grad[:, 0].abs().max()) == 0.0
    t("ycrcb2rgb(y) dy", lg.grad, lr.grad)
    # ... and with only the luminance wanting a gradient (the one-plane form of the backward kernel)
    lg = leaf(yl, "cuda")
    ag.ycrcb2rgb(ycc.cuda(), lg).backward(g.cuda())
    t("ycrcb2rgb(y) dy alone", lg.grad, lr.grad)


@pytest.mark.parametrize("C", [9, 32])
def test_nchw_to_nhwc_node(ag, C):
    B, H, W = 2, 37, 5
    x, g = rnd(B, C, H, W, seed=130), rnd(B, H, W, C, seed=131)
    xg = leaf(x, "cuda")
    y = ag.NchwToNhwcFn.apply(xg)
    assert y.is_contiguous() and torch.equal(y.cpu(), x.permute(0, 2, 3, 1))
    y.backward(g.cuda())
    assert xg.grad.is_contiguous() and torch.equal(xg.grad.cpu(), g.permute(0, 3, 1, 2))
    observed(f"nodes_nchw_to_nhwc[{C}]", 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. placed outputs and sliced gradients on the nodes test_gpu_backward.py tests contiguous
# ------------------------------------------------------------------------------------------------------------------------------
def test_linear_placed_output_and_sliced_gradient(ag):
    M, N, K, before = 777, 32, 64, 8
    x, w, b, G = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(M, before + N, seed=4)
    xr, wr, br = leaf(x, double=True), leaf(w, double=True), leaf(b, double=True)
    y = F.linear(xr, wr, br)
    y.backward(G[:, before:].double())
    t = Track("nodes_placed_linear")
    xg, wg, bg = leaf(x, "cuda"), leaf(w, "cuda"), leaf(b, "cuda")
    buf = nan_buf(M, N + 32)
    yg = ag.linear(xg, wg, bg, out=ag.Out(buf[:, 16:16 + N]))
    assert yg.data_ptr() == buf[:, 16:].data_ptr() and only_view_written(buf, 16, 16 + N)
    t("y", yg, y.detach())
    sliced_cotangent(yg, G.cuda(), before)
    t("dx", xg.grad, xr.grad)
    t("dw", wg.grad, wr.grad)
    t("db", bg.grad, br.grad)
    assert only_view_written(buf, 16, 16 + N)


def test_layernorm_placed_output_and_sliced_gradient(ag):
    rows, C, before = 517, 64, 8
    x, gm, bt, G = rnd(rows, C, seed=9, lo=-3, hi=5), rnd(C, seed=10), rnd(C, seed=11), rnd(rows, before + C, seed=12)
    xr, gr, br = leaf(x, double=True), leaf(gm, double=True), leaf(bt, double=True)
    y = F.layer_norm(xr, (C,), gr, br, 1e-6)
    y.backward(G[:, before:].double())
    t = Track("nodes_placed_layernorm")
    xg, gg, bg = leaf(x, "cuda"), leaf(gm, "cuda"), leaf(bt, "cuda")
    buf = nan_buf(rows, C + 32)
    yg = ag.layernorm(xg, gg, bg, 1e-6, out=ag.Out(buf[:, 16:16 + C]))
    assert yg.data_ptr() == buf[:, 16:].data_ptr() and only_view_written(buf, 16, 16 + C)
    t("y", yg, y.detach())
    sliced_cotangent(yg, G.cuda(), before)
    t("dx", xg.grad, xr.grad)
    t("dgamma", gg.grad, gr.grad)
    t("dbeta", bg.grad, br.grad)
    assert only_view_written(buf, 16, 16 + C)


@pytest.mark.parametrize("C", [32, 9])  # 9: pitch 17, no 16-byte rows - the node copies the slice before the scalar kernel reads it
def test_bilinear_placed_output_and_sliced_gradient(ag, C):
    B, IH, IW, OH, OW, before = 1, 5, 7, 18, 26, 8
    x, G = rnd(B, IH, IW, C, seed=17), rnd(B, OH, OW, before + C, seed=18)
    xr = leaf(x.permute(0, 3, 1, 2), double=True)
    y = F.interpolate(xr, size=[OH, OW], mode="bilinear", align_corners=False)
    y.backward(G[..., before:].permute(0, 3, 1, 2).double())
    t = Track(f"nodes_placed_bilinear[{C}]")
    xg = leaf(x, "cuda")
    buf = nan_buf(B, OH, OW, C + 32)
    yg = ag.bilinear(xg, OH, OW, out=ag.Out(buf[..., 16:16 + C]))
    assert yg.data_ptr() == buf[..., 16:].data_ptr() and only_view_written(buf, 16, 16 + C)
    t("y", yg, y.detach().permute(0, 2, 3, 1))
    sliced_cotangent(yg, G.cuda(), before)
    t("dx", xg.grad, xr.grad.permute(0, 2, 3, 1))
    assert only_view_written(buf, 16, 16 + C)
