"""The fp32 row kernels - LayerNorm, softmax / cross-entropy, GELU / SiLU, BatchNorm, the fp32 attention and their backward nodes -
held to fp32 accuracy across scales and offsets (tests/_value_domain.py: regimes, float64 references, conditioning terms,
yardsticks; tests/test_value_domain_host.py: the measure proven on the CPU).

Every compared tensor must satisfy  rho_kernel <= F * max(rho_yardstick, 1),  rho = max |got - ref| / (u cond + tiny), both sides
computed here on the same input, the yardstick by torch in fp32 on the CPU.  F is one constant per family: the next power of two
at or above twice the worst ratio rho_kernel / max(rho_yardstick, 1) observed on an MI355X, and never above 8.  Every ratio is
printed and recorded under value_domain_* (tests/_observed.py) before anything is asserted; a test asserts once, at its end, so
one run shows every figure of a family."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _value_domain as vd
from _observed import observed
from test_value_domain_host import (add_layernorm_inputs, ce_labels, conv_ln_case, conv_ln_inputs, linear_ln_case,
                                    linear_ln_inputs)

pytestmark = pytest.mark.gpu

# F = the next power of two at or above twice the worst ratio observed on an MI355X (gfx950); every ratio of that run is kept in
# profiles/value_domain_parity_observed/.  Worst ratio (case): rho of the kernel there / rho of the yardstick there.
F_LAYERNORM = 4.0   # 1.27 (forward C=64 scales eps=1e-5): 1.53 / 1.21; over all 210 figures kernel 0.41 .. 3.78, yardstick 0.45 .. 4.94
F_SOFTMAX = 2.0     # 1.00 (ce grad, row_softmax_bwd, pseudo_label, tta_vote: the kernel's rho IS the yardstick's); kernel 0.01 .. 3.09
F_ACTIVATION = 4.0  # 1.26 (pointwise2_bwd mode 1 db): 1.59 / 1.26; kernel 0.10 .. 1.84, yardstick 0.30 .. 4.14
F_BATCHNORM = 4.0   # 1.02 (backward dbeta): 1.02 / 0.32; kernel 0.51 .. 1.58, yardstick 0.18 .. 1.84
F_ATTENTION = 4.0   # 1.45 (fused hd=64 spread=100 dkv): 1.45 / 0.66; kernel 0.11 .. 1.45, yardstick 0.12 .. 0.98

ROWS = 96
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from segmif_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def ag(ops):
    from segmif_amd import autograd as _ag
    return _ag


class Check:
    """rho of the kernel and of the yardstick for every compared tensor of one test; asserts once, in done()."""

    def __init__(self, family, factor):
        assert factor <= vd.F_CAP
        self.family, self.factor, self.bad, self.worst = family, factor, [], 0.0

    def __call__(self, case, got, ref, cond, yard):
        rk, ry = vd.rho(got, ref, cond), vd.rho(yard, ref, cond)
        ratio = rk / max(ry, 1.0)
        self.worst = max(self.worst, ratio)
        observed(f"value_domain_{self.family} {case}", {"kernel": rk, "yardstick": ry, "ratio": ratio})
        print(f"value_domain_{self.family} {case}: kernel {rk:.3f} yardstick {ry:.3f} ratio {ratio:.3f}")
        if not vd.passes(rk, ry, self.factor):
            self.bad.append((case, rk, ry))
        return rk

    def that(self, case, ok):
        if not ok:
            self.bad.append((case, "property"))

    def done(self):
        print(f"value_domain_{self.family}: worst ratio {self.worst:.3f} (F = {self.factor})")
        assert not self.bad, self.bad


def leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (32, 64, 160, 320, 1024))  # layernorm_kernel / layernorm_bwd_kernel <8..64, 1>, <64, 1>, <64, 2>, <64, 4>
def test_layernorm_forward_and_backward(ops, ag, C):
    chk = Check("layernorm", F_LAYERNORM)
    g, b = vd.affine(C)
    for regime in vd.REGIMES:
        x = vd.rows_regime(regime, ROWS, C, seed=C)
        dy = vd.cotangent(x.shape, seed=1)
        for eps in (1e-6, 1e-5):
            ref, cond, yard = vd.layernorm_case(x, g, b, eps)
            pitched = regime == "offset" and eps == 1e-5  # once into a channel slice of a wider buffer
            wide = torch.full((ROWS, C + 32), NAN, device="cuda") if pitched else None
            y = ops.layernorm(x.cuda(), g.cuda(), b.cuda(), eps, out=wide[:, 16:16 + C] if pitched else None)
            chk(f"forward C={C} {regime} eps={eps}", y, ref, cond, yard)
            if pitched:
                chk.that("pitched out= leaves its neighbours alone", bool(torch.isnan(wide[:, :16]).all() and torch.isnan(wide[:, 16 + C:]).all()))
            if regime == "zero":
                zero_rows = (x.abs().amax(-1) == 0).nonzero()[:, 0]
                chk.that(f"zero rows return beta bit for bit (C={C}, eps={eps})",
                         len(zero_rows) == 3 and all(torch.equal(y[r].cpu(), b) for r in zero_rows))
            xg, gg, bg = leaf(x), leaf(g), leaf(b)
            ag.layernorm(xg, gg, bg, eps).backward(dy.cuda())
            for (k, (r, c, yd)), got in zip(vd.layernorm_bwd_case(x, g, b, dy, eps).items(), (xg.grad, gg.grad, bg.grad)):
                chk(f"backward {k} C={C} {regime} eps={eps}", got, r, c, yd)
    chk.done()


@pytest.mark.parametrize("C", (64, 160))
def test_add_layernorm_forward_and_backward(ag, C):
    chk = Check("layernorm", F_LAYERNORM)
    g, b = vd.affine(C)
    for regime in vd.REGIMES:
        x, br, sc, ds, dn = add_layernorm_inputs(regime, 2, ROWS // 2, C)
        xg, brg, gg, bg = leaf(x), leaf(br), leaf(g), leaf(b)
        s, n = ag.add_layernorm(xg, brg, sc.cuda(), gg, bg, 1e-6)
        torch.autograd.backward([s, n], [ds.cuda(), dn.cuda()])
        got = {"s": s, "n": n, "dx": xg.grad, "dbranch": brg.grad, "dgamma": gg.grad, "dbeta": bg.grad}
        for k, (r, c, yd) in vd.add_layernorm_case(x, br, sc, g, b, ds, dn, 1e-6).items():
            chk(f"add_layernorm {k} C={C} {regime}", got[k], r, c, yd)
        if regime == "zero":
            both = ((x.abs().amax(-1) == 0) & (br.abs().amax(-1) == 0)).nonzero()
            chk.that("zero rows return beta bit for bit", len(both) > 0 and all(torch.equal(n[i, j].detach().cpu(), b) for i, j in both))
    chk.done()


def test_layernorm_epilogues_of_linear_and_conv(ops):
    """N = 64: the LayerNorm rides in the GEMM's / conv's epilogue; the residual puts its input in the offset regime."""
    chk = Check("layernorm", F_LAYERNORM)
    g, b = vd.affine(64)
    x, w, bias, res = linear_ln_inputs()
    ref, cond, yard = linear_ln_case(x, w, bias, res, g, b, 1e-6)
    y = ops.linear(x.cuda(), ops.pack_weight(w.cuda()), 64, bias=bias.cuda(), res=res.cuda(), ln=(g.cuda(), b.cuda(), 1e-6))
    chk("linear epilogue offset", y, ref, cond, yard)
    x, w, bias, res = conv_ln_inputs()
    ref, cond, yard = conv_ln_case(x, w, bias, res, g, b, 1e-5)
    y = ops.conv2d(x.cuda(), ops.pack_weight(w.cuda()), 64, 3, pad=1, bias=bias.cuda(), res=res.cuda(), ln=(g.cuda(), b.cuda(), 1e-5))
    chk("conv epilogue offset", y, ref, cond, yard)
    chk.done()


# ------------------------------------------------------------------------------------------------------------------------------
# softmax family
# ------------------------------------------------------------------------------------------------------------------------------
def test_softmax_ce_loss_and_gradient(ag):
    """C = 9 on a (2, 6, 8) image with ignored pixels: all pixels at once, then one logit regime at a time (the mean over all
    96 pixels is dominated by the widest spread), the equal-logit pixels last: their loss is log C.
    (This test found softmax_ce_kernel forming (log sum + max) - x_label: rounded at |max|'s size, rho 16 .. 103 on the rows around
    -16384 and 1024 against the yardstick's 0.1 .. 0.8; the kernel now forms log sum + (max - x_label).)"""
    chk = Check("softmax", F_SOFTMAX)
    C = 9
    x, which = vd.logit_rows(ROWS, C, seed=C)
    lab = ce_labels(ROWS, C)
    equal = torch.zeros(ROWS, dtype=torch.bool)
    equal[:vd.N_EQUAL] = True
    for name, keep in [("all", None)] + [(f"spread{si}", which == si) for si in range(-1, len(vd.LOGIT_SPREADS))] + [("equal", equal)]:
        l2 = lab.clone()
        if keep is not None:
            l2[~keep] = 255
        if name == "equal":
            l2[:vd.N_EQUAL] = torch.arange(vd.N_EQUAL)
        case = vd.ce_case(x, l2)
        xg = leaf(x.view(2, 6, 8, C))
        loss = ag.softmax_ce(xg, l2.view(2, 6, 8).cuda(), 255)
        loss.backward()
        chk(f"ce loss {name}", loss.detach().cpu(), *case["loss"])
        chk(f"ce grad {name}", xg.grad.view(ROWS, C), *case["grad"])
        if name == "equal":
            r, c, yd = case["loss"]
            chk("ce loss of equal logits against log C", loss.detach().cpu(), torch.tensor(math.log(C), dtype=torch.float64), c, yd)
    chk.done()


@pytest.mark.parametrize("L", (6, 35, 300))
@pytest.mark.parametrize("scale", (0.125, 32 ** -0.5))
def test_row_softmax_and_its_backward(ops, L, scale):
    """segmif_row_softmax_f32 / segmif_row_softmax_bwd_f32 through the C ABI, in place on a pitched buffer (ld = L rounded up to 16,
    the padding must come back zero)."""
    from segmif_amd import _lib
    lib = _lib.load()
    chk = Check("softmax", F_SOFTMAX)
    x, _ = vd.logit_rows(ROWS, L, seed=L)
    ld = (L + 15) // 16 * 16
    buf = torch.full((ROWS, ld), NAN, device="cuda")
    buf[:, :L] = x.cuda()
    _lib.check(lib.segmif_row_softmax_f32(buf.data_ptr(), ROWS, L, ld, float(scale), ops._stream()), "segmif_row_softmax_f32")
    p, cond, yard = vd.softmax_case(x, scale)
    chk(f"row_softmax L={L} scale={scale:.4f}", buf[:, :L], p, cond, yard)
    chk.that("padding zeroed", float(buf[:, L:].abs().sum()) == 0.0)
    eq = slice(0, vd.N_EQUAL)
    chk(f"row_softmax equal logits against 1/L L={L} scale={scale:.4f}", buf[eq, :L], torch.full((vd.N_EQUAL, L), 1.0 / L, dtype=torch.float64),
        cond[eq], yard[eq])
    p32, dp = p.float(), vd.cotangent(x.shape, seed=3)
    pb, db = torch.zeros((ROWS, ld), device="cuda"), torch.full((ROWS, ld), NAN, device="cuda")
    pb[:, :L], db[:, :L] = p32.cuda(), dp.cuda()
    _lib.check(lib.segmif_row_softmax_bwd_f32(pb.data_ptr(), db.data_ptr(), ROWS, L, ld, float(scale), ops._stream()), "segmif_row_softmax_bwd_f32")
    chk(f"row_softmax_bwd L={L} scale={scale:.4f}", db[:, :L], *vd.softmax_bwd_case(p32, dp, scale))
    chk.that("padding zeroed (backward)", float(db[:, L:].abs().sum()) == 0.0)
    chk.done()


def test_pseudo_label_confidence_and_tta_probabilities(ops):
    """both at the output size: the bilinear weights are 1 and 0, the logits reach the softmax unchanged"""
    chk = Check("softmax", F_SOFTMAX)
    C, H, W = 9, 8, 12
    x, _ = vd.logit_rows(ROWS, C, seed=C)
    p, cond, yard = vd.softmax_case(x)
    top = p.argmax(-1, keepdim=True)
    labels, count, conf = ops.pseudo_label(x.view(1, H, W, C).cuda(), H, W, return_conf=True)
    chk("pseudo_label confidence", conf.view(ROWS), p.gather(1, top)[:, 0], cond.gather(1, top)[:, 0], yard.amax(-1))
    stable = (p.topk(2, -1).values[:, 0] - p.topk(2, -1).values[:, 1]) > 1e-3
    chk.that("pseudo_label labels", torch.equal(labels.view(ROWS).cpu()[stable], top[:, 0][stable]))
    chk.that("pseudo_label count", int(count[0]) == int((conf.view(ROWS) > 0.968).sum()))
    _, probs = ops.tta_vote([x.view(1, H, W, C).cuda()], [False], H, W, want_probs=True)
    chk("tta_vote probabilities", probs.view(ROWS, C), p, cond, yard)
    eq = slice(0, vd.N_EQUAL)
    chk("tta_vote equal logits against 1/C", probs.view(ROWS, C)[eq], torch.full((vd.N_EQUAL, C), 1.0 / C, dtype=torch.float64), cond[eq], yard[eq])
    chk.done()


# ------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------
def centre_tap(C):
    w = torch.zeros(C, 1, 3, 3)
    w[:, 0, 1, 1] = 1.0
    return w, torch.zeros(C)


# W >= 16: the two-column forward kernel, W < 16: the one-column one.  The backward kernel takes C % 128 == 0 only: 128 there.
@pytest.mark.parametrize("H,W,C,backward", [(9, 25, 64, False), (9, 25, 128, True), (25, 9, 128, True)])
def test_dwconv_gelu_forward_and_backward_on_the_grid(ops, ag, H, W, C, backward):
    """centre tap 1, bias 0: the depthwise conv hands the grid to the GELU unchanged"""
    chk = Check("activation", F_ACTIVATION)
    x = vd.grid_filled((1, H * W, C), seed=H)
    w, bias = centre_tap(C)
    ref, cond, yard = vd.gelu_case(x)
    y = ops.dwconv3x3_gelu(x.cuda(), ops.pack_dw_weight(w.cuda()), bias.cuda(), H, W)
    chk(f"dwconv3x3_gelu {H}x{W}x{C}", y, ref, cond, yard)
    if not backward:
        return chk.done()
    dy = vd.cotangent(x.shape, seed=4)
    hg, wg, bg = leaf(x), leaf(w), leaf(bias)
    ag.dwconv_gelu(hg, wg, bg, H, W).backward(dy.cuda())

    def run(dt):
        hs, ws, bs = (t.detach().to(dt).requires_grad_(True) for t in (x, w, bias))
        img = hs.transpose(1, 2).reshape(1, C, H, W)
        F.gelu(F.conv2d(img, ws, bs, padding=1, groups=C)).flatten(2).transpose(1, 2).backward(dy.to(dt))
        return hs.grad, ws.grad, bs.grad

    r, yd = run(torch.float64), run(torch.float32)
    cdz = dy.double().abs() * (1.0 + x.double().abs())  # dz = dy gelu'(x); the centre tap hands it to dh unchanged
    xs = x.double().requires_grad_(True)
    F.gelu(xs).sum().backward()
    dz_abs = (dy.double() * xs.grad).abs()
    as_img = lambda t: t.transpose(1, 2).reshape(1, C, H, W)  # noqa: E731
    # dw[c][tap] = sum over pixels of dz * h(shifted): the error of dz times |h| plus the products' own roundings; db = sum dz
    cdw = torch.nn.grad.conv2d_weight(as_img(x.double().abs()), w.shape, as_img(cdz + dz_abs), padding=1, groups=C)
    cdb = (cdz + dz_abs).sum((0, 1))
    chk(f"dwconv_gelu backward dh {H}x{W}x{C}", hg.grad, r[0], cdz, yd[0])
    chk(f"dwconv_gelu backward dw {H}x{W}x{C}", wg.grad, r[1], cdw, yd[1])
    chk(f"dwconv_gelu backward db {H}x{W}x{C}", bg.grad, r[2], cdb, yd[2])
    chk.done()


def test_gelu_epilogue_of_linear(ops):
    """identity weight, K = N = 64: the GEMM hands the grid to ACT_GELU unchanged"""
    chk = Check("activation", F_ACTIVATION)
    x = vd.grid_filled((ROWS, 64), seed=2)
    y = ops.linear(x.cuda(), ops.pack_weight(torch.eye(64).cuda()), 64, act=ops.ACT_GELU)
    chk("linear ACT_GELU epilogue", y, *vd.gelu_case(x))
    chk.done()


def test_dwconv_gelu_pairs_against_the_as_restatement(ops):
    """gelu_as (csrc/split_ops.h) inside a guarded scope: held to the float64 restatement of A&S 7.1.26 (which the host test
    holds to the header's 7.5e-8 |x| of the true GELU), yardstick the same formula in fp32 numpy.  The result is a PAIRS tensor:
    its 22 bits are a documented format, so cond carries vd.pairs_extra (no larger F)."""
    chk = Check("activation", F_ACTIVATION)
    H, W, C = 9, 25, 64
    x = vd.grid_filled((1, H * W, C), seed=H)
    w, bias = centre_tap(C)
    prev = ops.install_guard(ops.Planes16Guard("cuda", 1))
    try:
        yp = ops.dwconv3x3_gelu_pairs(x.cuda(), ops.pack_dw_weight(w.cuda()), bias.cuda(), H, W)
        y = ops.pairs_to_f32(yp)
    finally:
        ops.install_guard(prev)
    ref = torch.from_numpy(vd.gelu_as(x.double().numpy()))
    yard = torch.from_numpy(vd.gelu_as(x.numpy(), np.float32))
    chk("dwconv3x3_gelu_pairs", y, ref, x.double().abs() + vd.pairs_extra(ref), yard)
    chk.done()


@pytest.mark.parametrize("mode", (1, 2))
def test_pointwise2_silu_forward_and_backward(ops, mode):
    """silu_f divides by 1 + __expf(-z): the hardware exponential's published error enters cond (vd.silu_fast_exp_extra), not F.
    The backward uses expf."""
    chk = Check("activation", F_ACTIVATION)
    a, b = vd.grid_filled((24, 64), extend=100, seed=5), vd.grid_filled((24, 64), extend=100, seed=6)
    ra, ca, ya = vd.silu_case(a)
    ca = ca + vd.silu_fast_exp_extra(a)
    if mode == 1:
        rb, cb, yb = vd.silu_case(b)
        ref, cond, yard = ra + rb, ca + cb + vd.silu_fast_exp_extra(b), ya + yb
    else:
        ref, cond, yard = ra, ca, ya
    y = ops.pointwise2(a.cuda(), b.cuda() if mode == 1 else None, mode)
    chk(f"pointwise2 mode {mode}", y, ref, cond, yard)
    dy = vd.cotangent(a.shape, seed=7)
    da, db = ops.pointwise2_bwd(dy.cuda(), a.cuda(), b.cuda() if mode == 1 else None, mode)
    chk(f"pointwise2_bwd mode {mode} da", da, *vd.act_bwd_case(F.silu, a, dy))
    if mode == 1:
        chk(f"pointwise2_bwd mode {mode} db", db, *vd.act_bwd_case(F.silu, b, dy))
    else:
        chk.that("mode 2 has no db", db is None)
    chk.done()


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU (train mode)
# ------------------------------------------------------------------------------------------------------------------------------
def test_batchnorm_relu_train_forward_and_backward(ag):
    """rows = 300 (two 256-row blocks, the second partial), C = 32, columns from scales, offset and both.  The elements whose
    float64 pre-activation lies within 16 u cond of zero may sit on either side of the ReLU: they (at most 1 %) get a zero
    cotangent, nothing else is left out."""
    chk = Check("batchnorm", F_BATCHNORM)
    rows, C, eps = 300, 32, 1e-5
    x = vd.batchnorm_columns(rows, C)
    g, b = vd.batchnorm_affine(C)
    ref, cond, yard, z, flip = vd.batchnorm_case(x, g, b, eps)
    share = float(flip.double().mean())
    print("mask-flip candidates:", share)
    chk.that("mask-flip candidates at most 1 %", share <= 0.01)
    dy = vd.cotangent(x.shape, seed=2) * ~flip
    xg, gg, bg = leaf(x), leaf(g), leaf(b)
    y, mean, var = ag.batchnorm_relu_train(xg, gg, bg, eps)
    y.backward(dy.cuda())
    chk("forward", y, ref, cond, yard)
    stats = vd.batchnorm_stats_case(x)
    chk("batch mean", mean, *stats["mean"])
    chk("batch var", var, *stats["var"])
    for (k, (r, c, yd)), got in zip(vd.batchnorm_bwd_case(x, g, b, dy, eps).items(), (xg.grad, gg.grad, bg.grad)):
        chk(f"backward {k}", got, r, c, yd)
    chk.done()


# ------------------------------------------------------------------------------------------------------------------------------
# attention backward (and the fp32 forward in front of it)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,geom", [("fused", (1, 1, 96, 35, 64)), ("materialize", (1, 2, 64, 35, 32))])
@pytest.mark.parametrize("spread,late", [(1, False), (30, False), (100, False), (1, True)])
def test_sr_attention_backward_across_logit_spreads(ops, ag, mode, geom, spread, late):
    """rows from flat (spread 1) to saturated (spread 100: one key holds the row), and a key that dominates late"""
    chk = Check("attention", F_ATTENTION)
    B, heads, N, Nk, hd = geom
    q, kv, do = vd.attention_inputs(B, heads, N, Nk, hd, spread, late)
    qg, kvg = leaf(q), leaf(kv)
    with ops.modes(attn_bwd=mode):
        out = ag.sr_attention(qg, kvg, heads, hd ** -0.5)
        out.backward(do.cuda())
    got = {"out": out, "dq": qg.grad, "dkv": kvg.grad}
    for k, (r, c, yd) in vd.attention_case(q, kv, do, heads, hd ** -0.5).items():
        chk(f"{mode} hd={hd} spread={spread}{'+late' if late else ''} {k}", got[k], r, c, yd)
    chk.done()
