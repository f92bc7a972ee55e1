"""The value-domain measure of tests/_value_domain.py, proven on the CPU before any kernel is held to it:
  1. torch's own fp32 evaluation (the yardstick) reads rho <= 8 in every regime of every family and >= 0.1 in at least one - the
     conditioning terms are neither too tight for a correct fp32 evaluation nor so loose that they say nothing;
  2. fp32 restatements that are wrong in a way order-1 inputs hide (one-pass variance, softmax without its maximum, tanh GELU,
     CE as -log softmax) read rho > 1000 in at least one regime, while the suite's older max|got - ref| / max|ref| < 5e-5 bar on
     uniform [-3, 5) inputs lets them through (where it does not, the restatement's comment says so);
  3. the ReLU mask-flip exclusion of the BatchNorm node stays at or below 1 % of the elements;
  4. the float64 restatement of A&S 7.1.26 that the gelu_as kernels are held to is within the header's 7.5e-8 |x| of the true GELU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _value_domain as vd
from test_gpu_backward import TOL as OLD_TOL, err as old_err, rnd

LN_C = (32, 160, 1024)
EPS = (1e-6, 1e-5)
ROWS = 96


def check_range(name, rhos):
    """rhos: {regime: rho of the yardstick}"""
    print(name, {k: round(v, 3) for k, v in rhos.items()})
    assert max(rhos.values()) <= 8.0, (name, rhos)
    assert any(0.1 <= v for v in rhos.values()), (name, rhos)


# ------------------------------------------------------------------------------------------------------------------------------
# 0. the generators deliver what their names say
# ------------------------------------------------------------------------------------------------------------------------------
def test_regimes_are_finite_seeded_and_span_what_they_claim():
    for regime in vd.REGIMES:
        x = vd.rows_regime(regime, ROWS, 32, seed=3)
        assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
        assert torch.equal(x, vd.rows_regime(regime, ROWS, 32, seed=3))
    amax = vd.rows_regime("scales", ROWS, 160).abs().amax(-1)
    assert float(amax.min()) < 2.0 ** -20 and float(amax.max()) > 2.0 ** 19
    off = vd.rows_regime("offset", ROWS, 160).double()
    ratio = off.mean(-1).abs() / off.std(-1)
    assert float(ratio.max()) > 4096 * 64  # a mean 2^18 spreads above the row's spread
    zero = vd.rows_regime("zero", ROWS, 32)
    assert int((zero.abs().amax(-1) == 0).sum()) == 3
    x, which = vd.logit_rows(ROWS, 9)
    assert all(float(x[i].max()) == float(x[i].min()) for i in range(vd.N_EQUAL))
    assert sorted(set(which.tolist())) == [-1, 0, 1, 2, 3, 4]
    g = vd.activation_grid()
    assert g.numel() == 18 * 64 + 1 + 70 and float(g.abs().min()) == 0.0 and float(g.abs()[g != 0].min()) == 2.0 ** -30
    assert float(vd.activation_grid(100).max()) == 100.0
    bn = vd.batchnorm_columns(300, 32)
    assert tuple(bn.shape) == (300, 32) and bn.is_contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. yardstick range
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", LN_C)
def test_yardstick_layernorm(C):
    g, b = vd.affine(C)
    fwd, bwd = {}, {"dx": {}, "dgamma": {}, "dbeta": {}}
    for regime in vd.REGIMES:
        x = vd.rows_regime(regime, ROWS, C, seed=C)
        dy = vd.cotangent(x.shape, seed=1)
        for eps in EPS:
            ref, cond, yard = vd.layernorm_case(x, g, b, eps)
            fwd[f"{regime}/{eps}"] = vd.rho(yard, ref, cond)
            for k, (r, c, y) in vd.layernorm_bwd_case(x, g, b, dy, eps).items():
                bwd[k][f"{regime}/{eps}"] = vd.rho(y, r, c)
    check_range(f"layernorm C={C}", fwd)
    for k, v in bwd.items():
        check_range(f"layernorm_bwd {k} C={C}", v)


def add_layernorm_inputs(regime, B, N, C, seed=5):
    x, br = vd.rows_regime(regime, B * N, C, seed=seed).view(B, N, C), vd.rows_regime(regime, B * N, C, seed=seed + 1).view(B, N, C)
    sc = torch.tensor([1.0, 1.0 / 0.9] * B)[:B]  # (a DropPath keep of 0.9)
    return x, br, sc, vd.cotangent((B, N, C), seed=seed + 2), vd.cotangent((B, N, C), seed=seed + 3)


@pytest.mark.parametrize("C", (64, 160))
def test_yardstick_add_layernorm(C):
    g, b = vd.affine(C)
    table = {}
    for regime in vd.REGIMES:
        case = vd.add_layernorm_case(*add_layernorm_inputs(regime, 2, ROWS // 2, C)[:3], g, b, *add_layernorm_inputs(regime, 2, ROWS // 2, C)[3:], 1e-6)
        for k, (r, c, y) in case.items():
            table.setdefault(k, {})[regime] = vd.rho(y, r, c)
    for k, v in table.items():
        check_range(f"add_layernorm {k} C={C}", v)


def row_offsets(rows, N):
    """the per-row offset m_r of the offset regime as a (rows, N) residual"""
    return torch.tensor(vd.OFFSETS)[torch.arange(rows) % len(vd.OFFSETS)][:, None].expand(rows, N).contiguous()


def linear_ln_inputs(M=ROWS, K=64, N=64, seed=7):
    """x of order 1, w of order 0.1 and a residual that holds m_r in every column of row r: res + x w^T + bias, the epilogue's
    input, is in the offset regime.  -> x, w, bias, res"""
    g = vd.gen(seed)
    return vd.uniform(g, M, K).float(), (0.1 * vd.uniform(g, N, K)).float(), vd.uniform(g, N).float(), row_offsets(M, N)


def conv_ln_inputs(B=1, H=8, W=12, cin=8, N=64, seed=8):
    """the same through a 3 x 3 conv (x NHWC, res (B, H, W, N))"""
    g = vd.gen(seed)
    return (vd.uniform(g, B, H, W, cin).float(), (0.1 * vd.uniform(g, N, cin, 3, 3)).float(), vd.uniform(g, N).float(),
            row_offsets(B * H * W, N).view(B, H, W, N))


def linear_ln_case(x, w, bias, res, gamma, beta, eps):
    z64 = F.linear(x.double(), w.double(), bias.double()) + res.double()
    zabs = F.linear(x.double().abs(), w.double().abs(), bias.double().abs()) + res.double().abs()
    return vd.epilogue_layernorm_case(z64, zabs, F.linear(x, w, bias) + res, gamma, beta, eps)


def conv_ln_case(x, w, bias, res, gamma, beta, eps):
    nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    z64 = nhwc(F.conv2d(nchw(x.double()), w.double(), bias.double(), padding=1)) + res.double()
    zabs = nhwc(F.conv2d(nchw(x.double().abs()), w.double().abs(), bias.double().abs(), padding=1)) + res.double().abs()
    return vd.epilogue_layernorm_case(z64, zabs, nhwc(F.conv2d(nchw(x), w, bias, padding=1)) + res, gamma, beta, eps)


def test_yardstick_layernorm_epilogues():
    g, b = vd.affine(64)
    for name, case, inputs in (("linear", linear_ln_case, linear_ln_inputs), ("conv", conv_ln_case, conv_ln_inputs)):
        ref, cond, yard = case(*inputs(), g, b, 1e-6)
        assert float(ref.abs().max()) > 1.0  # (normalised, not flattened by eps)
        check_range(f"{name} + LayerNorm epilogue", {"offset": vd.rho(yard, ref, cond)})


def test_yardstick_batchnorm_and_mask_flip_share():
    rows, C = 300, 32
    x = vd.batchnorm_columns(rows, C)
    g, b = vd.batchnorm_affine(C)
    third = {"scales": slice(0, C // 3), "offset": slice(C // 3, 2 * (C // 3)), "both": slice(2 * (C // 3), C)}
    for eps in EPS:
        ref, cond, yard, z, flip = vd.batchnorm_case(x, g, b, eps)
        share = float(flip.double().mean())
        print("batchnorm mask-flip share", eps, share)
        assert share <= 0.01
        assert bool((ref > 0).all(0).any()) and bool((ref == 0).all(0).any()) and bool(((ref > 0).any(0) & (ref == 0).any(0)).any())
        check_range(f"batchnorm eps={eps}", {k: vd.rho(yard[:, s], ref[:, s], cond[:, s]) for k, s in third.items()})
        for k, (r, c, y) in vd.batchnorm_stats_case(x).items():
            check_range(f"batchnorm {k}", {name: vd.rho(y[s], r[s], c[s]) for name, s in third.items()})
        dy = vd.cotangent(x.shape, seed=2) * ~flip
        for k, (r, c, y) in vd.batchnorm_bwd_case(x, g, b, dy, eps).items():
            sel = (lambda t: t[:, s]) if k == "dx" else (lambda t: t[s])
            rh = {}
            for name, s in third.items():
                rh[name] = vd.rho(sel(y), sel(r), sel(c))
            check_range(f"batchnorm_bwd {k} eps={eps}", rh)


@pytest.mark.parametrize("L", (6, 9, 35, 300))
def test_yardstick_softmax(L):
    x, which = vd.logit_rows(ROWS, L, seed=L)
    dp = vd.cotangent(x.shape, seed=3)
    for scale in (1.0, 0.125, 32 ** -0.5):
        p, cond, yard = vd.softmax_case(x, scale)
        r, cb, yb = vd.softmax_bwd_case(p.float(), dp, scale)
        fwd, bwd = {}, {}
        for si in range(-1, len(vd.LOGIT_SPREADS)):
            rows = which == si
            fwd[si] = vd.rho(yard[rows], p[rows], cond[rows])
            bwd[si] = vd.rho(yb[rows], r[rows], cb[rows])
        check_range(f"softmax L={L} scale={scale}", fwd)
        check_range(f"softmax_bwd L={L} scale={scale}", bwd)


def ce_labels(rows, C, seed=1):
    lab = torch.randint(0, C, (rows,), generator=vd.gen(seed))
    lab[5::13] = 255
    return lab


def test_yardstick_cross_entropy():
    C = 9
    x, which = vd.logit_rows(ROWS, C, seed=C)
    lab = ce_labels(ROWS, C)
    loss, grad = {}, {}
    for si in [None] + list(range(-1, len(vd.LOGIT_SPREADS))):
        l2 = lab.clone()
        if si is not None:
            l2[which != si] = 255
        case = vd.ce_case(x, l2)
        loss[si], grad[si] = (vd.rho(y, r, c) for r, c, y in (case["loss"], case["grad"]))
    check_range("ce loss", loss)
    check_range("ce grad", grad)


def test_yardstick_activations():
    grid, ext = vd.activation_grid(), vd.activation_grid(100)
    dy = vd.cotangent((1, ext.numel()), seed=4)[0]
    parts = {"tail": ext < -3, "middle": ext.abs() <= 3, "right": ext > 3}
    for name, case, fn in (("gelu", vd.gelu_case, F.gelu), ("silu", vd.silu_case, F.silu)):
        for x in (grid, ext):
            r, c, y = case(x)
            check_range(f"{name} forward n={x.numel()}", {"all": vd.rho(y, r, c)})
        r, c, y = vd.act_bwd_case(fn, ext, dy)
        check_range(f"{name} derivative", {k: vd.rho(y[m], r[m], c[m]) for k, m in parts.items()})
    assert bool((vd.silu_fast_exp_extra(ext) >= 0).all()) and float(vd.silu_fast_exp_extra(ext).max()) < 8.0  # a few u at most


def test_gelu_as_restatement_is_within_the_documented_error_and_its_fp32_form_within_the_bar():
    x = vd.activation_grid(100)
    x64 = x.double().numpy()
    as64, true = vd.gelu_as(x64), vd.gelu_true(x).numpy()
    worst = float(np.max(np.abs(as64 - true) / np.maximum(np.abs(x64), 2.0 ** -126)))
    print("A&S 7.1.26 restatement against the true GELU: max |error| / |x| =", worst)
    assert worst <= vd.AS_GELU_ERR
    as32 = vd.gelu_as(x.numpy(), np.float32)
    check_range("gelu_as fp32 against its float64 restatement", {"all": vd.rho(torch.from_numpy(as32), torch.from_numpy(as64), x.double().abs())})


@pytest.mark.parametrize("geom", [(1, 1, 96, 35, 64), (1, 2, 64, 35, 32)])
def test_yardstick_attention(geom):
    B, heads, N, Nk, hd = geom
    table = {"out": {}, "dq": {}, "dkv": {}}
    for spread, late in ((1, False), (30, False), (100, False), (1, True)):
        q, kv, do = vd.attention_inputs(B, heads, N, Nk, hd, spread, late)
        got = vd.attention_logit_spread(q, kv, heads, hd ** -0.5)
        assert late or abs(got - spread) < 0.01 * spread, (got, spread)
        for k, (r, c, y) in vd.attention_case(q, kv, do, heads, hd ** -0.5).items():
            table[k][f"{spread}{'+late' if late else ''}"] = vd.rho(y, r, c)
    for k, v in table.items():
        check_range(f"attention {k} hd={hd}", v)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. known-wrong fp32 restatements: rho > 1000 in at least one regime, and the old bar on order-1 inputs passes them
# ------------------------------------------------------------------------------------------------------------------------------
def one_pass_norm(x, g, b, eps, dim):
    """variance as E[x^2] - mean^2"""
    m = x.mean(dim, keepdim=True)
    v = (x * x).mean(dim, keepdim=True) - m * m
    return (x - m) * torch.rsqrt(v.clamp_min(0.0) + eps) * g + b


def test_one_pass_variance_layernorm_is_rejected():
    C = 160
    g, b = vd.affine(C)
    x = rnd(333, C, seed=9, lo=-3, hi=5)
    assert old_err(one_pass_norm(x, g, b, 1e-6, -1), F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)) < OLD_TOL
    rhos = {}
    for regime in vd.REGIMES:
        x = vd.rows_regime(regime, ROWS, C, seed=C)
        ref, cond, _ = vd.layernorm_case(x, g, b, 1e-6)
        rhos[regime] = vd.rho(one_pass_norm(x, g, b, 1e-6, -1), ref, cond, finite=False)
    print("one-pass LayerNorm", rhos)
    assert rhos["scales"] < 8.0  # scale alone does not expose it ...
    assert rhos["offset"] > 1000 and rhos["both"] > 1000  # ... an offset does


def test_one_pass_variance_batchnorm_is_rejected():
    rows, C = 300, 32
    g, b = vd.batchnorm_affine(C)
    x = rnd(rows, C, seed=9, lo=-3, hi=5)
    ref = F.relu(F.batch_norm(x.double(), None, None, g.double(), b.double(), True, 0.0, 1e-5))
    assert old_err(F.relu(one_pass_norm(x, g, b, 1e-5, 0)), ref) < OLD_TOL
    x = vd.batchnorm_columns(rows, C)
    ref, cond, _, _, _ = vd.batchnorm_case(x, g, b, 1e-5)
    r = vd.rho(F.relu(one_pass_norm(x, g, b, 1e-5, 0)), ref, cond, finite=False)
    print("one-pass BatchNorm", r)
    assert r > 1000


def test_softmax_without_the_max_subtraction_is_rejected():
    def bare(x):
        e = torch.exp(x)
        return e / e.sum(-1, keepdim=True)

    x = rnd(333, 9, seed=22, lo=-3, hi=5)
    assert old_err(bare(x), torch.softmax(x.double(), -1)) < OLD_TOL
    x, which = vd.logit_rows(ROWS, 9, seed=9)
    p, cond, _ = vd.softmax_case(x)
    rhos = {si: vd.rho(bare(x[which == si]), p[which == si], cond[which == si], finite=False) for si in range(5)}
    print("softmax without max", rhos)
    assert max(rhos.values()) > 1000


def test_tanh_gelu_is_rejected():
    """Does NOT pass the old bar either when the tensor holds nothing but the activation (its worst error, 4.7e-4 near |x| = 2.6,
    is 9e-5 of max |ref| = 5); behind a depthwise conv's parameter gradients or at max |ref| of 10 and more it does."""
    x = rnd(333, 32, seed=13, lo=-3, hi=5)
    e = old_err(F.gelu(x, approximate="tanh"), F.gelu(x.double()))
    print("tanh GELU on the old bar", e)
    assert OLD_TOL < e < 4 * OLD_TOL
    r, c, _ = vd.gelu_case(vd.activation_grid())
    assert vd.rho(F.gelu(vd.activation_grid(), approximate="tanh"), r, c) > 1000
    ext = vd.activation_grid(100)
    dy = vd.cotangent((1, ext.numel()), seed=4)[0]
    r, c, _ = vd.act_bwd_case(F.gelu, ext, dy)
    xs = ext.clone().requires_grad_(True)
    F.gelu(xs, approximate="tanh").backward(dy)
    assert vd.rho(xs.grad, r, c) > 1000


def test_ce_as_minus_log_softmax_is_rejected():
    def naive(x, lab):
        valid = lab != 255
        return -torch.log(torch.softmax(x, -1)).gather(1, lab.clamp(0, x.shape[1] - 1)[:, None])[:, 0][valid].mean()

    x = rnd(391, 9, seed=22, lo=-3, hi=5)
    lab = ce_labels(391, 9)
    ref = float(F.cross_entropy(x.double(), lab, ignore_index=255))
    assert abs(float(naive(x, lab)) - ref) / abs(ref) < 1e-5  # test_softmax_ce_with_ignore's bar for the loss
    x, which = vd.logit_rows(ROWS, 9, seed=9)
    lab = ce_labels(ROWS, 9)
    rhos = {}
    for si in range(5):
        l2 = lab.clone()
        l2[which != si] = 255
        r, c, _ = vd.ce_case(x, l2)["loss"]
        rhos[si] = vd.rho(naive(x, l2), r, c, finite=False)
    print("CE as -log softmax", rhos)
    assert max(rhos.values()) > 1000


def test_measure_floor_and_cap():
    assert vd.TINY == 2.0 ** -126 and vd.U == 2.0 ** -24 and vd.F_CAP == 8.0
    assert vd.passes(7.9, 0.2, 8.0) and not vd.passes(8.1, 0.2, 8.0) and vd.passes(15.0, 2.0, 8.0)
    with pytest.raises(AssertionError):
        vd.passes(1.0, 1.0, 16.0)
    assert vd.rho(torch.tensor([math.inf]), torch.tensor([1.0]), torch.tensor([1.0]), finite=False) == math.inf
    with pytest.raises(AssertionError):
        vd.rho(torch.tensor([math.nan]), torch.tensor([1.0]), torch.tensor([1.0]))
