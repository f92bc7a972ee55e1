"""Value-domain inputs, float64 references, conditioning terms and fp32 yardsticks for the fp32 row kernels (LayerNorm, BatchNorm,
softmax / cross-entropy, GELU / SiLU, attention).  torch / numpy only: tests/test_value_domain_host.py proves the measure on the
CPU, tests/test_gpu_value_domain.py holds the HIP kernels to it.

The measure.  u = 2^-24 (fp32's rounding unit) and

    rho(got, ref, cond) = max |got - ref| / (u * cond + tiny)

tiny = 2^-126, fp32's smallest normal number: below it a result may be flushed to zero or keep only a few bits (a probability of
1e-40 is as good as 0), and no cond term can speak for that.  ref is float64 aten on the CPU; cond is the operation's own formula
with absolute values on every term (the `yard` tensors of test_gpu_round5.py, per element): an evaluation that rounds every
intermediate once lands at rho of a few, whatever the scale or the offset of its input; one that cancels where the formula does
not (a one-pass variance, a softmax without its maximum) lands at 1e3 .. 1e12.  The yardstick of a case is the same operation
evaluated by torch in fp32 on the CPU on the same input; a kernel passes with rho_kernel <= F * max(rho_yardstick, 1).

Every generator draws from a seeded torch.Generator in float64 and casts to fp32 once, at the end.  All inputs are finite."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
F_CAP = 8.0  # no family's F may exceed this (the bug classes hunted here show ratios of 1e3 and more)


def rho(got, ref, cond, finite=True):
    """finite=False: a non-finite output is rho = inf instead of an assertion (the known-wrong restatements of the host test)"""
    got = torch.as_tensor(got).detach().double().cpu()
    ref, cond = torch.as_tensor(ref).detach().double(), torch.as_tensor(cond).detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        assert not finite, "non-finite output"
        return math.inf
    cond = cond.expand_as(ref) if cond.shape != ref.shape else cond
    if ref.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (U * cond + TINY)).max())


def passes(r_kernel, r_yard, factor):
    assert factor <= F_CAP
    return r_kernel <= factor * max(r_yard, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# input regimes
# ------------------------------------------------------------------------------------------------------------------------------
REGIMES = ("scales", "offset", "both", "zero")
OFFSETS = (0.0, 64.0, -64.0, 1024.0, 4096.0, -4096.0)
SPREADS = (1.0, 2.0 ** -6)


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def uniform(g, *shape):
    """float64, uniform in [-1, 1)"""
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2.0 - 1.0


def row_exponents(g, rows):
    """one integer in [-20, 20] per row; both ends are always present"""
    e = torch.randint(-20, 21, (rows,), generator=g).double()
    e[0] = -20.0
    e[1 % rows] = 20.0
    return e


def rows_regime(regime, rows, C, seed=0):
    """(rows, C) fp32.  scales: U 2^e_r; offset: m_r + s_r U with m_r cycling through OFFSETS and s_r through SPREADS (every pair
    occurs within 12 rows); both: the offset values times 2^e_r; zero: U with rows 0, rows / 2 and rows - 1 all zero."""
    g = gen(seed)
    u = uniform(g, rows, C)
    r = torch.arange(rows)
    m = torch.tensor(OFFSETS, dtype=torch.float64)[r % len(OFFSETS)][:, None]
    s = torch.tensor(SPREADS, dtype=torch.float64)[(r // len(OFFSETS)) % len(SPREADS)][:, None]
    e = row_exponents(g, rows)[:, None]
    if regime == "scales":
        x = u * 2.0 ** e
    elif regime == "offset":
        x = m + s * u
    elif regime == "both":
        x = (m + s * u) * 2.0 ** e
    elif regime == "zero":
        x = u.clone()
        x[[0, rows // 2, rows - 1]] = 0.0
    else:
        raise ValueError(regime)
    return x.float()


def affine(C, seed=0):
    """gamma in [0.5, 1.5), beta in [-1, 1)"""
    g = gen(1000 + seed)
    return (1.0 + 0.5 * uniform(g, C)).float(), uniform(g, C).float()


def cotangent(shape, seed=0):
    """uniform [-1, 1) with every 7th row a factor 2^10 up and every 11th a factor 2^-10 down"""
    g = gen(2000 + seed)
    dy = uniform(g, *shape)
    flat = dy.view(-1, shape[-1])
    flat[::7] *= 2.0 ** 10
    flat[::11] *= 2.0 ** -10
    return dy.float()


LOGIT_OFFSETS = (0.0, 1024.0, -16384.0)
LOGIT_SPREADS = (2.0 ** -8, 1.0, 16.0, 128.0, 1024.0)
N_EQUAL = len(LOGIT_OFFSETS)  # rows 0 .. N_EQUAL - 1 of logit_rows hold C equal values; row N_EQUAL has one dominant class


def logit_rows(rows, C, seed=0):
    """(rows, C) fp32 logits off + spread U.  Rows 0 .. 2: C equal values (one row per offset); row 3: a single dominant class;
    the others cycle through the 15 (off, spread) pairs.  -> (x, spread_index (rows,), -1 for the four special rows)."""
    assert rows >= N_EQUAL + 1 + len(LOGIT_OFFSETS) * len(LOGIT_SPREADS)
    g = gen(3000 + seed)
    u = uniform(g, rows, C)
    x = torch.empty(rows, C, dtype=torch.float64)
    which = torch.full((rows,), -1, dtype=torch.long)
    for i, off in enumerate(LOGIT_OFFSETS):
        x[i] = off if off else 0.7109375
    x[N_EQUAL] = u[N_EQUAL]
    x[N_EQUAL, C // 2] = 60.0
    for r in range(N_EQUAL + 1, rows):
        k = r - N_EQUAL - 1
        si = k % len(LOGIT_SPREADS)
        x[r] = LOGIT_OFFSETS[(k // len(LOGIT_SPREADS)) % len(LOGIT_OFFSETS)] + LOGIT_SPREADS[si] * u[r]
        which[r] = si
    return x.float(), which


def activation_grid(extend=None):
    """pre-activations: [-9, 9] in steps of 1/64 plus +-2^k, k = -30 .. 4 (extend: also +-extend and steps of 1 out to it)"""
    dense = torch.arange(-9 * 64, 9 * 64 + 1, dtype=torch.float64) / 64.0
    pw = 2.0 ** torch.arange(-30, 5, dtype=torch.float64)
    parts = [dense, pw, -pw]
    if extend:
        far = torch.arange(10, int(extend) + 1, dtype=torch.float64)
        parts += [far, -far]
    return torch.cat(parts).float()


def grid_filled(shape, extend=None, seed=0):
    """the grid repeated (in a seeded random order) to fill `shape`"""
    gr = activation_grid(extend)
    n = math.prod(shape)
    idx = torch.cat([torch.randperm(gr.numel(), generator=gen(4000 + seed + i)) for i in range((n + gr.numel() - 1) // gr.numel())])
    return gr[idx[:n]].view(*shape).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm (rows) and BatchNorm (columns)
# ------------------------------------------------------------------------------------------------------------------------------
def norm_cond(z, ref, gamma, beta, eps, dim, zabs=None):
    """|gamma_c| rstd_r max_c |z_rc| + |y_rc - beta_c| + |beta_c|: the first term is what one rounding of z (or of the mean) is
    worth after the division by the spread, the others are the roundings of the affine tail.  zabs: the absolute-value form of
    z where z is itself computed (a GEMM / residual add in front of the normalisation), |z| otherwise.  dim = -1: LayerNorm,
    dim = 0: BatchNorm (statistics per column)."""
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    zabs = z.abs() if zabs is None else zabs.double()
    rstd = torch.rsqrt(z.var(dim, unbiased=False, keepdim=True) + eps)
    return gamma.abs() * rstd * zabs.amax(dim, keepdim=True) + (ref - beta).abs() + beta.abs()


def layernorm_case(x, gamma, beta, eps, zabs=None):
    """-> ref (float64), cond, yardstick (torch fp32) of F.layer_norm over the last dim"""
    C = x.shape[-1]
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps)
    return ref, norm_cond(x, ref, gamma, beta, eps, -1, zabs), F.layer_norm(x.float(), (C,), gamma, beta, eps)


def _norm_bwd_conds(x, gamma, dy, eps, dim, zabs=None):
    """Conditioning of the normalisation's backward, g = dy gamma, mean over `dim`:
        dx = rstd (g - mean g - xhat mean(g xhat)),  dgamma = sum dy xhat,  dbeta = sum dy      (sums over the other dim)
    Absolute-value form A = rstd (|g| + mean |g| + |xhat| mean |g xhat|).  On top of it xhat and rstd are themselves computed:
    one rounding of x (or of the mean) moves xhat by u K, K = rstd max |x|, and rstd by a relative u K, hence
        cond_dx = (1 + K) A + rstd K (mean |g xhat| + |xhat| mean |g|)   and   cond_dgamma = sum |dy| (|xhat| + K)."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    mu = x.mean(dim, keepdim=True)
    rstd = torch.rsqrt(x.var(dim, unbiased=False, keepdim=True) + eps)
    xh = (x - mu) * rstd
    K = rstd * (x.abs() if zabs is None else zabs.double()).amax(dim, keepdim=True)
    g = (dy * gamma).abs()
    mg, mgx = g.mean(dim, keepdim=True), (g * xh.abs()).mean(dim, keepdim=True)
    A = rstd * (g + mg + xh.abs() * mgx)
    return ((1.0 + K) * A + rstd * K * (mgx + xh.abs() * mg), (dy.abs() * (xh.abs() + K)).sum(0), dy.abs().sum(0))


def layernorm_bwd_case(x, gamma, beta, dy, eps):
    """-> {name: (ref, cond, yard)} for dx, dgamma, dbeta of F.layer_norm (rows = every dim but the last)"""
    C = x.shape[-1]

    def run(dt):
        xs, gs, bs = (t.detach().to(dt).requires_grad_(True) for t in (x, gamma, beta))
        F.layer_norm(xs, (C,), gs, bs, eps).backward(dy.to(dt))
        return xs.grad, gs.grad, bs.grad

    ref, yard = run(torch.float64), run(torch.float32)
    x2, dy2 = x.reshape(-1, C), dy.reshape(-1, C)
    cdx, cdg, cdb = _norm_bwd_conds(x2, gamma, dy2, eps, -1)
    return {"dx": (ref[0], cdx.view(x.shape), yard[0]), "dgamma": (ref[1], cdg, yard[1]), "dbeta": (ref[2], cdb, yard[2])}


def add_layernorm_case(x, br, sc, gamma, beta, ds, dn, eps):
    """(s, n) = (x + sc[b] br, LayerNorm(s)) over tokens (B, N, C) with cotangents (ds, dn).  The sum is computed in front of the
    normalisation, so its absolute-value form |x| + |sc br| takes |s|'s place in K; dx = ds + LN'(dn) adds |ds|, and
    dbranch = sc dx scales all of it.  -> {s, n, dx, dbranch, dgamma, dbeta: (ref, cond, yard)}"""
    C = x.shape[-1]

    def run(dt):
        xs, bs_, gs, bt = (t.detach().to(dt).requires_grad_(True) for t in (x, br, gamma, beta))
        s = xs + sc.to(dt).view(-1, 1, 1) * bs_
        n = F.layer_norm(s, (C,), gs, bt, eps)
        torch.autograd.backward([s, n], [ds.to(dt), dn.to(dt)])
        return s.detach(), n.detach(), xs.grad, bs_.grad, gs.grad, bt.grad

    ref, yard = run(torch.float64), run(torch.float32)
    scd = sc.double().view(-1, 1, 1)
    zabs = x.double().abs() + (scd * br.double()).abs()
    cn = norm_cond(ref[0], ref[1], gamma, beta, eps, -1, zabs)
    cdx, cdg, cdb = _norm_bwd_conds(ref[0].reshape(-1, C), gamma, dn.reshape(-1, C), eps, -1, zabs.reshape(-1, C))
    cdx = cdx.view(x.shape) + ds.double().abs()
    conds = (zabs, cn, cdx, scd.abs() * cdx, cdg, cdb)
    return {k: (ref[i], conds[i], yard[i]) for i, k in enumerate(("s", "n", "dx", "dbranch", "dgamma", "dbeta"))}


def epilogue_layernorm_case(z64, zabs, z32, gamma, beta, eps):
    """LayerNorm in a GEMM's / conv's epilogue: z64 the float64 pre-normalisation values, zabs their absolute-value form
    (|x| |w|^T + |bias|), z32 torch's fp32 evaluation of the same GEMM / conv.  -> ref, cond, yard"""
    C = z64.shape[-1]
    ref = F.layer_norm(z64, (C,), gamma.double(), beta.double(), eps)
    return ref, norm_cond(z64, ref, gamma, beta, eps, -1, zabs), F.layer_norm(z32, (C,), gamma, beta, eps)


def batchnorm_columns(rows, C, seed=0):
    """(rows, C) fp32 whose COLUMNS come from scales, offset and both (a third of the columns each)"""
    n = [C // 3, C // 3, C - 2 * (C // 3)]
    return torch.cat([rows_regime(r, k, rows, seed + i) for i, (r, k) in enumerate(zip(("scales", "offset", "both"), n))]).t().contiguous()


def batchnorm_affine(C, seed=0):
    """gamma in [0.5, 1.5); beta cycles through -2.5, -0.5, 0.5, 2.5 (+ U / 4): columns that the ReLU cuts entirely, partly, and
    not at all."""
    g = gen(1100 + seed)
    gamma = 1.0 + 0.5 * uniform(g, C)
    beta = torch.tensor([-2.5, -0.5, 0.5, 2.5], dtype=torch.float64)[torch.arange(C) % 4] + 0.25 * uniform(g, C)
    return gamma.float(), beta.float()


def batchnorm_case(x, gamma, beta, eps):
    """train-mode BatchNorm + ReLU over (rows, C).  -> ref y, cond, yard y, pre-activation z (float64), mask-flip candidates:
    the elements whose float64 pre-activation lies within 16 u cond of zero (a correctly rounded kernel may put those on the
    other side of the ReLU; nothing else)."""
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    z = F.batch_norm(xd, None, None, gd, bd, True, 0.0, eps)
    cond = norm_cond(xd, z, gd, bd, eps, 0)
    yard = F.relu(F.batch_norm(x.float(), None, None, gamma, beta, True, 0.0, eps))
    return F.relu(z), cond, yard, z, z.abs() <= 16.0 * U * cond


def batchnorm_stats_case(x):
    """batch mean and biased variance per column.  mean: cond mean |x|.  var = mean d^2, d = x - mean, in two passes: an error e
    of the mean cancels to first order (sum d = 0) and shifts the variance by e^2; a mean held in fp32 has e <= u max |x|, i.e.
    u max |x|^2 in units of u; the differences, squares and their sum add a few u var: cond = 4 var + u max |x|^2.
    (A one-pass variance is off by u mean^2: 1 / u times the second term.)  -> {mean, var: (ref, cond, yard)}"""
    xd = x.double()
    mu, var = xd.mean(0), xd.var(0, unbiased=False)
    cvar = 4.0 * var + U * xd.abs().amax(0) ** 2
    return {"mean": (mu, xd.abs().mean(0), x.float().mean(0)), "var": (var, cvar, x.float().var(0, unbiased=False))}


def batchnorm_bwd_case(x, gamma, beta, dy, eps):
    """dy must already be zero on the mask-flip candidates.  -> {name: (ref, cond, yard)} for dx, dgamma, dbeta"""
    def run(dt):
        xs, gs, bs = (t.detach().to(dt).requires_grad_(True) for t in (x, gamma, beta))
        F.relu(F.batch_norm(xs, None, None, gs, bs, True, 0.0, eps)).backward(dy.to(dt))
        return xs.grad, gs.grad, bs.grad

    ref, yard = run(torch.float64), run(torch.float32)
    z = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, eps)
    dz = dy.double() * (z > 0)
    cdx, cdg, cdb = _norm_bwd_conds(x, gamma, dz, eps, 0)
    return {"dx": (ref[0], cdx, yard[0]), "dgamma": (ref[1], cdg, yard[1]), "dbeta": (ref[2], cdb, yard[2])}


# ------------------------------------------------------------------------------------------------------------------------------
# softmax family
# ------------------------------------------------------------------------------------------------------------------------------
def f32(v):
    """the fp32 value a C float parameter takes"""
    return float(np.float32(v))


def is_pow2(s):
    return math.frexp(abs(s))[0] == 0.5


def softmax_case(x, scale=1.0):
    """p = softmax(s x) over the last dim, s the fp32 value of scale.  cond_j = p_j (4 + |s x_j - m| + [s not 2^k] (|s x_j| + |m|)):
    exp turns an absolute error of its argument into a relative one of p_j; s x_j - m is exact up to its own rounding when s is a
    power of two, and carries the roundings of both products otherwise; 4 = exp, the sum, the division, the store.
    -> ref, cond, yard"""
    s = f32(scale)
    z = s * x.double()
    m = z.amax(-1, keepdim=True)
    p = torch.softmax(z, -1)
    cond = p * (4.0 + (z - m).abs() + (0.0 if is_pow2(s) else (z.abs() + m.abs())))
    return p, cond, torch.softmax(x.float() * torch.tensor(s, dtype=torch.float32), -1)


def softmax_bwd_case(p, dp, scale):
    """ds = p (dp - sum p dp) s from the fp32 probabilities p and cotangent dp; absolute-value form |s| p (|dp| + sum p |dp|)."""
    s = f32(scale)
    pd, dd = p.double(), dp.double()
    ref = pd * (dd - (pd * dd).sum(-1, keepdim=True)) * s
    cond = abs(s) * pd * (dd.abs() + (pd * dd.abs()).sum(-1, keepdim=True))
    s32 = torch.tensor(s, dtype=torch.float32)
    return ref, cond, p * (dp - (p * dp).sum(-1, keepdim=True)) * s32


def ce_case(x, labels, ignore_index=255):
    """mean cross-entropy over the non-ignored rows of (rows, C) logits.  Per row the loss log sum exp(x - m) + m - x_label has
    cond 4 + |x_label - m| + log C (the sum is at most C, the difference m - x_label is exact up to its rounding); the mean's cond
    is the mean of the rows' conds.  Gradient (softmax - onehot) / count: the softmax term plus u plus the one-hot itself, over the
    count (p - 1 at the label is rounded at its own size, which is 1 and not p when the label's class is improbable: without
    the one-hot term torch's own fp32 cross-entropy reads rho = 2.9e6 on the dominant-class row).
    -> {loss: (ref, cond, yard), grad: (ref, cond, yard)}"""
    C = x.shape[-1]
    valid = labels != ignore_index
    n = int(valid.sum())

    def run(dt):
        xs = x.detach().to(dt).requires_grad_(True)
        loss = F.cross_entropy(xs, labels, ignore_index=ignore_index)
        loss.backward()
        return loss.detach(), xs.grad

    ref, yard = run(torch.float64), run(torch.float32)
    xd = x.double()
    m = xd.amax(-1)
    xl = xd.gather(1, labels.clamp(0, C - 1)[:, None])[:, 0]
    closs = ((4.0 + (xl - m).abs() + math.log(C)) * valid).sum() / n
    _, cp, _ = softmax_case(x)
    cgrad = (cp + U + F.one_hot(labels.clamp(0, C - 1), C)) * valid[:, None] / n
    return {"loss": (ref[0], closs, yard[0]), "grad": (ref[1], cgrad, yard[1])}


# ------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------
def gelu_case(x):
    """erf GELU: cond |x|"""
    return F.gelu(x.double()), x.double().abs(), F.gelu(x.float())


def silu_case(x):
    return F.silu(x.double()), x.double().abs(), F.silu(x.float())


def silu_fast_exp_extra(x):
    """The extra conditioning of silu(z) = z / (1 + e(-z)) when e is the hardware exponential, exp2(-z log2 e) (HIP's __expf).
    Its published error is 2 + floor(|1.173 z|) ulp = 2 u (2 + 1.173 |z|) relative (the product z log2 e is rounded before it
    reaches exp2, which turns that rounding into a relative error proportional to |z|).  A relative error r of e(-z) moves
    silu by silu * r * e(-z) / (1 + e(-z)) = |silu(z)| (1 - sigmoid(z)) r.  In units of u:"""
    xd = x.double()
    return F.silu(xd).abs() * (1.0 - torch.sigmoid(xd)) * 2.0 * (2.0 + 1.173 * xd.abs())


def act_bwd_case(fn, x, dy):
    """dx = dy fn'(x): cond |dy| (1 + |x|)"""
    def run(dt):
        xs = x.detach().to(dt).requires_grad_(True)
        fn(xs).backward(dy.to(dt))
        return xs.grad

    return run(torch.float64), dy.double().abs() * (1.0 + x.double().abs()), run(torch.float32)


AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_GELU_ERR = 7.5e-8  # csrc/split_ops.h: |erf error| <= 1.5e-7 (A&S 7.1.26), i.e. <= 7.5e-8 |x| on GELU


def gelu_as(x, dtype=np.float64):
    """GELU(x) = x Phi(x) with erfc(z), z = |x| / sqrt 2, by Abramowitz & Stegun 7.1.26:
    erfc(z) ~ (a1 t + .. + a5 t^5) exp(-z^2), t = 1 / (1 + p z); Phi = x >= 0 ? 1 - erfc / 2 : erfc / 2.
    dtype float64: the restatement gelu_as kernels are held to; float32: the same formula rounded at every step (their yardstick)."""
    x = np.asarray(x, dtype=dtype)
    one, half = dtype(1.0), dtype(0.5)
    ax = np.abs(x)
    t = one / (one + ax * dtype(AS_P) * dtype(math.sqrt(0.5)))
    q = dtype(AS_A[4])
    for a in AS_A[3::-1]:
        q = q * t + dtype(a)
    e = np.exp(-(x * x) * half)
    half_erfc = half * q * t * e
    phi = np.where(x >= 0, one - half_erfc, half_erfc)
    out = x * phi
    assert out.dtype == dtype
    return out


def gelu_true(x):
    """x Phi(x) through erfc: accurate in the negative tail (float64)"""
    xd = x.double()
    return 0.5 * xd * torch.special.erfc(-xd * math.sqrt(0.5))


PAIRS_EXTRA_REL, PAIRS_EXTRA_ABS = 4.0, 2.0 ** -12


def pairs_extra(y):
    """A PAIRS tensor stores y as two halves, y = hi + 2^-11 lo (csrc/gemm_pairs.hip): 22 significant bits, so a relative 2^-22 =
    4 u, and lo's half-denormal step 2^-24 * 2^-11 = 2^-35, so an absolute 2^-36 = 2^-12 u at most."""
    return PAIRS_EXTRA_REL * y.double().abs() + PAIRS_EXTRA_ABS


# ------------------------------------------------------------------------------------------------------------------------------
# attention: out = softmax(scale q k^T) v per (batch, head)
# ------------------------------------------------------------------------------------------------------------------------------
def _heads(q, kv, heads):
    B, N, C = q.shape
    Nk, hd = kv.shape[1], C // heads
    qh = q.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    kvh = kv.reshape(B, Nk, 2, heads, hd)
    return qh, kvh[:, :, 0].permute(0, 2, 1, 3), kvh[:, :, 1].permute(0, 2, 1, 3)


def _unheads(t):  # (B, heads, N, hd) -> (B, N, C)
    B, h, N, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, h * hd)


def _kv_of(k, v):  # (B, heads, Nk, hd) x 2 -> (B, Nk, 2C)
    return torch.cat([_unheads(k), _unheads(v)], dim=-1)


def attention_logit_spread(q, kv, heads, scale):
    """mean over the query rows of max_j - min_j of scale q k_j (float64)"""
    qh, k, _ = _heads(q.double(), kv.double(), heads)
    s = qh @ k.transpose(-2, -1) * f32(scale)
    return float((s.amax(-1) - s.amin(-1)).mean())


def attention_case(q, kv, do, heads, scale):
    """-> {out, dq, dkv: (ref, cond, yard)}.  Absolute-value forms, every one in units of u:
      logits  s = scale q k^T           A = |scale| |q| |k|^T                     (A >= |s|)
      probs   p = softmax(s)            cp = p (4 + |s - m| + A + sum_k p_k A_k)   (dp_j = p_j (ds_j - sum_k p_k ds_k))
      out     o = p v                   cp |v| + p |v|
      dP = dO v^T                       cdP = |dO| |v|^T
      D  = sum_j p dP (= dO . o)        cD = sum_j (p cdP + cp |dP|) + sum_j p |dP|
      dS = scale p (dP - D)             cdS = |scale| (cp (|dP| + |D|) + p (cdP + cD) + p (|dP| + sum_j p |dP|))
      dq = dS k, dk = dS^T q            cdS |k| + |dS| |k|,   cdS^T |q| + |dS|^T |q|
      dv = p^T dO                       cp^T |dO| + p^T |dO|"""
    sc = f32(scale)

    def run(dt):
        qs, kvs = q.detach().to(dt).requires_grad_(True), kv.detach().to(dt).requires_grad_(True)
        qh, k, v = _heads(qs, kvs, heads)
        out = _unheads(torch.softmax(qh @ k.transpose(-2, -1) * torch.tensor(sc, dtype=dt), -1) @ v)
        out.backward(do.to(dt))
        return out.detach(), qs.grad, kvs.grad

    ref, yard = run(torch.float64), run(torch.float32)
    qh, k, v = _heads(q.double(), kv.double(), heads)
    doh = _heads(do.double(), kv.double(), heads)[0]
    s = qh @ k.transpose(-2, -1) * sc
    A = abs(sc) * (qh.abs() @ k.abs().transpose(-2, -1))
    p = torch.softmax(s, -1)
    cp = p * (4.0 + (s - s.amax(-1, keepdim=True)).abs() + A + (p * A).sum(-1, keepdim=True))
    c_out = cp @ v.abs() + p @ v.abs()
    dP = doh @ v.transpose(-2, -1)
    cdP = doh.abs() @ v.abs().transpose(-2, -1)
    pdP = (p * dP.abs()).sum(-1, keepdim=True)
    D = (p * dP).sum(-1, keepdim=True)
    cD = (p * cdP + cp * dP.abs()).sum(-1, keepdim=True) + pdP
    dS = sc * p * (dP - D)
    cdS = abs(sc) * (cp * (dP.abs() + D.abs()) + p * (cdP + cD) + p * (dP.abs() + pdP))
    c_dq = cdS @ k.abs() + dS.abs() @ k.abs()
    c_dk = cdS.transpose(-2, -1) @ qh.abs() + dS.abs().transpose(-2, -1) @ qh.abs()
    c_dv = cp.transpose(-2, -1) @ doh.abs() + p.transpose(-2, -1) @ doh.abs()
    return {"out": (ref[0], _unheads(c_out), yard[0]), "dq": (ref[1], _unheads(c_dq), yard[1]),
            "dkv": (ref[2], _kv_of(c_dk, c_dv), yard[2])}


def attention_inputs(B, heads, N, Nk, hd, spread, late_key=False, seed=0):
    """q, kv, do (fp32) with q scaled so that the mean logit spread (max - min over the keys, scale hd^-1/2) is `spread`;
    late_key: key Nk - 3 is 40 x query row 5 of head 0 (that row's maximum jumps in the last key tile)."""
    g = gen(5000 + seed)
    C = heads * hd
    q, kv, do = uniform(g, B, N, C), uniform(g, B, Nk, 2 * C), uniform(g, B, N, C)
    if late_key:
        kv[:, Nk - 3, :hd] = 40.0 * q[0, 5, :hd]
    q = q * (spread / attention_logit_spread(q.float(), kv.float(), heads, hd ** -0.5))
    return q.float(), kv.float(), do.float()
