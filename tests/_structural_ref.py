"""float64 numpy restatement of Qabf, SSIM and the pixel-domain VIF for the tests, independent of segmif_amd: the windows are
the full N x N Gaussians normalised in float64, and "valid" / "same" filtering are sums over taps of shifted slices.  Qabf
and VIF have no external implementation to compare with: the formulas written out here are the specification."""
import functools

import numpy as np

from _fusion_ref import luma, make_inputs

SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.int64)
SOBEL_Y = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=np.int64)


def gaussian_window(n, sd):
    """(n, n) float64, exp(-(x^2 + y^2) / (2 sd^2)) about the centre, normalised to sum 1"""
    c = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    w = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2.0 * sd * sd))
    return w / w.sum()


def filter_valid(x, w):
    """out[y][x] = sum_ij w[i][j] x[y + i][x + j], (H - n + 1, W - n + 1); for the symmetric windows used here correlation
    and convolution agree"""
    n, m = w.shape
    H, W = x.shape
    out = np.zeros((H - n + 1, W - m + 1), dtype=np.result_type(x.dtype, w.dtype))
    for i in range(n):
        for j in range(m):
            out += w[i, j] * x[i:i + H - n + 1, j:j + W - m + 1]
    return out


def conv_same(x, k):
    """true convolution of the same size with zero padding: out[y][x] = sum_ij k[i][j] x[y + c - i][x + c - j], c the centre"""
    n = k.shape[0]
    return filter_valid(np.pad(x, n // 2), k[::-1, ::-1])


def qabf_sums(f, a, v):
    """-> (num, den) of one image from the integer planes"""
    def edges(x):
        sx, sy = conv_same(x, SOBEL_X), conv_same(x, SOBEL_Y)
        m2 = sx * sx + sy * sy
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(sx == 0, np.pi / 2, np.arctan(sy.astype(np.float64) / np.where(sx == 0, 1, sx)))
        return m2, np.sqrt(m2.astype(np.float64)), alpha

    m2f, gf, alf = edges(f)

    def q(x):
        m2s, gs, als = edges(x)
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.where(m2s > m2f, gf / np.where(gs == 0, 1, gs), np.where(m2s == m2f, gf, gs / np.where(gf == 0, 1, gf)))
        A = 1.0 - np.abs(als - alf) / (np.pi / 2)
        return 0.9994 / (1.0 + np.exp(-15.0 * (G - 0.5))) * 0.9879 / (1.0 + np.exp(-22.0 * (A - 0.8))), gs

    qa, ga = q(a)
    qv, gv = q(v)
    return float((qa * ga + qv * gv).sum()), float((ga + gv).sum())


def ssim_map(x, y):
    """pytorch_ssim's map of two integer planes taken as x / 255: 11 x 11 Gaussian, sigma 1.5, zero padding of 5"""
    w = gaussian_window(11, 1.5)
    x, y = x.astype(np.float64) / 255.0, y.astype(np.float64) / 255.0
    blur = lambda t: filter_valid(np.pad(t, 5), w)
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def vifp_sums(ref, dist):
    """-> (sums (4, 2) = [scale][num, den], variances: every sigma1^2 and sigma2^2 of every scale after the clip at 0)"""
    ref, dist = ref.astype(np.float64), dist.astype(np.float64)
    sums, variances = np.zeros((4, 2)), []
    for scale in range(1, 5):
        n = 2 ** (5 - scale) + 1
        w = gaussian_window(n, n / 5.0)
        if scale > 1:
            ref, dist = filter_valid(ref, w)[::2, ::2], filter_valid(dist, w)[::2, ::2]
        mu1, mu2 = filter_valid(ref, w), filter_valid(dist, w)
        s1 = np.maximum(filter_valid(ref * ref, w) - mu1 * mu1, 0.0)
        s2 = np.maximum(filter_valid(dist * dist, w) - mu2 * mu2, 0.0)
        s12 = filter_valid(ref * dist, w) - mu1 * mu2
        variances += [s1.ravel().copy(), s2.ravel().copy()]
        g = s12 / (s1 + 1e-10)
        sv = s2 - g * s12
        m = s1 < 1e-10
        g[m], sv[m], s1[m] = 0.0, s2[m], 0.0
        m = s2 < 1e-10
        g[m], sv[m] = 0.0, 0.0
        m = g < 0
        sv[m], g[m] = s2[m], 0.0
        sv[sv <= 1e-10] = 1e-10
        sums[scale - 1, 0] = np.log10(1.0 + g * g * s1 / (sv + 2.0)).sum()
        sums[scale - 1, 1] = np.log10(1.0 + s1 / 2.0).sum()
    return sums, np.concatenate(variances)


def _ratio(num, den):
    return float("nan") if den == 0 else num / den


def ref_structural(fused, vis, ir, vif=True):
    """fused, vis (B, H, W, 3) uint8, ir (B, H, W) uint8 -> dict of float64 arrays of length B (Qabf, SSIM, SSIM_ir, SSIM_vis and,
    with vif, VIF, VIF_ir, VIF_vis) and 'variances': every local variance the VIF branches look at, over the whole batch"""
    B = ir.shape[0]
    names = ("Qabf", "SSIM", "SSIM_ir", "SSIM_vis") + (("VIF", "VIF_ir", "VIF_vis") if vif else ())
    out = {k: np.empty(B) for k in names}
    variances = []
    for b in range(B):
        f, v, a = luma(fused[b]), luma(vis[b]), ir[b].astype(np.int64)
        out["Qabf"][b] = _ratio(*qabf_sums(f, a, v))
        out["SSIM_ir"][b], out["SSIM_vis"][b] = ssim_map(f, a).mean(), ssim_map(f, v).mean()
        out["SSIM"][b] = 0.5 * (out["SSIM_ir"][b] + out["SSIM_vis"][b])
        if vif:
            for name, src in (("VIF_ir", a), ("VIF_vis", v)):
                sums, var = vifp_sums(src, f)
                variances.append(var)
                out[name][b] = _ratio(sums[:, 0].sum(), sums[:, 1].sum())
            out["VIF"][b] = out["VIF_ir"][b] + out["VIF_vis"][b]
    out["variances"] = np.concatenate(variances) if variances else np.zeros(0)
    return out


@functools.lru_cache(maxsize=None)
def cached_case(kind, B, H, W, seed=0):
    """(inputs, reference) of one seeded case, computed once and shared by the tests; nobody writes to the arrays.  VIF is left
    out for all255 (undefined: see structural_scores)."""
    inputs = make_inputs(kind, B, H, W, seed=seed)
    ref = ref_structural(*inputs, vif=kind != "all255")
    for arr in inputs + tuple(ref.values()):
        arr.setflags(write=False)
    return inputs, ref
