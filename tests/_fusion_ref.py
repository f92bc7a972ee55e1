"""numpy restatement of the fusion statistics and scores for the tests (independent of segmif_amd: the luma, the
histograms and every definition are written out here), and the seeded uint8 test images."""
import numpy as np

SCORES = ("EN", "MI", "SD", "SF", "AG", "CC", "PSNR", "SCD")


def luma(rgb):
    """(..., 3) uint8 -> int64, L = (299 R + 587 G + 114 B + 500) // 1000"""
    c = rgb.astype(np.int64)
    return (299 * c[..., 0] + 587 * c[..., 1] + 114 * c[..., 2] + 500) // 1000


def ref_stats(fused, vis, ir):
    """fused, vis (B, H, W, 3) uint8, ir (B, H, W) uint8 -> joint_fa, joint_fv (B, 256, 256) int64, sums (B, 4) int64, ag (B,) float64"""
    B, H, W = ir.shape
    f, v, a = luma(fused), luma(vis), ir.astype(np.int64)
    jfa = np.stack([np.bincount((f[b] * 256 + a[b]).ravel(), minlength=65536).reshape(256, 256) for b in range(B)]).astype(np.int64)
    jfv = np.stack([np.bincount((f[b] * 256 + v[b]).ravel(), minlength=65536).reshape(256, 256) for b in range(B)]).astype(np.int64)
    sums = np.empty((B, 4), dtype=np.int64)
    sums[:, 0] = (a * v).sum(axis=(1, 2))
    sums[:, 1] = ((f[:, :, 1:] - f[:, :, :-1]) ** 2).sum(axis=(1, 2))
    sums[:, 2] = ((f[:, 1:, :] - f[:, :-1, :]) ** 2).sum(axis=(1, 2))
    sums[:, 3] = H * W
    dx = (f[:, :-1, 1:] - f[:, :-1, :-1]).astype(np.float64)
    dy = (f[:, 1:, :-1] - f[:, :-1, :-1]).astype(np.float64)
    ag = np.sqrt((dx * dx + dy * dy) / 2.0).sum(axis=(1, 2))
    return jfa, jfv, sums, ag


def _entropy(x):
    p = np.bincount(x.ravel(), minlength=256).astype(np.float64) / x.size
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def _mi(x, y):
    p = np.bincount((x * 256 + y).ravel(), minlength=65536).reshape(256, 256).astype(np.float64) / x.size
    px, py = p.sum(axis=1, keepdims=True), p.sum(axis=0, keepdims=True)
    nz = p > 0
    return float((p[nz] * np.log2(p[nz] / (px * py)[nz])).sum())


def _r(x, y):
    """Pearson correlation of two integer images; NaN when one of them is constant"""
    if x.min() == x.max() or y.min() == y.max():
        return float("nan")
    xc, yc = x.astype(np.float64) - x.mean(), y.astype(np.float64) - y.mean()
    return float((xc * yc).sum() / np.sqrt((xc * xc).sum() * (yc * yc).sum()))


def ref_scores(fused, vis, ir):
    """The eight scores per image, float64, straight from the definitions on the pixels."""
    B, H, W = ir.shape
    out = {k: np.empty(B) for k in SCORES}
    for b in range(B):
        f, v, a = luma(fused[b]), luma(vis[b]), ir[b].astype(np.int64)
        fd = f.astype(np.float64)
        out["EN"][b] = _entropy(f)
        out["MI"][b] = _mi(f, a) + _mi(f, v)
        out["SD"][b] = np.sqrt(((fd - fd.mean()) ** 2).sum() / (H * W))
        rf2 = ((fd[:, 1:] - fd[:, :-1]) ** 2).sum() / (H * W)
        cf2 = ((fd[1:, :] - fd[:-1, :]) ** 2).sum() / (H * W)
        out["SF"][b] = np.sqrt(rf2 + cf2)
        dx, dy = fd[:-1, 1:] - fd[:-1, :-1], fd[1:, :-1] - fd[:-1, :-1]
        out["AG"][b] = np.sqrt((dx * dx + dy * dy) / 2.0).sum() / ((H - 1) * (W - 1))
        out["CC"][b] = (_r(f, a) + _r(f, v)) / 2
        mse = (((f - a) ** 2).sum() / (H * W) + ((f - v) ** 2).sum() / (H * W)) / 2
        out["PSNR"][b] = 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0 else np.inf
        out["SCD"][b] = _r(f - v, a) + _r(f - a, v)
    return out


KINDS = ("smooth", "noise", "all255", "all0", "vramp", "hramp")


def _smooth_field(rng, B, H, W):
    """a random low-resolution field enlarged by repetition and blurred once along each axis: neighbouring pixels are close"""
    ch, cw = max(1, (H + 7) // 8), max(1, (W + 7) // 8)
    coarse = rng.uniform(20, 235, (B, ch, cw))
    fine = np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :H, :W]
    fine = (fine + np.roll(fine, 1, axis=1) + np.roll(fine, 2, axis=1) + np.roll(fine, 3, axis=1)) / 4
    return (fine + np.roll(fine, 1, axis=2) + np.roll(fine, 2, axis=2) + np.roll(fine, 3, axis=2)) / 4


def make_inputs(kind, B, H, W, seed=0):
    """-> fused (B, H, W, 3), vis (B, H, W, 3), ir (B, H, W) uint8.  smooth: one smooth field under all three images plus a
    little noise - the joint histograms hug the diagonal (the collision-heavy case); noise: independent uniform bytes."""
    rng = np.random.default_rng([seed, B, H, W, KINDS.index(kind)])
    u8 = lambda x: np.clip(np.rint(x), 0, 255).astype(np.uint8)
    if kind == "smooth":
        base = _smooth_field(rng, B, H, W)
        ir = u8(base + rng.normal(0, 2, (B, H, W)))
        vis = u8(base[..., None] + rng.normal(0, 2, (B, H, W, 3)))
        fused = u8(base[..., None] + rng.normal(0, 1.5, (B, H, W, 3)))
    elif kind == "noise":
        ir = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        vis = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        fused = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    elif kind in ("all255", "all0"):
        c = 255 if kind == "all255" else 0
        ir, vis, fused = (np.full(s, c, dtype=np.uint8) for s in ((B, H, W), (B, H, W, 3), (B, H, W, 3)))
    else:
        if kind == "vramp":
            ramp = np.broadcast_to((np.arange(H) * 255 // (H - 1))[None, :, None], (B, H, W))
        else:
            ramp = np.broadcast_to((np.arange(W) * 255 // (W - 1))[None, None, :], (B, H, W))
        ir = u8(ramp)
        fused = np.repeat(ir[..., None], 3, axis=3)
        vis = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return np.ascontiguousarray(fused), np.ascontiguousarray(vis), np.ascontiguousarray(ir)
