"""A float64 numpy restatement of include/segmif_calib.h's rule, written from the rule, and the seeded cases the GPU tests run
(tests/test_gpu_calibration.py) and the host tests vet (tests/test_calibration_host.py).  The coordinates and the reciprocal
temperature are float32 as the rule states them (numpy forms them without fused multiply-adds); everything after is float64."""
import numpy as np

F32 = np.float32
THRESHOLDS8 = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.968, 0.99)
T16 = (1.0,) + tuple(float(v) for v in np.exp(np.linspace(np.log(0.5), np.log(4.0), 15)))
ODD_LABELS = (255, -1, 256, 2 ** 40 + 3)


def _axis(I, O):
    s = F32(I) / F32(O)
    f = np.maximum(s * (np.arange(O, dtype=F32) + F32(0.5)) - F32(0.5), F32(0))
    i0 = np.minimum(f.astype(np.int32), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    l = f - i0.astype(F32)
    return i0, i1, l.astype(np.float64), (F32(1) - l).astype(np.float64)


def interp(x, OH, OW):
    """x (B, IH, IW, C) -> v (B, OH, OW, C) float64: hy (hx p00 + lx p01) + ly (hx p10 + lx p11)"""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly, hy = _axis(x.shape[1], OH)
    x0, x1, lx, hx = _axis(x.shape[2], OW)
    lx, hx, ly, hy = lx[None, None, :, None], hx[None, None, :, None], ly[None, :, None, None], hy[None, :, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = hx * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
        bot = hx * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
        return hy * top + ly * bot


def pixels(x, label, OH, OW, temperatures):
    """-> dict of per-pixel float64 values: valid / ignored / nonfinite (B, OH, OW) bool, pred, correct, gap (the top-2 gap, inf for
    C = 1), conf / nll / brier (NT, B, OH, OW); zeros where the pixel is not valid"""
    v = interp(x, OH, OW)
    C = v.shape[-1]
    label = np.asarray(label, dtype=np.int64)
    labelled = (label >= 0) & (label < C)
    finite = np.all(np.isfinite(v), axis=-1)
    valid, ignored, nonfinite = labelled & finite, ~labelled, labelled & ~finite
    v = np.where(valid[..., None], v, 0.0)
    y = np.where(valid, label, 0)
    pred = np.argmax(v, axis=-1)  # (the first maximum: ties to the lowest index)
    vmax = np.max(v, axis=-1)
    srt = np.sort(v, axis=-1)
    gap = srt[..., -1] - srt[..., -2] if C > 1 else np.full(vmax.shape, np.inf)
    vy = np.take_along_axis(v, y[..., None], axis=-1)[..., 0]
    onehot = np.arange(C)[None, None, None, :] == y[..., None]
    conf, nll, brier = [], [], []
    for T in temperatures:
        r = np.float64(F32(1) / F32(T))
        e = np.exp((v - vmax[..., None]) * r)
        s = e.sum(axis=-1)
        conf.append(np.where(valid, 1.0 / s, 0.0))
        nll.append(np.where(valid, np.log(s) - (vy - vmax) * r, 0.0))
        brier.append(np.where(valid, ((e / s[..., None] - onehot) ** 2).sum(axis=-1), 0.0))
    return {"valid": valid, "ignored": ignored, "nonfinite": nonfinite, "pred": np.where(valid, pred, -1), "correct": valid & (pred == y),
            "gap": gap, "conf": np.stack(conf), "nll": np.stack(nll), "brier": np.stack(brier)}


def bins(conf, edges):
    """the number of edges with conf >= edge; conf and edges compared in the dtype of conf (float32: exactly the kernel's compare)"""
    e = np.asarray(edges, dtype=conf.dtype)
    return (conf[..., None] >= e).sum(axis=-1) if e.size else np.zeros(conf.shape, dtype=np.int64)


def tables(conf, correct, keep, edges, thresholds, exact_q):
    """counts (NT, M, 3) and above (NT, NK, 2) of the pixels `keep` (NT, ...) bool.  exact_q: conf is the kernel's float32 and the third
    column the exact integer sum of conf * 2^32; otherwise it is round(sum of conf * 2^32) of float64 values (compare with a tolerance)."""
    NT, M, NK = conf.shape[0], len(edges) + 1, len(thresholds)
    counts, above = np.zeros((NT, M, 3), dtype=np.int64), np.zeros((NT, NK, 2), dtype=np.int64)
    for t in range(NT):
        k = keep[t]
        c, ok = conf[t][k], correct[k]
        b = bins(c, edges)
        q = (c.astype(np.float64) * 4294967296.0)
        q = q.astype(np.int64) if exact_q else q
        for m in range(M):
            sel = b == m
            counts[t, m] = (int(sel.sum()), int((sel & ok).sum()), int(q[sel].sum()) if exact_q else int(round(float(q[sel].sum()))))
        for j, tau in enumerate(np.asarray(thresholds, dtype=conf.dtype)):
            sel = c > tau
            above[t, j] = (int(sel.sum()), int((sel & ok).sum()))
    return counts, above


def stable(p, edges, thresholds, conf_margin=1e-5, gap_margin=1e-4):
    """(NT, B, OH, OW) bool: valid pixels whose float64 confidence keeps `conf_margin` from every edge and threshold and whose top-2
    gap is at least `gap_margin` - the pixels on which a float32 evaluation must land in the float64 evaluation's cell"""
    marks = np.concatenate([np.asarray(edges, dtype=F32).astype(np.float64), np.asarray(thresholds, dtype=F32).astype(np.float64)])
    far = np.all(np.abs(p["conf"][..., None] - marks) > conf_margin, axis=-1) if marks.size else np.ones(p["conf"].shape, dtype=bool)
    return far & (p["valid"] & (p["gap"] >= gap_margin))[None]


def ece(counts_t, N):
    """sum_m (n_m / N) |acc_m - conf_m| of one temperature's (M, 3) table, in plain Python floats"""
    total = 0.0
    for n, c, q in counts_t.tolist():
        if n:
            total += (n / N) * abs(c / n - (q / 4294967296.0) / n)
    return total


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------------

def uniform_edges(M):
    return np.array([F32(k) / F32(M) for k in range(1, M)], dtype=F32)


def _labels(rng, x, OH, OW, odd):
    """labels that agree with the net's argmax on roughly 70 % of the pixels; `odd`: a sprinkle of every ignored value"""
    C = x.shape[-1]
    pred = np.argmax(interp(x, OH, OW), axis=-1)
    label = np.where(rng.random(pred.shape) < 0.7, pred, rng.integers(0, C, pred.shape)).astype(np.int64)
    if odd and label.size >= 16:
        flat = label.reshape(-1)
        where = rng.choice(flat.size, size=max(4, flat.size // 10), replace=False)
        flat[where] = np.asarray(ODD_LABELS, dtype=np.int64)[np.arange(where.size) % 4]
    return label


#        name            (B, IH, IW, C)  (OH, OW)   temperatures  bins thresholds    layout       scale special
CASES = {
    "one_pixel":        ((1, 1, 1, 1), (1, 1), (1.0,), 15, (0.968,), "dense", 3.0, None),
    "small":            ((2, 3, 5, 9), (11, 19), T16, 15, THRESHOLDS8, "dense", 3.0, "odd"),
    "columns_plus_one": ((1, 33, 65, 9), (129, 257), (1.0, 2.0), 15, (0.968,), "dense", 3.0, "odd"),
    "identity":         ((2, 7, 6, 9), (7, 6), (1.0,), 1, (), "dense", 3.0, "odd"),
    "c12":              ((1, 5, 7, 12), (13, 21), (1.0, 0.7), 32, (0.968,), "dense", 3.0, "odd"),
    "c13":              ((1, 5, 7, 13), (13, 21), (1.0, 0.7), 32, (0.968,), "dense", 3.0, "odd"),
    "c32":              ((2, 4, 5, 32), (9, 14), T16, 15, THRESHOLDS8, "dense", 3.0, "odd"),
    "pitched":          ((2, 3, 5, 9), (11, 19), (1.0,), 15, (0.968,), "pitched", 3.0, None),
    "misaligned":       ((2, 3, 5, 9), (11, 19), (1.0,), 15, (0.968,), "misaligned", 3.0, None),
    "nonfinite":        ((1, 4, 6, 9), (16, 24), (1.0, 2.0), 15, (0.968,), "dense", 3.0, "nonfinite"),
    "extreme":          ((1, 4, 6, 9), (10, 13), (0.25, 1.0, 8.0), 15, (0.968,), "dense", 80.0, "extreme"),
}


def make_case(name, seed=None):
    """-> dict(x float32 (B, IH, IW, C), label int64 (B, OH, OW), OH, OW, temperatures, edges float32, thresholds, layout)"""
    shape, (OH, OW), temps, M, thr, layout, scale, special = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1000 if seed is None else seed)
    x = (scale * rng.standard_normal(shape)).astype(F32)
    if special == "extreme":  # every source pixel: one logit of +80, one of -80, ordinary ones beside them (no exact ties between channels)
        x = (x / F32(20.0)).astype(F32)
        hi = rng.integers(0, shape[3], shape[:3])
        lo = (hi + rng.integers(1, shape[3], shape[:3])) % shape[3]
        np.put_along_axis(x, hi[..., None], F32(80.0), axis=-1)
        np.put_along_axis(x, lo[..., None], F32(-80.0), axis=-1)
    clean = x.copy()
    if special == "nonfinite":  # one source pixel with an infinite, one with a NaN logit; the labels are drawn from the clean logits
        x[0, 0, 1, 3], x[0, 3, 4, 5] = np.inf, np.nan
    label = _labels(rng, clean, OH, OW, odd=special == "odd")
    return {"x": x, "label": label, "OH": OH, "OW": OW, "temperatures": tuple(temps), "edges": uniform_edges(M), "thresholds": tuple(thr),
            "layout": layout}
