"""The rule of segmif_boundary_stats_i32 (include/segmif_hip.h) restated in numpy: brute-force shifted compares over a padded
copy, one shift per window position.  Deliberately NOT the separable run-length form of csrc/boundary_stats.hip, so the two
cannot share a mistake.  Also the synthetic label maps the boundary tests use."""
import numpy as np

IGN = -1       # a value like any other in a compare; never counted
OUTSIDE = -2   # the padding around the frame

COLUMNS = ("g_band", "p_band", "band_inter", "g_contour", "p_contour", "g_matched", "p_matched", "reserved")


def maps(pred, label, K):
    """(H, W) pred, label -> g, p as int64 maps with IGN."""
    label = np.asarray(label).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    g = np.where((label >= 0) & (label < K), label, IGN)
    p = np.where((g != IGN) & (pred >= 0) & (pred < K), pred, IGN)
    return g, p


def _shifted(m, r, fill):
    """yields m displaced by every (dy, dx) of the (2 r + 1)^2 window; positions outside the frame read `fill`"""
    H, W = m.shape
    pad = np.full((H + 2 * r, W + 2 * r), fill, dtype=m.dtype)
    pad[r:r + H, r:r + W] = m
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            yield pad[dy:dy + H, dx:dx + W]


def band(m, d):
    uniform = np.ones(m.shape, dtype=bool)
    for s in _shifted(m, d, OUTSIDE):
        uniform &= s == m
    return (m != IGN) & ~uniform


def contour(m):
    diff = np.zeros(m.shape, dtype=bool)
    for s in _shifted(m, 1, OUTSIDE):
        diff |= (s != m) & (s != OUTSIDE)
    return (m != IGN) & diff


def near(S, theta):
    out = np.zeros(S.shape, dtype=bool)
    for s in _shifted(S, theta, False):
        out |= s
    return out


def frame_tables(pred, label, K, d, theta):
    """one frame -> cls (K, 8), trimap (K, K) int64"""
    g, p = maps(pred, label, K)
    gb, pb, gc, pc = band(g, d), band(p, d), contour(g), contour(p)
    cls = np.zeros((K, 8), dtype=np.int64)
    tri = np.zeros((K, K), dtype=np.int64)
    for c in range(K):
        GB, PB, GC, PC = gb & (g == c), pb & (p == c), gc & (g == c), pc & (p == c)
        cls[c, :7] = (GB.sum(), PB.sum(), (GB & PB).sum(), GC.sum(), PC.sum(), (GC & near(PC, theta)).sum(),
                      (PC & near(GC, theta)).sum())
        for q in range(K):
            tri[c, q] = (GB & (p == q)).sum()
    return cls, tri


def boundary_stats(pred, label, K, d, theta):
    """(B, H, W) arrays -> cls (B, K, 8), trimap (B, K, K) int64"""
    both = [frame_tables(pred[b], label[b], K, d, theta) for b in range(len(label))]
    return np.stack([c for c, _ in both]), np.stack([t for _, t in both])


def synthetic(B, H, W, K, d, seed, ignore=True):
    """Blocky label maps with edges at every offset: a seeded coarse grid (blocks of side about 3 d) upsampled by nearest
    neighbour, diagonal stripes wider than 2 d + 1 laid over it, and as the prediction the label shifted by (2, 1) with some
    blocks re-labelled.  With ignore=True the labels also hold 255, -1, 256 and 2^40 + 3, and the prediction -1 and K on valid
    pixels.  -> pred (B, H, W) int32, label (B, H, W) int64."""
    rng = np.random.default_rng(seed)
    side = max(2, 3 * d)
    gh, gw = H // side + 3, W // side + 3
    yy, xx = np.mgrid[0:H + 2, 0:W + 1]
    label = np.empty((B, H, W), dtype=np.int64)
    pred = np.empty((B, H, W), dtype=np.int32)
    for b in range(B):
        grid = np.where(rng.random((gh, gw)) < 0.6, 0, rng.integers(0, K, (gh, gw)))  # (mostly background, as real frames are)
        oy, ox = rng.integers(0, side, 2)
        big = grid[(yy + oy) // side, (xx + ox) // side]
        period = 6 * (2 * d + 2)
        stripe = ((yy + xx + rng.integers(0, period)) % period) < (2 * d + 2)
        big = np.where(stripe, (big + 1) % K, big)
        label[b] = big[2:, 1:]
        regrid = np.where(rng.random((gh, gw)) < 0.25, rng.integers(0, K, (gh, gw)), grid)
        pbig = regrid[(yy + oy) // side, (xx + ox) // side]
        pbig = np.where(stripe, (pbig + 1) % K, pbig)
        pred[b] = pbig[:H, :W]  # = the label's construction displaced by (2, 1)
    if ignore:
        for v in (255, -1, 256, 2 ** 40 + 3):
            y, x = rng.integers(0, H), rng.integers(0, W)
            label[:, y:y + max(1, H // 6), x:x + max(1, W // 6)] = v
        m = rng.random((B, H, W)) < 0.01
        pred[m] = np.where(rng.random(int(m.sum())) < 0.5, -1, K).astype(np.int32)
    return pred, label
