"""The rule of segmif_object_stats_i32 (include/segmif_objects.h) restated in numpy.  Roots come from MIN-PROPAGATION to a fixed
point: root = own index at valid pixels, then root = min(root, root of each equal-valued neighbour) until nothing changes.  That
yields the canonical minimum-index root directly and shares no idea with the union-find of csrc/objects.hip, so the two cannot
share a mistake.  The tables are np.bincount over the roots.  No scipy.  Also the seeded inputs (CASES) the object tests use."""
import functools

import numpy as np

IGN = -1
DECILES = 11
DEFAULT_SIZE_EDGES = (1024, 9216)
ODD_LABELS = (255, -1, 256, 2 ** 40 + 3)
NEIGHBOURS = {4: ((0, 1), (1, 0), (0, -1), (-1, 0)),
              8: ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))}


def maps(pred, label, K):
    """pred, label of any shape -> g, p as int64 maps with IGN (boundary_stats' conventions)"""
    label = np.asarray(label).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    g = np.where((label >= 0) & (label < K), label, IGN)
    p = np.where((g != IGN) & (pred >= 0) & (pred < K), pred, IGN)
    return g, p


def roots(m, conn):
    """(H, W) map with IGN -> (H, W) int32: the smallest linear index of each pixel's component, -1 at IGN"""
    H, W = m.shape
    BIG = H * W  # larger than any index: what a pixel outside the frame or of another value offers
    valid = m != IGN
    root = np.where(valid, np.arange(H * W, dtype=np.int64).reshape(H, W), BIG)
    pm = np.full((H + 2, W + 2), -2, dtype=np.int64)  # the padding equals no value, IGN included
    pm[1:-1, 1:-1] = m
    joined = [(dy, dx, valid & (pm[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == m)) for dy, dx in NEIGHBOURS[conn]]
    while True:
        pr = np.full((H + 2, W + 2), BIG, dtype=np.int64)
        pr[1:-1, 1:-1] = root
        new = root
        for dy, dx, same in joined:
            new = np.where(same, np.minimum(new, pr[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]), new)
        if np.array_equal(new, root):
            break
        root = new
    return np.where(valid, root, -1).astype(np.int32)


def frame_tables(g, p, K, conn, edges):
    """one frame's g, p -> root_g, root_p (H, W) int32, obj (2, K, S, 11), mass (2, K, S, 2) int64"""
    H, W = g.shape
    N, S = H * W, len(edges) + 1
    obj = np.zeros((2, K, S, DECILES), dtype=np.int64)
    mass = np.zeros((2, K, S, 2), dtype=np.int64)
    out = []
    for side, (m, other) in enumerate(((g, p), (p, g))):
        r = roots(m, conn)
        out.append(r)
        valid = r >= 0
        area = np.bincount(r[valid], minlength=N)
        hit = np.bincount(r[valid & (other == m)], minlength=N)
        for q in np.flatnonzero(area):
            c = int(m.reshape(-1)[q])
            a, h = int(area[q]), int(hit[q])
            s = sum(1 for e in edges if a >= e)
            j = (10 * h) // a
            obj[side, c, s, j] += 1
            mass[side, c, s, 0] += a
            mass[side, c, s, 1] += h
    return out[0], out[1], obj, mass


def object_stats(pred, label, K, conn=8, edges=DEFAULT_SIZE_EDGES):
    """(B, H, W) arrays -> root_g, root_p (B, H, W) int32, obj (B, 2, K, S, 11), mass (B, 2, K, S, 2) int64"""
    g, p = maps(pred, label, K)
    frames = [frame_tables(g[b], p[b], K, conn, tuple(edges)) for b in range(len(g))]
    return tuple(np.stack([f[i] for f in frames]) for i in range(4))


def scores(obj, coverage=0.5):
    """the scores of the header from obj (2, K, S, 11), plain loops in float64"""
    k = int(round(coverage * 10))
    K, S = obj.shape[1], obj.shape[2]

    def ratio(n, d):
        return float("nan") if d == 0 else n / d
    R = [ratio(int(obj[0, c, :, k:].sum()), int(obj[0, c].sum())) for c in range(K)]
    P = [ratio(int(obj[1, c, :, k:].sum()), int(obj[1, c].sum())) for c in range(K)]
    F = [float("nan") if (r != r or p != p) else (0.0 if p + r == 0 else 2 * p * r / (p + r)) for p, r in zip(P, R)]
    return np.array(R), np.array(P), np.array(F)


# ---- the seeded inputs ----------------------------------------------------------------------------------------------------------------

def serpentine(H, W):
    """a width-1 path of class 1 on class 0: rows 0, 2, 4, ... full, joined alternately at the right and the left end, so one
    component of about H W / 2 pixels whose minimum travels the whole path (the sweeps of `roots` number as many)"""
    m = np.zeros((H, W), dtype=np.int64)
    m[0::2, :] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def blocky(B, H, W, K, seed, side=5):
    """seeded blocky maps: a coarse grid upsampled by nearest neighbour, the prediction the label displaced by (1, 2) with some
    blocks re-labelled"""
    rng = np.random.default_rng(seed)
    gh, gw = H // side + 3, W // side + 3
    yy, xx = np.mgrid[0:H + 1, 0:W + 2]
    label = np.empty((B, H, W), dtype=np.int64)
    pred = np.empty((B, H, W), dtype=np.int32)
    for b in range(B):
        grid = np.where(rng.random((gh, gw)) < 0.5, 0, rng.integers(0, K, (gh, gw)))
        oy, ox = rng.integers(0, side, 2)
        big = grid[(yy + oy) // side, (xx + ox) // side]
        label[b] = big[1:, 2:]
        regrid = np.where(rng.random((gh, gw)) < 0.25, rng.integers(0, K, (gh, gw)), grid)
        pred[b] = regrid[(yy + oy) // side, (xx + ox) // side][:H, :W]
    return pred, label


def _shifted_pred(label, K):
    """the label displaced by one column, so that every object is covered in part"""
    p = np.roll(label, 1, axis=-1)
    return np.where((p >= 0) & (p < K), p, 0).astype(np.int32)


def _case_small(H, W, seed):
    pred, label = blocky(1, H, W, 3, seed, side=2)
    return dict(pred=pred, label=label, K=3)


def _case_serpentine(H, W):
    label = serpentine(H, W)[None]
    pred = np.where(np.arange(W)[None, None, :] % 3 == 0, 0, label).astype(np.int32)
    return dict(pred=pred, label=label, K=2)


def _case_diagonal(n, anti):
    label = np.zeros((1, n, n), dtype=np.int64)
    i = np.arange(n)
    label[0, i, (n - 1 - i) if anti else i] = 1
    pred = label.astype(np.int32).copy()
    pred[0, i[::2], ((n - 1 - i) if anti else i)[::2]] = 0
    return dict(pred=pred, label=label, K=2)


def _case_checkerboard(n):
    yy, xx = np.mgrid[0:n, 0:n]
    label = ((yy + xx) % 2).astype(np.int64)[None]
    pred = ((yy + xx + (xx >= n // 2)) % 2).astype(np.int32)[None]
    return dict(pred=pred, label=label, K=2)


def _case_constant(n):
    label = np.full((1, n, n), 2, dtype=np.int64)
    pred = np.full((1, n, n), 2, dtype=np.int32)
    pred[0, : n // 3] = 1
    return dict(pred=pred, label=label, K=9)


def _case_blocky(K, seed, H=65, W=129, B=2):
    pred, label = blocky(B, H, W, K, seed)
    return dict(pred=pred, label=label, K=K)


def _case_odd_labels():
    pred, label = blocky(1, 70, 90, 9, 21)
    for n, v in enumerate(ODD_LABELS):
        label[0, 5 + 15 * n: 14 + 15 * n, 10 + 12 * n: 40 + 12 * n] = v
    return dict(pred=pred, label=label, K=9)


def _case_pred_out_of_range():
    pred, label = blocky(1, 70, 90, 9, 22)
    rng = np.random.default_rng(5)
    m = rng.random(pred.shape) < 0.05
    pred[m] = np.where(rng.random(int(m.sum())) < 0.5, -1, 9).astype(np.int32)
    pred[0, 30:40, 50:70] = 2 ** 31 - 1
    pred[0, 50:60, 10:30] = -2 ** 31
    return dict(pred=pred, label=label, K=9)


def _case_all_ign():
    return dict(pred=np.zeros((1, 66, 67), dtype=np.int32), label=np.full((1, 66, 67), 255, dtype=np.int64), K=9)


def _case_ignored_stripe():
    label = np.zeros((1, 40, 80), dtype=np.int64)
    label[0, 10:30, 10:70] = 3
    label[0, :, 38:42] = 255  # cuts the ground truth AND, by blanking, the predicted blob
    pred = np.zeros((1, 40, 80), dtype=np.int32)
    pred[0, 12:28, 20:60] = 3
    return dict(pred=pred, label=label, K=9)


CASES = {
    "1x1": lambda: dict(pred=np.ones((1, 1, 1), dtype=np.int32), label=np.ones((1, 1, 1), dtype=np.int64), K=2),
    "1x9": lambda: _case_small(1, 9, 1),
    "9x1": lambda: _case_small(9, 1, 2),
    "7x5": lambda: _case_small(7, 5, 3),
    "64x64": lambda: _case_blocky(9, 4, 64, 64, 1),
    "65x129": lambda: _case_blocky(9, 5, 65, 129, 1),
    "serpentine_64": lambda: _case_serpentine(64, 64),
    "serpentine_130": lambda: _case_serpentine(130, 130),
    "diagonal_130": lambda: _case_diagonal(130, False),
    "antidiagonal_130": lambda: _case_diagonal(130, True),
    "checkerboard_66": lambda: _case_checkerboard(66),
    "constant_130": lambda: _case_constant(130),
    "blocky_K1": lambda: _case_blocky(1, 6),
    "blocky_K9": lambda: _case_blocky(9, 7),
    "blocky_K32": lambda: _case_blocky(32, 8),
    "odd_labels": _case_odd_labels,
    "pred_out_of_range": _case_pred_out_of_range,
    "all_ign": _case_all_ign,
    "ignored_stripe": _case_ignored_stripe,
}


@functools.lru_cache(maxsize=None)
def case(name, conn=8, edges=DEFAULT_SIZE_EDGES):
    """-> dict(pred, label, K, conn, edges, root_g, root_p, obj, mass): the input and the restatement's answer, read-only, computed
    once per (name, conn, edges) and shared"""
    c = CASES[name]()
    c["pred"] = np.ascontiguousarray(c["pred"], dtype=np.int32)
    c["label"] = np.ascontiguousarray(c["label"], dtype=np.int64)
    c["conn"], c["edges"] = conn, tuple(edges)
    c["root_g"], c["root_p"], c["obj"], c["mass"] = object_stats(c["pred"], c["label"], c["K"], conn, edges)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
