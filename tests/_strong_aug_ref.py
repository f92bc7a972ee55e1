"""Numpy restatement of the strong-augmentation rule of include/segmif_hip.h (segmif_strong_augment_f32), parametrised by dtype:
evaluated in float64 it is the truth the kernels are held to, the same code in float32 is the yardstick for what float32
arithmetic costs.  Every product and sum is written as the rule writes it; nothing here is vectorised across the rule's steps."""
import numpy as np

MAX_RADIUS = 8


def record(jitter=None, radius=0, taps=None):
    """one record as a dict: jitter (fb, fc, fs, fh) or None, radius and taps[0..8]"""
    t = np.zeros(MAX_RADIUS + 1, dtype=np.float32)
    t[0] = 1.0
    if taps is not None:
        t[:len(taps)] = taps
    return dict(jitter=None if jitter is None else tuple(float(np.float32(v)) for v in jitter), radius=int(radius), taps=t)


def to_table(records, dtype):
    """the records as a (B,) array of ops.strong_rec_dtype()"""
    table = np.zeros(len(records), dtype=dtype)
    for b, r in enumerate(records):
        table["jitter_on"][b] = r["jitter"] is not None
        table["fb"][b], table["fc"][b], table["fs"][b], table["fh"][b] = r["jitter"] if r["jitter"] is not None else (1.0, 1.0, 1.0, 0.0)
        table["radius"][b], table["taps"][b] = r["radius"], r["taps"]
    return table


def from_table(table):
    return [dict(jitter=(float(t["fb"]), float(t["fc"]), float(t["fs"]), float(t["fh"])) if t["jitter_on"] else None,
                 radius=int(t["radius"]), taps=np.array(t["taps"], dtype=np.float32)) for t in table]


def clamp(v):
    return np.clip(v, v.dtype.type(0), v.dtype.type(1))


def luma(v):
    dt = v.dtype.type
    return (dt(np.float32(0.299)) * v[0] + dt(np.float32(0.587)) * v[1]) + dt(np.float32(0.114)) * v[2]


def brightness(v, fb):
    return clamp(v.dtype.type(fb) * v)


def luma_mean(v):
    """the double sum of luma over the pixels, divided by their number, rounded to the dtype"""
    return v.dtype.type(luma(v).astype(np.float64).sum() / float(v[0].size))


def contrast(v, fc, m):
    dt = v.dtype.type
    return clamp(dt(fc) * v + (dt(1) - dt(fc)) * dt(m))


def saturation(v, fs):
    dt = v.dtype.type
    return clamp(dt(fs) * v + ((dt(1) - dt(fs)) * luma(v))[None])


def frac(t):
    return t - np.floor(t)


def rgb_to_hsv(v):
    dt = v.dtype.type
    r, g, b = v
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eq, cr = mx == mn, mx - mn
    one = np.ones_like(mx)
    s, d = cr / np.where(eq, one, mx), np.where(eq, one, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    h = np.where(mx == r, bc - gc, np.where(mx == g, (dt(2) + rc) - bc, (dt(4) + gc) - rc))
    return frac(h / dt(6) + dt(1)), s, mx


def hsv_to_rgb(h, s, V):
    dt = V.dtype.type
    h6 = dt(6) * h
    fl = np.floor(h6)
    f, i = h6 - fl, fl.astype(np.int64) % 6
    p, q, t = clamp(V * (dt(1) - s)), clamp(V * (dt(1) - s * f)), clamp(V * (dt(1) - s * (dt(1) - f)))
    return np.stack([np.choose(i, [V, q, p, p, t, V]), np.choose(i, [t, V, V, q, p, p]), np.choose(i, [p, p, t, V, V, q])])


def hue(v, fh):
    h, s, V = rgb_to_hsv(v)
    return hsv_to_rgb(frac(h + v.dtype.type(fh)), s, V)


def jitter(v, fb, fc, fs, fh):
    """-> (the jittered (3, h, w) sample, m_b)"""
    v = brightness(v, fb)
    m = luma_mean(v)
    return hue(saturation(contrast(v, fc, m), fs), fh), m


def reflect_index(n, radius):
    """source index of positions -radius .. n - 1 + radius: -i -> i, n - 1 + i -> n - 1 - i"""
    i = np.arange(-radius, n + radius)
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def blur_axis(v, taps, radius, axis):
    dt = v.dtype.type
    n = v.shape[axis]
    padded = np.take(v, reflect_index(n, radius), axis=axis)
    at = lambda k: np.take(padded, np.arange(radius + k, radius + k + n), axis=axis)
    acc = dt(taps[0]) * at(0)
    for k in range(1, radius + 1):
        acc = acc + dt(taps[k]) * (at(-k) + at(k))
    return acc


def blur(v, taps, radius):
    """rows first (along the width), then columns"""
    return blur_axis(blur_axis(v, taps, radius, 2), taps, radius, 1)


def effective_radius(radius, h, w):
    return radius if 0 <= radius <= min(MAX_RADIUS, h - 1, w - 1) else 0


def strong_augment(x, records, dtype):
    """x (B, 3, h, w) -> (y (B, 3, h, w) of dtype, mean (B,) of dtype)"""
    x = np.asarray(x)
    B, _, h, w = x.shape
    y, mean = np.empty(x.shape, dtype=dtype), np.zeros(B, dtype=dtype)
    for b, r in enumerate(records):
        v = x[b].astype(dtype)
        if r["jitter"] is not None:
            v, mean[b] = jitter(v, *r["jitter"])
        R = effective_radius(r["radius"], h, w)
        y[b] = blur(v, r["taps"], R) if R else v
    return y, mean
