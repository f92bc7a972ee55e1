"""Integer numpy model of the training loader's augmentation, for the tests only; independent of segmif_amd.data (the tables
are rebuilt here with plain loops that follow Pillow's C code line by line, the package builds them vectorised).

The transform (datasets/voc_fusion3.py:169-216, datasets/imutils.py): Pillow BILINEAR resize of the three images and NEAREST
resize of the label to (nw, nh); np.fliplr; on the visible image brightness then contrast, each
uint8(clip(float32(v) * alpha + beta, 0, 255)); a float32 canvas of max(crop, n) filled with mean_rgb per channel (255 for the
label) that holds the image at (pad_h, pad_w); the first of the ten candidate windows whose label counts pass the class-balance
test, else the last; / 255 in float32; CHW.
"""
import numpy as np

PREC = 22
MEAN_RGB = np.array([123.675, 116.28, 103.53], dtype=np.float32)
PARAM_KEYS = ("nw", "nh", "flip", "bright_on", "beta", "contrast_on", "alpha", "pad_h", "pad_w", "cand")


def coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle) filter -> list of (xmin, [k...])"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * (1.0 / fs))
            wv = 1.0 - a if a < 1.0 else 0.0
            ws.append(wv)
            ww += wv
        if ww != 0.0:
            ws = [v / ww for v in ws]
        out.append((xmin, [int(0.5 + v * (1 << PREC)) for v in ws]))
    return out


def _pass(img, table, axis):
    """one pass over `axis` (0 rows, 1 columns) of an (h, w, c) uint8 image"""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(table),) + src.shape[1:], dtype=np.int64)
    for i, (lo, ks) in enumerate(table):
        acc = np.full(src.shape[1:], 1 << (PREC - 1), dtype=np.int64)
        for t, k in enumerate(ks):
            acc = acc + k * src[lo + t]
        out[i] = np.clip(acc >> PREC, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize_bilinear(img, nw, nh):
    """Image.fromarray(img).resize((nw, nh), BILINEAR) for uint8 (h, w) or (h, w, c): horizontal pass, rounded, then vertical;
    an axis that keeps its size is skipped"""
    a = img[:, :, None] if img.ndim == 2 else img
    h, w = a.shape[:2]
    if nw != w:
        a = _pass(a, coeffs(w, nw), 1)
    if nh != h:
        a = _pass(a, coeffs(h, nh), 0)
    return a[:, :, 0] if img.ndim == 2 else a


def nearest_index(in_size, out_size):
    """Geometry.c ImagingScaleAffine: xo = a / 2, then xo += a per output index, accumulated in double"""
    if in_size == out_size:
        return np.arange(out_size)
    a = in_size / out_size
    xo, idx = a * 0.5, []
    for _ in range(out_size):
        idx.append(int(xo))
        xo += a
    return np.array(idx)


def resize_nearest(lab, nw, nh):
    h, w = lab.shape
    return lab[nearest_index(h, nh)][:, nearest_index(w, nw)]


def convert(img_u8, alpha, beta):
    """PhotoMetricDistortion.convert with the scalars as float32 (numpy's arithmetic of a float32 array with Python scalars)"""
    f = img_u8.astype(np.float32) * np.float32(alpha) + np.float32(beta)
    return np.clip(f, 0, 255).astype(np.uint8)


def accepted(window):
    """imutils.py:232-235 on one crop window of the padded label, in integers"""
    cnt = np.bincount(window.reshape(-1).astype(np.int64), minlength=256)[:255]
    return bool(cnt.sum() > 0 and 4 * cnt.max() < 3 * cnt.sum())


def accepted_mask(label, p, crop):
    """bit c set = candidate c of p passes accepted() on the resized, flipped, 255-padded label: what the pick kernel leaves in
    the record's `accepted` field (it tests all ten, the loop of transform() stops at the first)"""
    nw, nh = int(p["nw"]), int(p["nh"])
    lab_r = resize_nearest(label, nw, nh)
    if p["flip"]:
        lab_r = lab_r[:, ::-1]
    y, x = int(p["pad_h"]), int(p["pad_w"])
    lab_c = np.full((max(crop, nh), max(crop, nw)), 255, dtype=np.int64)
    lab_c[y:y + nh, x:x + nw] = lab_r
    cand = np.asarray(p["cand"]).reshape(-1, 2)
    return sum(1 << i for i, (hs, ws) in enumerate(cand) if accepted(lab_c[hs:hs + crop, ws:ws + crop]))


def transform(ir, vis, mask, label, p, crop):
    """uint8 ir, mask, label (h, w) and vis (h, w, 3), parameters p (PARAM_KEYS) -> ir3, vis3, mask3 (3, crop, crop) float32,
    label (crop, crop) int64, box (row, column), index of the kept candidate"""
    nw, nh = int(p["nw"]), int(p["nh"])
    ir_r, mask_r, vis_r = resize_bilinear(ir, nw, nh), resize_bilinear(mask, nw, nh), resize_bilinear(vis, nw, nh)
    lab_r = resize_nearest(label, nw, nh)
    if p["flip"]:
        ir_r, mask_r, vis_r, lab_r = ir_r[:, ::-1], mask_r[:, ::-1], vis_r[:, ::-1], lab_r[:, ::-1]
    if p["bright_on"]:
        vis_r = convert(vis_r, 1.0, p["beta"])
    if p["contrast_on"]:
        vis_r = convert(vis_r, p["alpha"], 0.0)
    H, W = max(crop, nh), max(crop, nw)
    y, x = int(p["pad_h"]), int(p["pad_w"])
    canvas = np.empty((3, H, W, 3), dtype=np.float32)
    canvas[:] = MEAN_RGB
    canvas[0, y:y + nh, x:x + nw] = ir_r[:, :, None]
    canvas[1, y:y + nh, x:x + nw] = vis_r
    canvas[2, y:y + nh, x:x + nw] = mask_r[:, :, None]
    lab_c = np.full((H, W), 255, dtype=np.int64)
    lab_c[y:y + nh, x:x + nw] = lab_r
    cand = np.asarray(p["cand"]).reshape(-1, 2)
    chosen = len(cand) - 1
    for i, (hs, ws) in enumerate(cand):
        if accepted(lab_c[hs:hs + crop, ws:ws + crop]):
            chosen = i
            break
    hs, ws = (int(v) for v in cand[chosen])
    out = (canvas[:, hs:hs + crop, ws:ws + crop] / np.float32(255.0)).transpose(0, 3, 1, 2)
    assert out.dtype == np.float32
    return out[0], out[1], out[2], lab_c[hs:hs + crop, ws:ws + crop], (hs, ws), chosen


def random_params(rng, h, w, crop, ratio):
    """seeded parameters for the model-against-kernel tests (numpy Generator; not the package's sampler)"""
    nw, nh = int(ratio * w), int(ratio * h)
    H, W = max(crop, nh), max(crop, nw)
    return {"nw": nw, "nh": nh, "flip": bool(rng.integers(2)), "bright_on": bool(rng.integers(2)), "beta": float(rng.uniform(-32, 32)),
            "contrast_on": bool(rng.integers(2)), "alpha": float(rng.uniform(0.5, 1.5)), "pad_h": int(rng.integers(H - nh + 1)),
            "pad_w": int(rng.integers(W - nw + 1)),
            "cand": [(int(rng.integers(H - crop + 1)), int(rng.integers(W - crop + 1))) for _ in range(10)], "H": H, "W": W, "ratio": ratio}

