"""Numpy restatement of the class-balance device code, for the tests only: the per-frame count table of csrc/label_stats.hip and
the second pick rule of csrc/augment.hip (segmif_augment_pick_class_u8), built on _augment_ref's nearest resize."""
import numpy as np

import _augment_ref as ar


def counts(label):
    """(N, ...) integer label maps -> (N, 257) int64: column v < 256 the pixels equal to v, column 256 the values outside 0..255"""
    lab = np.asarray(label).astype(np.int64).reshape(len(label), -1)
    lab = np.where((lab < 0) | (lab > 255), 256, lab)
    return np.stack([np.bincount(row, minlength=257) for row in lab]).astype(np.int64)


def windows(label, p, crop):
    """the ten candidate windows of parameters p on the nearest-resized, flipped, 255-padded label"""
    nw, nh = int(p["nw"]), int(p["nh"])
    lab_r = ar.resize_nearest(label, nw, nh)
    if p["flip"]:
        lab_r = lab_r[:, ::-1]
    y, x = int(p["pad_h"]), int(p["pad_w"])
    canvas = np.full((max(crop, nh), max(crop, nw)), 255, dtype=np.int64)
    canvas[y:y + nh, x:x + nw] = lab_r
    return [canvas[hs:hs + crop, ws:ws + crop] for hs, ws in np.asarray(p["cand"]).reshape(-1, 2)]


def pick_class(label, p, crop, c, t):
    """-> (chosen, (box_h, box_w), accepted mask, got, hit) of one sample with want = (c, t)"""
    wins = windows(label, p, crop)
    cand = np.asarray(p["cand"]).reshape(-1, 2)
    if c < 0:  # the reference's rule: first accepted, else the last
        ok = [ar.accepted(w) for w in wins]
        chosen = ok.index(True) if any(ok) else len(wins) - 1
        got = -1
    else:
        n = [int((w == c).sum()) for w in wins]
        ok = [v > t for v in n]
        chosen = ok.index(True) if any(ok) else int(np.argmax(n))  # (argmax: the lowest index among equal counts)
        got = n[chosen]
    mask = sum(1 << k for k, v in enumerate(ok) if v)
    return chosen, (int(cand[chosen][0]), int(cand[chosen][1])), mask, got, any(ok)


def tally(wants, hits, n_class):
    """(n_class, 2) int64: drawn and hit per class over samples with want[b] = (c, t), c >= 0"""
    out = np.zeros((n_class, 2), dtype=np.int64)
    for (c, _), hit in zip(wants, hits):
        if 0 <= c < n_class:
            out[c, 0] += 1
            out[c, 1] += int(hit)
    return out
