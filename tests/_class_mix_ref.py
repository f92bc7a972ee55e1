"""Numpy restatement of the ClassMix rule of include/segmif_hip.h (segmif_class_mix_select / segmif_class_mix_apply_f32),
written from the rule and not from the kernels.  Integers and verbatim copies only: float planes are passed as int32 views."""
import numpy as np


def counts(label, n_class):
    """(B, n_class): pixels of crop b equal to c, on the full integer value (255, negatives, 256, 2^40 + 3 never count)"""
    return np.stack([[int((lab == c).sum()) for c in range(n_class)] for lab in label]).astype(np.int64).reshape(len(label), n_class)


def select(counts, table, n_class, min_pixels):
    """counts (B, >= n_class) per-crop class counts, table (B, 2 + n_class) rows (donor, force, keys)
    -> sel (B, 8) int32 bit words, pasted (B,) int64, chosen: the list of the selected classes per receiver"""
    B = len(table)
    sel, pasted, chosen = np.zeros((B, 8), dtype=np.uint32), np.zeros(B, dtype=np.int64), []
    for b in range(B):
        d, force, key = int(table[b][0]), int(table[b][1]), [int(k) for k in table[b][2:2 + n_class]]
        picked = []
        if d != b:
            present = [c for c in range(n_class) if int(counts[d][c]) > min_pixels]
            if force >= 0:
                picked = [force] if force in present else []
            else:
                k = (len(present) + len(present) % 2) // 2
                picked = sorted(sorted(present, key=lambda c: key[c])[:k])
        for c in picked:
            sel[b, c >> 5] |= np.uint32(1 << (c & 31))
            pasted[b] += int(counts[d][c])
        chosen.append(picked)
    return sel.view(np.int32), pasted, chosen


def tally(counts, table, chosen, n_class):
    """(n_class, 2): samples that selected c, pixels pasted of c"""
    t = np.zeros((n_class, 2), dtype=np.int64)
    for b, picked in enumerate(chosen):
        for c in picked:
            t[c] += (1, int(counts[int(table[b][0])][c]))
    return t


def apply(planes, label, donor, sel):
    """planes: arrays (B, C, h, w) of any dtype, label (B, h, w) int64, donor (B,), sel (B, 8) int32
    -> (mixed planes, mixed label, M (B, h, w) bool).  Donors are the unmixed inputs."""
    words = np.asarray(sel).view(np.uint32)
    M = np.zeros(label.shape, dtype=bool)
    for b in range(len(label)):
        d = int(donor[b])
        if d == b:
            continue
        inside = [c for c in range(256) if (int(words[b, c >> 5]) >> (c & 31)) & 1]
        M[b] = np.isin(label[d], inside)
    don = [int(d) for d in donor]
    out = [np.where(M[:, None], p[don], p) for p in planes]
    return out, np.where(M, label[don], label), M
