"""The rules of include/segmif_paste.h restated in numpy, written from the header and sharing no code with csrc/copy_paste.hip: boxes
and areas per root with np.unique / np.where over roots taken from tests/_objects_ref.py (min-propagation), the patch store by a loop
over objects, the paste by a loop over slots from FIRST to LAST, overwriting (the kernel walks from last to first and stops at the
first hit: the two orders meet in the same picture).  self_checks() holds the cases worked by hand; the host test also compares the
boxes with scipy.ndimage.find_objects."""
import numpy as np

import _objects_ref as objects_ref

WORDS, MAX_SLOTS, MAX_SIZE, MAX_STEP = 8, 8, 4096, 1 << 24
ODD_LABELS = (255, -1, 256, 2 ** 40 + 3)


def roots_of(label, K, conn=8):
    """(n, H, W) uint8 labels -> (n, H, W) int32 roots: values outside 0..K-1 belong to no component"""
    label = np.asarray(label).astype(np.int64)
    m = np.where((label >= 0) & (label < K), label, objects_ref.IGN)
    return np.stack([objects_ref.roots(f, conn) for f in m])


def boxes(root, label, K, class_mask, min_area, max_box, frame0=0):
    """-> (M, 8) int32 records {frame, root, cls, area, x0, y0, bw, bh}, sorted by (frame, root)"""
    out = []
    for f in range(len(root)):
        r = root[f]
        W = r.shape[1]
        ys, xs = np.where(r >= 0)
        if not len(ys):
            continue
        q, inv, area = np.unique(r[ys, xs], return_inverse=True, return_counts=True)
        x0, x1, y0, y1 = (np.full(len(q), v, dtype=np.int64) for v in (1 << 40, -1, 1 << 40, -1))
        np.minimum.at(x0, inv, xs), np.maximum.at(x1, inv, xs), np.minimum.at(y0, inv, ys), np.maximum.at(y1, inv, ys)
        for i, root_i in enumerate(q):  # np.unique sorts: ascending roots
            cls = int(label[f][root_i // W, root_i % W])
            bw, bh = int(x1[i] - x0[i] + 1), int(y1[i] - y0[i] + 1)
            if cls < K and (class_mask >> cls) & 1 and area[i] >= min_area and bw * bh <= max_box:
                out.append((frame0 + f, int(root_i), cls, int(area[i]), int(x0[i]), int(y0[i]), bw, bh))
    return np.asarray(out, dtype=np.int32).reshape(-1, WORDS)


def offsets_of(records):
    return np.concatenate(([0], np.cumsum(records[:, 6].astype(np.int64) * records[:, 7]))).astype(np.int64)


def pack(records, offsets, root, ir, vis, mask):
    """root, ir, mask (N, H, W), vis (N, H, W, 3) of the WHOLE set (a record's frame indexes them) -> patches (offsets[-1], 8) uint8"""
    patches = np.zeros((int(offsets[-1]), WORDS), dtype=np.uint8)
    for m, (frame, r, _, _, x0, y0, bw, bh) in enumerate(records):
        box = (frame, slice(y0, y0 + bh), slice(x0, x0 + bw))
        alpha = root[box] == r
        px = np.zeros((bh, bw, WORDS), dtype=np.uint8)
        px[..., 0], px[..., 1:4], px[..., 4], px[..., 5] = ir[box], vis[box], mask[box], 1
        px[~alpha] = 0
        patches[offsets[m]:offsets[m] + bw * bh] = px.reshape(-1, WORDS)
    return patches


def slot_is_empty(slot, records, offsets, store_pixels):
    obj, _, _, ow, oh, sx, sy, _ = (int(v) for v in slot)
    if not 0 <= obj < len(records) or not 1 <= ow <= MAX_SIZE or not 1 <= oh <= MAX_SIZE or not 1 <= sx <= MAX_STEP or not 1 <= sy <= MAX_STEP:
        return True
    bw, bh, off = int(records[obj, 6]), int(records[obj, 7]), int(offsets[obj])
    return bw < 1 or bh < 1 or off < 0 or off + bw * bh > store_pixels  # (a bank that does not hold its own record)


def unit(byte):
    """byte / 255 rounded to nearest in float32: numpy's float32 division is IEEE's"""
    return np.asarray(byte).astype(np.float32) / np.float32(255.0)


def paste(ir3, vis3, mask3, label, records, offsets, patches, table, n_class, tally=None):
    """-> (ir3', vis3', mask3', label', pasted (B,), tally (n_class, 2)) as new arrays; floats are moved as their bits"""
    out = [np.array(t, copy=True) for t in (ir3, vis3, mask3, label)]
    B, h, w = label.shape
    table = np.asarray(table).reshape(B, -1, WORDS)
    tally = np.zeros((n_class, 2), dtype=np.int64) if tally is None else np.array(tally, copy=True)
    win = np.full((B, h, w), -1, dtype=np.int64)
    for b in range(B):
        for s, slot in enumerate(table[b]):  # first to last, overwriting: the last one lies on top
            if slot_is_empty(slot, records, offsets, len(patches)):
                continue
            obj, dx, dy, ow, oh, sx, sy, flip = (int(v) for v in slot)
            cls, bw, bh, off = int(records[obj, 2]), int(records[obj, 6]), int(records[obj, 7]), int(offsets[obj])
            if 0 <= cls < n_class:
                tally[cls, 0] += 1
            u, v = np.arange(ow, dtype=np.int64), np.arange(oh, dtype=np.int64)
            su = np.minimum(bw - 1, (u * sx + (sx >> 1)) >> 16)
            if flip & 1:
                su = bw - 1 - su
            sv = np.minimum(bh - 1, (v * sy + (sy >> 1)) >> 16)
            x, y = u + dx, v + dy
            kx, ky = (x >= 0) & (x < w), (y >= 0) & (y < h)
            if not kx.any() or not ky.any():
                continue
            px = patches[off + sv[ky][:, None] * bw + su[kx][None, :]]  # (rows, cols, 8)
            on = px[..., 5] == 1
            yy, xx = np.meshgrid(y[ky], x[kx], indexing="ij")
            yy, xx, px = yy[on], xx[on], px[on]
            for c in range(3):
                out[0][b, c, yy, xx] = unit(px[:, 0])
                out[1][b, c, yy, xx] = unit(px[:, 1 + c])
                out[2][b, c, yy, xx] = unit(px[:, 4])
            out[3][b, yy, xx] = cls
            win[b, yy, xx] = s
        for s, slot in enumerate(table[b]):
            n = int((win[b] == s).sum())
            if n:
                cls = int(records[int(slot[0]), 2])
                if 0 <= cls < n_class:
                    tally[cls, 1] += n
    return out[0], out[1], out[2], out[3], (win >= 0).sum(axis=(1, 2)).astype(np.int64), tally


def slot(obj, dx, dy, bw, bh, scale=1.0, flip=0):
    """the slot the policy forms for a box of bw x bh at a scale: ow = round(bw * s), sx = (bw << 16) // ow"""
    ow, oh = max(1, int(round(bw * scale))), max(1, int(round(bh * scale)))
    return (obj, dx, dy, ow, oh, (bw << 16) // ow, (bh << 16) // oh, flip)


# ---- cases worked by hand -------------------------------------------------------------------------------------------------------------

def _hand_bank():
    """one frame 4 x 6 with a 2 x 3 object of class 2 whose top-right pixel belongs to the background: an L-shaped blob"""
    label = np.zeros((1, 4, 6), dtype=np.uint8)
    label[0, 1:3, 2:5] = 2
    label[0, 1, 4] = 0
    ir = (np.arange(24, dtype=np.uint8) * 10).reshape(1, 4, 6)
    vis = np.stack([ir + 1, ir + 2, ir + 3], axis=-1).astype(np.uint8)
    mask = (ir // 2).astype(np.uint8)
    root = roots_of(label, 3)
    rec = boxes(root, label, 3, 0b100, 1, 100)
    off = offsets_of(rec)
    return label, ir, vis, mask, root, rec, off, pack(rec, off, root, ir, vis, mask)


def _blank(B, h, w):
    z = np.zeros((B, 3, h, w), dtype=np.float32)
    return z, z.copy(), z.copy(), np.full((B, h, w), 7, dtype=np.int64)


def self_checks():
    label, ir, vis, mask, root, rec, off, patches = _hand_bank()
    # the box: root 8 (row 1, column 2), class 2, area 5, x0 2, y0 1, 3 wide and 2 high
    assert rec.tolist() == [[0, 8, 2, 5, 2, 1, 3, 2]] and off.tolist() == [0, 6]
    assert patches[:, 5].tolist() == [1, 1, 0, 1, 1, 1] and not patches[2].any()          # the background pixel leaves no trace
    assert patches[0].tolist() == [80, 81, 82, 83, 40, 1, 0, 0] and patches[5, 0] == 160   # ir 80 at (1, 2), 160 at (2, 4)

    # as it is, at (1, 0) of a 4 x 8 crop
    o = paste(*_blank(1, 4, 8), rec, off, patches, [[slot(0, 1, 0, 3, 2)]], 3)
    assert o[3][0].tolist() == [[7, 2, 2, 7, 7, 7, 7, 7], [7, 2, 2, 2, 7, 7, 7, 7], [7] * 8, [7] * 8]
    assert o[0][0, 1, 0, 1] == np.float32(80) / np.float32(255) and o[1][0, 2, 1, 3] == np.float32(163) / np.float32(255)
    assert o[2][0, 0, 1, 1] == np.float32(70) / np.float32(255) and o[4].tolist() == [5] and o[5].tolist() == [[0, 0], [0, 0], [1, 5]]

    # a flipped 2 x 3 object: the hole moves to the top LEFT, and ir 100 (column 4 of the frame) comes first in the bottom row
    o = paste(*_blank(1, 4, 8), rec, off, patches, [[slot(0, 1, 0, 3, 2, flip=1)]], 3)
    assert o[3][0, :2, :5].tolist() == [[7, 7, 2, 2, 7], [7, 2, 2, 2, 7]]
    assert o[0][0, 0, 1, 1] == np.float32(160) / np.float32(255) and o[0][0, 0, 1, 3] == np.float32(140) / np.float32(255)

    # a scale of 2: every source pixel becomes 2 x 2 (su = (u * 32768 + 16384) >> 16 = 0, 0, 1, 1, 2, 2)
    s2 = slot(0, 0, 0, 3, 2, scale=2.0)
    assert s2[3:7] == (6, 4, 32768, 32768)
    o = paste(*_blank(1, 4, 8), rec, off, patches, [[s2]], 3)
    assert o[3][0].tolist() == [[2, 2, 2, 2, 7, 7, 7, 7]] * 2 + [[2, 2, 2, 2, 2, 2, 7, 7]] * 2 and o[4].tolist() == [20]

    # a scale of 0.5: ow = round(1.5) = 2, oh = 1; sx = 98304, so su = (0 + 49152) >> 16 = 0 and (98304 + 49152) >> 16 = 2;
    # sy = 131072, sv = 65536 >> 16 = 1: columns 0 and 2 of the BOTTOM row, ir 140 and 160 (the hole is in the top row)
    sh = slot(0, 2, 3, 3, 2, scale=0.5)
    assert sh[3:7] == (2, 1, 98304, 131072)
    o = paste(*_blank(1, 4, 8), rec, off, patches, [[sh]], 3)
    assert o[3][0, 3].tolist() == [7, 7, 2, 2, 7, 7, 7, 7] and o[0][0, 0, 3, 2] == np.float32(140) / np.float32(255)
    assert o[0][0, 0, 3, 3] == np.float32(160) / np.float32(255)

    # two overlapping slots: the second lies on top where ITS alpha is set, and the first shows through the second's hole
    o = paste(*_blank(1, 4, 8), rec, off, patches, [[slot(0, 0, 0, 3, 2, scale=2.0), slot(0, 1, 1, 3, 2, flip=1)]], 3)
    assert o[4].tolist() == [20] and o[5][2].tolist() == [2, 20]
    assert o[0][0, 0, 1, 1] == np.float32(80) / np.float32(255)    # the second's hole at (1, 1): the first's pixel (source 0, 0)
    assert o[0][0, 0, 1, 2] == np.float32(90) / np.float32(255)    # the second's own (flipped: source column 1 of row 0)
    assert o[0][0, 0, 2, 1] == np.float32(160) / np.float32(255)   # the second's bottom row, flipped
    # an empty slot and one wholly outside change nothing, the latter still counts as drawn
    base = _blank(1, 4, 8)
    o = paste(*base, rec, off, patches, [[(1, 0, 0, 3, 2, 65536, 65536, 0), slot(0, 8, 0, 3, 2), (0, 0, 0, 0, 2, 65536, 65536, 0)]], 3)
    assert all(np.array_equal(a, b) for a, b in zip(o[:4], base)) and o[4].tolist() == [0] and o[5][2].tolist() == [1, 0]
