"""Training batches made on the device: the reference loader's `(name, ir3, vis3, mask3, label)` tuples
(datasets/voc_fusion3.py:142-216 with datasets/imutils.py; train.py:137-142, :211-215) from uint8 frames that stay resident
in device memory.  Per batch the host draws the random parameters and builds Pillow's resize tables (numpy, float64); the
pixels are produced by csrc/augment.hip and never cross the host link.

    ds = DeviceDataset.from_folder(PairFolder(root, lists, "train"))        # or DeviceDataset.from_arrays(**synthetic_pairs(...))
    for names, ir3, vis3, mask3, label in AugmentedBatches(ds, batch=8, seed=0):
        ...

What differs from the reference's loader is listed in INTEGRATION.md section 5: saturation and hue are not applied, all ten
crop candidates are always drawn, images are float32 (the reference's are float32 too, its labels float32: ours int64).
"""
import os
import random

import numpy as np
import torch

from . import dist
from .evaluate import _read

PRECISION_BITS = 22  # Pillow, Resample.c: 32 - 8 - 2
MEAN_RGB = (123.675, 116.28, 103.53)
PHOTOMETRIC = ("brightness", "contrast")
N_CANDIDATES = 10
MAX_SHRINK = 4  # csrc/augment.hip holds the horizontal-pass rows of one 16-row tile in LDS: in / out <= 4 per axis


# ------------------------------------------------------------------------------------------------------------ resize tables

def bilinear_table(in_size, out_size):
    """Pillow's coefficients of a BILINEAR resize of one axis, 8 bits per channel (Resample.c: precompute_coeffs with the
    triangle filter, then normalize_coeffs_8bpc) -> (taps, table) with table (out_size, 2 + taps) int32: first source index,
    tap count, fixed-point weights (22 bits).  An axis that keeps its size is not resampled by Pillow: identity table."""
    if in_size == out_size:
        t = np.zeros((out_size, 3), dtype=np.int32)
        t[:, 0] = np.arange(out_size)
        t[:, 1] = 1
        t[:, 2] = 1 << PRECISION_BITS
        return 1, t
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    taps = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (int) truncates; the argument is > -1 where it is negative
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    ss = 1.0 / fs
    x = np.arange(taps, dtype=np.float64)[None, :]
    arg = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    wgt = np.where((arg < 1.0) & (x < n[:, None]), 1.0 - arg, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for i in range(taps):  # (the C loop's order of additions)
        ww = ww + wgt[:, i]
    wgt = np.where(ww[:, None] != 0.0, wgt / np.where(ww == 0.0, 1.0, ww)[:, None], wgt)
    k = (0.5 + wgt * float(1 << PRECISION_BITS)).astype(np.int64)  # weights are >= 0 for this filter
    k[x.repeat(out_size, 0) >= n[:, None]] = 0
    t = np.empty((out_size, 2 + taps), dtype=np.int32)
    t[:, 0], t[:, 1], t[:, 2:] = xmin, n, k
    return taps, t


def nearest_table(in_size, out_size):
    """Source index of every output index of Pillow's NEAREST resize (Geometry.c, ImagingScaleAffine): xo starts at a / 2 with
    a = in / out and is ADVANCED by a, the sum accumulating in double; int((x + 0.5) * a) differs at some ratios."""
    if in_size == out_size:
        return np.arange(out_size, dtype=np.int32)
    a = float(in_size) / float(out_size)
    xo = np.add.accumulate(np.concatenate(([a * 0.5], np.full(out_size - 1, a, dtype=np.float64))))  # sequential, as the C loop
    return np.minimum(xo.astype(np.int64), in_size - 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- parameters

def sample_params(py, npr, h, w, crop_h, crop_w, rescale_range=(0.5, 2.0), fliplr=True, photometric=PHOTOMETRIC):
    """One sample's random parameters with the reference's distributions, from a private random.Random `py` and
    numpy.random.RandomState `npr` (the reference draws from the two global generators in the same roles)."""
    p = {"ratio": 1.0, "flip": False, "bright_on": False, "beta": 0.0, "contrast_on": False, "alpha": 1.0}
    if rescale_range:
        lo, hi = rescale_range
        p["ratio"] = py.uniform(lo, hi)                      # imutils.py:40
    p["nw"], p["nh"] = int(p["ratio"] * w), int(p["ratio"] * h)  # imutils.py:73
    if fliplr:
        p["flip"] = py.random() > 0.5                        # imutils.py:126
    if "brightness" in photometric and npr.randint(2):       # imutils.py:316-320
        p["bright_on"], p["beta"] = True, py.uniform(-32, 32)
    if "contrast" in photometric and npr.randint(2):         # imutils.py:325-328
        p["contrast_on"], p["alpha"] = True, py.uniform(0.5, 1.5)
    H, W = max(crop_h, p["nh"]), max(crop_w, p["nw"])        # imutils.py:202-203
    p["H"], p["W"] = H, W
    p["pad_h"] = int(npr.randint(H - p["nh"] + 1))           # imutils.py:213-214
    p["pad_w"] = int(npr.randint(W - p["nw"] + 1))
    p["cand"] = [(py.randrange(0, H - crop_h + 1), py.randrange(0, W - crop_w + 1)) for _ in range(N_CANDIDATES)]
    return p


def identity_params(h, w):
    """aug=False: the frame as it is (crop = the frame, box fixed at the origin)."""
    return {"ratio": 1.0, "nw": w, "nh": h, "flip": False, "bright_on": False, "beta": 0.0, "contrast_on": False, "alpha": 1.0,
            "H": h, "W": w, "pad_h": 0, "pad_w": 0, "cand": [(0, 0)] * N_CANDIDATES, "box": (0, 0)}


# word offsets of SegmifAugmentRec (include/segmif_hip.h; segmif_amd._lib.SegmifAugmentRec is the ctypes mirror)
REC_WORDS = 48
_SRC, _H, _W, _NW, _NH, _FLIP, _BON, _BETA, _CON, _ALPHA, _PADH, _PADW, _CH, _CW, _CAND = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14
_BOXH, _BOXW, _CHOSEN, _TICKET, _AMASK, _ACCEPTED, _TABX, _TABY, _NEARX, _NEARY, _TAPSX, _TAPSY = 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45


def pack_records(indices, params, h, w):
    """-> (rec (B, REC_WORDS) int32, tab (words,) int32): the records of a batch and the resize tables they point into."""
    B = len(indices)
    rec = np.zeros((B, REC_WORDS), dtype=np.int32)
    recf = rec.view(np.float32)
    parts, at = [], 0
    for b, (src, p) in enumerate(zip(indices, params)):
        nw, nh = p["nw"], p["nh"]
        if nw < 1 or nh < 1 or w > MAX_SHRINK * nw or h > MAX_SHRINK * nh:
            raise RuntimeError(f"augment: a {h} x {w} frame scaled to {nh} x {nw} is outside the kernels' range (in / out <= {MAX_SHRINK})")
        tx, bx = bilinear_table(w, nw)
        ty, by = bilinear_table(h, nh)
        r = rec[b]
        r[_SRC], r[_H], r[_W], r[_NW], r[_NH], r[_FLIP] = src, h, w, nw, nh, int(p["flip"])
        r[_BON], r[_CON] = int(p["bright_on"]), int(p["contrast_on"])
        recf[b, _BETA], recf[b, _ALPHA] = np.float32(p["beta"]), np.float32(p["alpha"])
        r[_PADH], r[_PADW], r[_CH], r[_CW] = p["pad_h"], p["pad_w"], p["H"], p["W"]
        r[_CAND:_CAND + 2 * N_CANDIDATES] = np.asarray(p["cand"], dtype=np.int32).reshape(-1)
        if "box" in p:
            r[_BOXH], r[_BOXW] = p["box"]
        r[_TAPSX], r[_TAPSY] = tx, ty
        for word, arr in ((_TABX, bx.reshape(-1)), (_TABY, by.reshape(-1)), (_NEARX, nearest_table(w, nw)), (_NEARY, nearest_table(h, nh))):
            r[word] = at
            parts.append(arr)
            at += arr.size
    return rec, np.concatenate(parts)


# ------------------------------------------------------------------------------------------------------------------- sources

class PairFolder:
    """The reference's directory contract (voc_fusion3.py:25-30): ROOT/Infrared, Visible, Mask2, Label hold NAME.png (or
    NAME.npy) for every NAME listed in NAME_LIST_DIR/SPLIT.txt.  .npy is always read, .png when PIL imports.
    labelled=False (an unlabelled split for self-training, segmif_amd.selftrain; not the reference's): Label/ is not read - it need
    not exist - and every label is 255, the ignore value."""

    SUBDIRS = {"ir": "Infrared", "vis": "Visible", "mask": "Mask2", "label": "Label"}

    def __init__(self, root_dir, name_list_dir, split="train", labelled=True):
        self.root_dir, self.labelled = root_dir, bool(labelled)
        path = os.path.join(name_list_dir, split + ".txt")
        with open(path) as f:
            self.names = [ln.split()[0] for ln in f if ln.strip()]
        if not self.names:
            raise RuntimeError(f"{path} lists no frames")

    def __len__(self):
        return len(self.names)

    def _file(self, kind, name):
        base = os.path.join(self.root_dir, self.SUBDIRS[kind], name)
        for ext in (".png", ".npy"):
            if os.path.isfile(base + ext):
                return base + ext
        raise FileNotFoundError(f"{base}.png / .npy not found")

    def __getitem__(self, i):
        """-> (name, ir (h, w), vis (h, w, 3), mask (h, w), label (h, w)) uint8 arrays"""
        name = self.names[i]
        ir, vis, mask = (np.asarray(_read(self._file(k, name))) for k in ("ir", "vis", "mask"))
        label = np.asarray(_read(self._file("label", name))) if self.labelled else np.full(ir.shape[:2], 255, dtype=np.uint8)
        if ir.ndim != 2 or mask.ndim != 2 or label.ndim != 2 or vis.ndim != 3 or vis.shape[2] != 3:
            raise RuntimeError(f"{name}: expected grey infrared / mask / label and an RGB visible image, got shapes "
                               f"{ir.shape}, {vis.shape}, {mask.shape}, {label.shape}")
        return name, ir.astype(np.uint8), vis.astype(np.uint8), mask.astype(np.uint8), label.astype(np.uint8)


def synthetic_pairs(n, H, W, seed, n_class=9):
    """A seeded stand-in data set: uint8 frames with image-like statistics (smooth large-scale structure plus fine noise, an
    infrared plane correlated with the visible luma, a saliency-like mask) and blocky label maps of rectangles over class 0.
    -> dict(names, ir (n, H, W), vis (n, H, W, 3), mask (n, H, W), label (n, H, W)), numpy uint8.  NOT data: for smoke runs,
    tests and timing only."""
    rng = np.random.default_rng(seed)

    def smooth(channels):
        gh, gw = max(2, H // 32 + 2), max(2, W // 32 + 2)
        g = rng.random((channels, gh, gw))
        ys, xs = np.linspace(0, gh - 1, H), np.linspace(0, gw - 1, W)
        y0, x0 = np.minimum(ys.astype(int), gh - 2), np.minimum(xs.astype(int), gw - 2)
        fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
        a, b = g[:, y0][:, :, x0], g[:, y0][:, :, x0 + 1]
        c, d = g[:, y0 + 1][:, :, x0], g[:, y0 + 1][:, :, x0 + 1]
        return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy

    out = {"names": [f"syn{seed}_{i:05d}" for i in range(n)], "ir": np.empty((n, H, W), np.uint8), "vis": np.empty((n, H, W, 3), np.uint8),
           "mask": np.empty((n, H, W), np.uint8), "label": np.zeros((n, H, W), np.uint8)}
    for i in range(n):
        vis = smooth(3) * 0.8 + 0.1 + rng.normal(0, 0.03, (3, H, W))
        luma = vis.mean(0)
        ir = 0.5 * luma + 0.5 * smooth(1)[0] + rng.normal(0, 0.02, (H, W))
        lab = out["label"][i]
        for _ in range(int(rng.integers(3, 9))):
            rh, rw = int(rng.integers(max(2, H // 12), max(3, H // 2))), int(rng.integers(max(2, W // 12), max(3, W // 2)))
            y, x = int(rng.integers(0, max(1, H - rh))), int(rng.integers(0, max(1, W - rw)))
            lab[y:y + rh, x:x + rw] = rng.integers(1, n_class)
        out["vis"][i] = np.clip(vis.transpose(1, 2, 0) * 255, 0, 255).astype(np.uint8)
        out["ir"][i] = np.clip(ir * 255, 0, 255).astype(np.uint8)
        out["mask"][i] = np.where(lab > 0, 255, 0).astype(np.uint8)
    return out


class DeviceDataset:
    """The whole set as uint8 tensors on the device: ir, mask, label (N, H, W) and vis (N, H, W, 3).  MFNet's training split
    (1 569 frames of 480 x 640) is 2.9 GB this way."""

    def __init__(self, names, ir, vis, mask, label):
        for t, what in ((ir, "ir"), (vis, "vis"), (mask, "mask"), (label, "label")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"segmif_amd: DeviceDataset {what} must be a tensor on the MI355X device (the HIP path has no CPU "
                                   "fallback); DeviceDataset.from_arrays uploads host arrays")
            if t.dtype != torch.uint8:
                raise RuntimeError(f"segmif_amd: DeviceDataset {what} must be uint8, got {t.dtype}")
        N, H, W = ir.shape
        if tuple(vis.shape) != (N, H, W, 3) or tuple(mask.shape) != (N, H, W) or tuple(label.shape) != (N, H, W) or len(names) != N:
            raise RuntimeError(f"DeviceDataset: ir {tuple(ir.shape)}, vis {tuple(vis.shape)}, mask {tuple(mask.shape)}, label "
                               f"{tuple(label.shape)} and {len(names)} names do not describe one set of frames")
        self.names = list(names)
        self.ir, self.vis, self.mask, self.label = ir.contiguous(), vis.contiguous(), mask.contiguous(), label.contiguous()
        self.shape = (H, W)

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_arrays(cls, names, ir, vis, mask, label, device="cuda"):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(device)
        return cls(names, up(ir), up(vis), up(mask), up(label))

    @classmethod
    def from_folder(cls, folder, device="cuda"):
        items = [folder[i] for i in range(len(folder))]
        stack_same_size(items)
        return cls.from_arrays([it[0] for it in items], *(np.stack([it[k] for it in items]) for k in (1, 2, 3, 4)), device=device)

    def augment(self, rec, tab, crop_h, crop_w, pick=True, want=None, tally=None, mix=None, paste=None):
        """rec (B, REC_WORDS), tab: host int32 arrays of pack_records -> (ir3, vis3, mask3, label, rec_dev).  One pinned,
        asynchronous upload, then the two kernels on the current stream.

        want: None, or a host (B, 2) integer array (class or -1, threshold) per sample.  It travels in the same upload and the
        pick step becomes ops.augment_pick_class (rare-class sampling, NOT the reference's loader); the result then ends with
        one more tensor, got (B,) int32.  tally: the (n_class, 2) int64 device tensor that step adds (drawn, hit) to.

        mix: None, or (table, n_class, min_pixels, tally): a host ClassMix table (ops.check_mix_table) that travels in the same
        upload.  The batch returned is then the MIXED one (ops.class_mix after apply; NOT the reference's loader) and the result
        ends with two more tensors, sel (B, 8) int32 and pasted (B,) int64; tally is class_mix's (n_class, 2) int64 or None.

        paste: None, or (table, bank, n_class, tally): a host copy-paste table (ops.check_paste_table) that travels in the same
        upload, and the ObjectBank its slots index.  The batch returned then has the objects pasted in (ops.copy_paste, after apply
        and after class_mix when both are on; NOT the reference's loader) and the result ends with one more tensor, the pasted
        pixels (B,) int64; tally is copy_paste's (n_class, 2) int64 or None."""
        from . import ops
        B = rec.shape[0]
        if paste is not None:
            paste_table, paste_bank, paste_classes, paste_tally = paste
            paste_table = ops.check_paste_table(paste_table, B)
        if mix is not None:
            mix_table, mix_classes, mix_min_pixels, mix_tally = mix
            mix_table = ops.check_mix_table(mix_table, B, mix_classes)
        if want is not None:
            if not pick:
                raise ValueError("augment: want belongs to the pick step (pick=True)")
            want = ops.check_want(want, B)
        words = rec.size + tab.size + (want.size if want is not None else 0)
        mix_at = words
        if mix is not None:
            words += mix_table.size
        paste_at = words
        if paste is not None:
            words += paste_table.size
        blob = self._staging(words)
        blob[:rec.size].copy_(torch.from_numpy(rec.reshape(-1)))
        blob[rec.size:rec.size + tab.size].copy_(torch.from_numpy(tab))
        if want is not None:
            blob[rec.size + tab.size:mix_at].copy_(torch.from_numpy(want.reshape(-1)))
        if mix is not None:
            blob[mix_at:paste_at].copy_(torch.from_numpy(mix_table.reshape(-1)))
        if paste is not None:
            blob[paste_at:words].copy_(torch.from_numpy(paste_table.reshape(-1)))
        dev = torch.empty(words, dtype=torch.int32, device=self.ir.device)
        dev.copy_(blob[:words], non_blocking=True)
        self._staged[self._turn][1].record()
        rec_d, tab_d = dev[:rec.size].view(B, REC_WORDS), dev[rec.size:rec.size + tab.size]
        extra = (rec_d,)
        if want is not None:
            extra += (ops.augment_pick_class(self.label, rec_d, tab_d, crop_h, crop_w, dev[rec.size + tab.size:mix_at].view(B, 2), tally),)
        elif pick:
            ops.augment_pick(self.label, rec_d, tab_d, crop_h, crop_w)
        out = ops.augment_apply(self.ir, self.vis, self.mask, self.label, rec_d, tab_d, crop_h, crop_w)
        if mix is not None:
            mixed = ops.class_mix(*out, dev[mix_at:paste_at].view(B, 2 + mix_classes), mix_classes, mix_min_pixels, mix_tally)
            out, extra = mixed[:4], extra + mixed[4:]
        if paste is not None:
            done = ops.copy_paste(*out, paste_bank, dev[paste_at:words].view(paste_table.shape), paste_classes, paste_tally)
            out, extra = done[:4], extra + done[4:]
        return out + extra

    def label_stats(self, n_class=9, ignore_index=255):
        """-> LabelStats of the resident labels: one launch (csrc/label_stats.hip) and one readback, then cached.  Raises
        ValueError for a label that is neither below n_class nor ignore_index."""
        from . import ops
        if not hasattr(self, "_label_counts"):
            self._label_counts = ops.label_stats(self.label).cpu().numpy()
        return LabelStats(self._label_counts, self.names, n_class, ignore_index)

    def _staging(self, words):
        """Two pinned buffers used in turn; a buffer is rewritten only after the copy that last read it has completed."""
        if not hasattr(self, "_staged"):
            self._staged, self._turn = [None, None], 0
        self._turn ^= 1
        slot = self._staged[self._turn]
        if slot is None or slot[0].numel() < words:
            if slot is not None:
                slot[1].synchronize()
            slot = [torch.empty(max(words, 1 << 18), dtype=torch.int32).pin_memory(), torch.cuda.Event()]
            self._staged[self._turn] = slot
        else:
            slot[1].synchronize()
        return slot[0]


def stack_same_size(items):
    """Raises unless every (name, ir, vis, mask, label) item has the size of the first."""
    h, w = items[0][1].shape
    for name, ir, vis, mask, label in items:
        for a, what in ((ir, "infrared"), (vis, "visible"), (mask, "mask"), (label, "label")):
            if a.shape[:2] != (h, w):
                raise RuntimeError(f"DeviceDataset holds frames of ONE size: {name} has a {a.shape[0]} x {a.shape[1]} {what} image, "
                                   f"{items[0][0]} is {h} x {w}.  Resize the set, or split it by size into several data sets.")


# ------------------------------------------------------------------------------------------------------------ class balance

RULES = ("inverse", "median", "enet")


class LabelStats:
    """Class statistics of a label set, from the (N, 257) int64 count table of ops.label_stats (a host array): what class
    weights and rare-class sampling are computed from.  None of it is the reference's.

    counts (N, K): pixels of class c in frame n; pixels (K,): per class over the set; frames (K,): frames holding at least one
    pixel of the class; freq (K,): pixels / pixels.sum(); valid (N,): labelled (non-ignore) pixels per frame."""

    def __init__(self, counts, names, n_class=9, ignore_index=255):
        counts = np.asarray(counts)
        if counts.ndim != 2 or counts.shape[1] != 257 or counts.dtype.kind not in "iu" or len(names) != counts.shape[0]:
            raise ValueError(f"LabelStats: counts must be an (N, 257) integer table with one name per row, got {counts.dtype} {counts.shape}")
        if not 1 <= n_class <= 255:
            raise ValueError(f"LabelStats: n_class {n_class} outside 1..255")
        bad = counts > 0
        bad[:, :n_class] = False
        if 0 <= ignore_index <= 255:
            bad[:, ignore_index] = False
        if bad.any():
            n = int(np.argmax(bad.any(axis=1)))
            v = int(np.argmax(bad[n]))
            raise ValueError(f"label_stats: frame {n} ({names[n]}) holds {int(counts[n, v])} pixels of "
                             + (f"value {v}" if v < 256 else "values outside 0..255")
                             + f", which is neither a class below {n_class} nor the ignore index {ignore_index}")
        self.names, self.n_class, self.ignore_index = list(names), n_class, ignore_index
        self.counts = counts[:, :n_class].astype(np.int64)
        self.pixels = self.counts.sum(axis=0)
        self.frames = (self.counts > 0).sum(axis=0)
        self.valid = self.counts.sum(axis=1)
        total = int(self.pixels.sum())
        self.freq = self.pixels / float(total) if total else np.zeros(n_class, dtype=np.float64)

    def table(self):
        """-> printable rows: a header, then class, pixels, share of the labelled pixels and frames per class"""
        rows = [f"{'class':>5} {'pixels':>14} {'share':>9} {'frames':>7}  of {len(self.names)} frames, {int(self.valid.sum())} labelled pixels"]
        for c in range(self.n_class):
            rows.append(f"{c:>5} {int(self.pixels[c]):>14} {self.freq[c]:>9.6f} {int(self.frames[c]):>7}")
        return rows

    def class_weights(self, rule):
        """-> (K,) float64 weights for weighted cross entropy; a class without a pixel gets 0.
        inverse: 1 / f_c, divided by the mean of 1 / f over the present classes.
        median:  median-frequency balancing (Eigen and Fergus 2015): phi_c = pixels_c / (labelled pixels of the frames that hold
                 c), w_c = median(phi over the present classes) / phi_c.
        enet:    1 / ln(1.02 + f_c) (Paszke et al. 2016)."""
        if rule not in RULES:
            raise ValueError(f"class_weights: rule {rule!r} is not one of {', '.join(RULES)}")
        present = self.pixels > 0
        w = np.zeros(self.n_class, dtype=np.float64)
        if not present.any():
            return w
        f = self.freq[present]
        if rule == "inverse":
            inv = 1.0 / f
            w[present] = inv / inv.mean()
        elif rule == "median":
            held = ((self.counts > 0) * self.valid[:, None]).sum(axis=0)[present]
            phi = self.pixels[present] / held.astype(np.float64)
            w[present] = np.median(phi) / phi
        else:
            w[present] = 1.0 / np.log(1.02 + f)
        return w


class RareClassSampler:
    """Rare-class sampling as DAFormer defines it (Hoyer et al. 2022); NOT the reference's loader, which walks its slice front
    to back.  P(c) is proportional to exp((1 - f_c) / temperature) over the classes that have a candidate frame, a frame of
    `indices` with MORE than min_pixels pixels of the class; f_c is the class's share of the whole table.  A sample is, with
    probability `fraction`, a class drawn from P and a frame drawn uniformly from that class's candidates, else the next frame of
    `indices` in order (that cursor moves for such samples only).  temperature, min_pixels and min_crop_ratio default to
    DAFormer's values; fraction is this project's.  Private generators: random.Random(seed), numpy RandomState(seed)."""

    def __init__(self, stats, indices, temperature=0.01, min_pixels=3000, min_crop_ratio=0.5, fraction=1.0, seed=0):
        if not temperature > 0 or min_pixels < 0 or not 0 <= min_crop_ratio or not 0.0 <= fraction <= 1.0:
            raise ValueError(f"RareClassSampler: temperature {temperature} > 0, min_pixels {min_pixels} >= 0, min_crop_ratio "
                             f"{min_crop_ratio} >= 0 and fraction {fraction} in [0, 1] are required")
        self.stats, self.indices = stats, [int(i) for i in indices]
        if not self.indices or min(self.indices) < 0 or max(self.indices) >= stats.counts.shape[0]:
            raise ValueError("RareClassSampler: indices must name frames of the statistics' table")
        self.temperature, self.min_pixels, self.min_crop_ratio, self.fraction = temperature, min_pixels, min_crop_ratio, fraction
        sub = stats.counts[self.indices]
        self.candidates = [[i for i, n in zip(self.indices, sub[:, c]) if n > min_pixels] for c in range(stats.n_class)]
        self.classes = [c for c in range(stats.n_class) if self.candidates[c]]
        self.dropped = [c for c in range(stats.n_class) if not self.candidates[c]]
        if not self.classes:
            raise ValueError(f"RareClassSampler: no class has a frame with more than {min_pixels} pixels of it: nothing to sample")
        z = (1.0 - stats.freq[self.classes].astype(np.float64)) / float(temperature)
        e = np.exp(z - z.max())
        self.prob = np.zeros(stats.n_class, dtype=np.float64)
        self.prob[self.classes] = e / e.sum()
        self._cum = np.cumsum(self.prob[self.classes])
        self._py, self._np = random.Random(seed), np.random.RandomState(seed)
        self._at = 0

    def crop_threshold(self, scaled_pixels, frame_pixels):
        """pixels of the wanted class a crop window must EXCEED: min_pixels * min_crop_ratio, scaled by the frame's resize"""
        return int(np.floor(self.min_pixels * self.min_crop_ratio * scaled_pixels / frame_pixels))

    def draw(self, n):
        """-> [(frame index, class or -1), ...]: -1 marks a sequential sample"""
        out = []
        for _ in range(n):
            if self._py.random() < self.fraction:
                k = min(int(np.searchsorted(self._cum, self._np.random_sample(), side="right")), len(self.classes) - 1)
                c = self.classes[k]
                frames = self.candidates[c]
                out.append((frames[self._py.randrange(len(frames))], c))
            else:
                out.append((self.indices[self._at], -1))
                self._at = (self._at + 1) % len(self.indices)
        return out


class ClassMix:
    """The policy of ClassMix (Olsson et al. 2021; the mixing step of DAFormer, Hoyer et al. 2022) for AugmentedBatches(mix=);
    NOT the reference's loader, which mixes nothing.  With probability `prob` a sample receives, from ANOTHER sample of its own
    batch, the pixels of half of the classes present in that donor's crop (classes="half": those with more than min_pixels
    pixels, (n + n % 2) / 2 of them, chosen by a random permutation) or, with classes="wanted", of the one class the rare-class
    sampler drew the donor for (the half rule for a donor drawn in order).  What differs from DAFormer: both samples are labelled
    (there the receiver is a target-domain image with pseudo-labels), the probability is `prob` (there every sample is mixed;
    the default 0.5 is this project's choice), and the donor comes from the same batch.  The rule itself: include/segmif_hip.h.

    draw(B, wanted) builds the table from a private random.Random seeded from (seed, rank); neither the global generators nor the
    loader's crop generators are touched.  Per sample, in order, it draws random() < prob, a donor uniform over the other B - 1
    samples and a permutation of the classes - all three always, so the stream does not depend on the outcomes."""

    CLASSES = ("half", "wanted")

    def __init__(self, prob=0.5, classes="half", min_pixels=0, n_class=9, seed=0, rank=0):
        if classes not in self.CLASSES:
            raise ValueError(f"ClassMix: classes {classes!r} is not one of {', '.join(self.CLASSES)}")
        if not 0.0 < prob <= 1.0 or min_pixels < 0 or not 1 <= n_class <= 255:
            raise ValueError(f"ClassMix: prob {prob} in (0, 1], min_pixels {min_pixels} >= 0 and n_class {n_class} in 1..255 are required")
        self.prob, self.classes, self.min_pixels, self.n_class, self.seed, self.rank = prob, classes, int(min_pixels), n_class, seed, rank
        self._py = random.Random(f"ClassMix {seed} {rank}")

    def draw(self, B, wanted=None):
        """-> (B, 2 + n_class) int32 rows (donor, force, keys); donor == the sample itself marks one that is not mixed.
        wanted: per sample the class the sampler drew it for, or -1 (classes="wanted" only)."""
        if B < 2:
            raise ValueError(f"ClassMix: mixing needs two samples, the batch holds {B}")
        if self.classes == "wanted" and (wanted is None or len(wanted) != B):
            raise ValueError("ClassMix: classes='wanted' needs the class each sample was drawn for (a RareClassSampler)")
        table = np.empty((B, 2 + self.n_class), dtype=np.int32)
        for b in range(B):
            mixes = self._py.random() < self.prob
            j = self._py.randrange(B - 1)
            donor = j if j < b else j + 1
            keys = list(range(self.n_class))
            self._py.shuffle(keys)
            force = -1
            if self.classes == "wanted" and 0 <= int(wanted[donor]) < self.n_class:
                force = int(wanted[donor])
            table[b, 0], table[b, 1], table[b, 2:] = (donor if mixes else b), force, keys
        return table


class StrongAugment:
    """The policy of the student's strong augmentation in self-training (DAFormer's strong_transform, Hoyer et al. 2022: colour
    jitter, then a Gaussian blur) for SelfTrainingStep(strong=); NOT the reference's training.  The constants are DAFormer's:
    jitter with probability 0.8, brightness, contrast and saturation factors in [1 - 0.2, 1 + 0.2], a hue shift in [-0.2, 0.2], a
    blur with probability 0.5 whose sigma is uniform over [0.15, 1.15].  The formulas are this project's (include/segmif_hip.h,
    segmif_strong_augment_f32): the four jitter operations in a fixed order, and taps from ops.strong_taps instead of a kernel
    size that follows the image's.

    draw(B) builds the table from a private random.Random seeded from (seed, rank); neither the global generators nor the
    loaders' are touched.  Per sample, in order, all seven values are always drawn - a coin, fb, fc, fs ~ U(1 - strength,
    1 + strength), fh ~ U(-hue, hue), a coin, sigma ~ U(sigma) - so the stream does not depend on the outcomes."""

    def __init__(self, jitter_prob=0.8, strength=0.2, hue=0.2, blur_prob=0.5, sigma=(0.15, 1.15), seed=0, rank=0):
        lo, hi = (float(s) for s in sigma)
        if not (0.0 <= jitter_prob <= 1.0 and 0.0 <= blur_prob <= 1.0 and 0.0 <= strength <= 1.0 and 0.0 <= hue <= 0.5 and 0.0 < lo <= hi <= 2.0):
            raise ValueError(f"StrongAugment: jitter_prob {jitter_prob} and blur_prob {blur_prob} in [0, 1], strength {strength} in [0, 1], "
                             f"hue {hue} in [0, 0.5] and 0 < sigma {lo} <= {hi} <= 2 are required")
        self.jitter_prob, self.strength, self.hue, self.blur_prob, self.sigma = float(jitter_prob), float(strength), float(hue), float(blur_prob), (lo, hi)
        self.seed, self.rank = seed, rank
        self._py = random.Random(f"StrongAugment {seed} {rank}")

    def draw(self, B):
        """-> (B,) records of ops.strong_rec_dtype(); a sample whose coins both fail is copied"""
        from . import ops
        if B < 1:
            raise ValueError(f"StrongAugment: B {B} < 1")
        table = np.zeros(B, dtype=ops.strong_rec_dtype())
        u = self._py.uniform
        for b in range(B):
            jitter = self._py.random() < self.jitter_prob
            fb, fc, fs = (u(1.0 - self.strength, 1.0 + self.strength) for _ in range(3))
            fh = u(-self.hue, self.hue)
            blur = self._py.random() < self.blur_prob
            radius, taps = ops.strong_taps(u(*self.sigma))
            table["jitter_on"][b] = int(jitter)
            table["fb"][b], table["fc"][b], table["fs"][b], table["fh"][b] = (fb, fc, fs, fh) if jitter else (1.0, 1.0, 1.0, 0.0)
            table["radius"][b] = radius if blur else 0
            table["taps"][b] = taps if blur else [1.0] + [0.0] * ops.STRONG_MAX_RADIUS
        return table


# ---------------------------------------------------------------------------------------------------------------- copy-paste

class ObjectBank:
    """The objects of a resident set for instance copy-paste (Ghiasi et al. 2021; the rule: include/segmif_paste.h); NOT the
    reference's loader.  An object is one connected component of one class in one frame.  The bank is
      records_host  (M, 8) int32 rows {frame, root, cls, area, x0, y0, bw, bh}, sorted by (frame, root); records: the same on the device
      offsets_host  (M + 1,) int64: the objects' first pixels in the store; offsets: the same on the device
      patches       (offsets[M], 8) uint8 on the device: per pixel of an object's box {ir, v0, v1, v2, mask, alpha, 0, 0}
      by_class      {class: indices of its objects, ascending}
    and depends on the data alone: the kernels' append order is sorted away."""

    def __init__(self, records, offsets, patches, n_class, shape, device_records=None, device_offsets=None):
        self.records_host = np.ascontiguousarray(records, dtype=np.int32)
        self.offsets_host = np.ascontiguousarray(offsets, dtype=np.int64)
        M = len(self.records_host)
        if self.records_host.ndim != 2 or self.records_host.shape[1] != 8 or M < 1 or self.offsets_host.shape != (M + 1,):
            raise ValueError(f"ObjectBank: records {self.records_host.shape} and offsets {self.offsets_host.shape} do not describe a bank")
        self.patches, self.n_class, self.shape = patches, int(n_class), tuple(shape)
        self.records = device_records if device_records is not None else torch.from_numpy(self.records_host).to(patches.device)
        self.offsets = device_offsets if device_offsets is not None else torch.from_numpy(self.offsets_host).to(patches.device)
        cls = self.records_host[:, 2]
        self.by_class = {int(c): np.flatnonzero(cls == c) for c in np.unique(cls)}

    def __len__(self):
        return len(self.records_host)

    @property
    def nbytes(self):
        return int(self.patches.numel() + self.records.numel() * 4 + self.offsets.numel() * 8)

    def table(self):
        """-> printable rows: a header, then class, objects, their pixels (area) and their boxes' pixels (what the store holds)"""
        rows = [f"{'class':>5} {'objects':>8} {'pixels':>12} {'box pixels':>12}  of {len(self)} objects, {self.nbytes} bytes on the device"]
        box = self.records_host[:, 6].astype(np.int64) * self.records_host[:, 7]
        for c, idx in sorted(self.by_class.items()):
            rows.append(f"{c:>5} {len(idx):>8} {int(self.records_host[idx, 3].sum()):>12} {int(box[idx].sum()):>12}")
        return rows

    @classmethod
    def build(cls, dataset, n_class=9, classes=None, connectivity=8, min_area=64, max_box=None, max_per_class=4096, max_bytes=1 << 30,
              frames=None, max_workspace_bytes=256 << 20):
        """Walks the resident labels of `frames` (None: all; else frame indices) in chunks bounded by the labeller's workspace,
        labels them (utils.objects.connected_components), appends the boxes (ops.object_boxes) and, after ONE readback and the
        sort by (frame, root), fills the patch store (ops.object_pack); the root maps are freed afterwards.
        classes: None means 1..n_class-1 (class 0 is the background and is never banked by default).  min_area: least pixels of
        an object.  max_box: most pixels of its box, None means H * W // 4.  A class with more than max_per_class objects keeps
        every ceil(n / max_per_class)-th of the sorted order.  ValueError: an empty bank, or a store over max_bytes.
        Peak device memory beside the data set: the chunking bounds the labeller's and the boxes' WORKSPACE only (at most
        max_workspace_bytes, and 20 bytes per pixel of a chunk); the root maps of ALL the frames, 4 bytes per pixel, live from the
        labelling to the pack, since the pack needs them after the sort (1.9 GB for 1 569 frames of 480 x 640), one chunk's int32
        copy of its labels at a time beside them, then the record list and the store itself.
        The defaults are this project's choices; Ghiasi et al. bank every annotated instance."""
        from . import _lib, ops
        from .utils.objects import connected_components
        H, W = dataset.shape
        K = int(n_class)
        if not 1 <= K <= 32:
            raise ValueError(f"ObjectBank: n_class {n_class}, the kernels take 1..32 (SEGMIF_EINVAL)")
        wanted = sorted(set(int(c) for c in (range(1, K) if classes is None else classes)))
        if not wanted or wanted[0] < 0 or wanted[-1] >= K:
            raise ValueError(f"ObjectBank: classes {list(wanted)} must name at least one class in 0..{K - 1}")
        max_box = H * W // 4 if max_box is None else int(max_box)
        if min_area < 1 or max_box < 1 or max_per_class < 1:
            raise ValueError(f"ObjectBank: min_area {min_area}, max_box {max_box} and max_per_class {max_per_class} must be >= 1")
        idx = sorted(set(int(f) for f in (range(len(dataset)) if frames is None else frames)))
        if not idx or idx[0] < 0 or idx[-1] >= len(dataset):
            raise ValueError(f"ObjectBank: frames must name frames of the data set (0..{len(dataset) - 1})")
        mask_bits = sum(1 << c for c in wanted)
        per_frame = int(_lib.load().segmif_object_workspace_bytes(1, H, W))
        step = max(1, min(int(max_workspace_bytes) // max(per_frame, 1), _lib.PASTE_MAX_FRAMES))
        chunks, start = [], 0  # (first frame, frames): consecutive frames only, so that frame0 + index names the frame
        for i in range(1, len(idx) + 1):
            if i == len(idx) or idx[i] != idx[i - 1] + 1 or i - start == step:
                chunks.append((idx[start], i - start))
                start = i
        dev = dataset.label.device
        roots = [connected_components(dataset.label[f0:f0 + n].to(torch.int32), K, connectivity)[0] for f0, n in chunks]
        capacity, count = 1 << 16, None
        while count is None or count > capacity:
            capacity = capacity if count is None else count
            records, counter, work = torch.empty((capacity, 8), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), None
            for (f0, n), root in zip(chunks, roots):
                work = ops.object_boxes(root, dataset.label[f0:f0 + n], K, mask_bits, min_area, max_box, records, counter, frame0=f0,
                                        workspace=work)
            host = torch.cat([counter, records.reshape(-1)]).cpu().numpy()  # the one readback (repeated only after an overflow)
            count = int(host[0])
        rec = host[1:1 + 8 * count].reshape(count, 8)
        rec = rec[np.lexsort((rec[:, 1], rec[:, 0]))]
        keep = np.zeros(count, dtype=bool)
        for c in np.unique(rec[:, 2]):
            of_c = np.flatnonzero(rec[:, 2] == c)
            keep[of_c[::-(-len(of_c) // int(max_per_class))]] = True  # every ceil(n / max_per_class)-th
        rec = np.ascontiguousarray(rec[keep])
        if not len(rec):
            raise ValueError(f"ObjectBank: no object of classes {wanted} with at least {min_area} pixels and a box of at most {max_box} "
                             f"in {len(idx)} frames: nothing to paste (min_area, max_box, classes)")
        offsets = np.concatenate(([0], np.cumsum(rec[:, 6].astype(np.int64) * rec[:, 7]))).astype(np.int64)
        nbytes = int(offsets[-1]) * 8
        if nbytes > max_bytes:
            raise ValueError(f"ObjectBank: the patch store of {len(rec)} objects holds {int(offsets[-1])} pixels = {nbytes} bytes, over "
                             f"max_bytes {max_bytes}; raise min_area ({min_area}), lower max_box ({max_box}) or max_per_class "
                             f"({max_per_class}), name fewer classes or frames, or raise max_bytes")
        rec_d, off_d = torch.from_numpy(rec).to(dev), torch.from_numpy(offsets).to(dev)
        patches = torch.empty((int(offsets[-1]), 8), dtype=torch.uint8, device=dev)
        for (f0, n), root in zip(chunks, roots):
            m0, m1 = (int(v) for v in np.searchsorted(rec[:, 0], [f0, f0 + n]))
            if m1 > m0:  # (sorted by frame: a chunk's objects are consecutive)
                ops.object_pack(rec_d[m0:m1], off_d[m0:m1 + 1], patches, root, dataset.ir[f0:f0 + n], dataset.vis[f0:f0 + n],
                                dataset.mask[f0:f0 + n], frame0=f0)
        return cls(rec, offsets, patches, K, (H, W), rec_d, off_d)


class CopyPaste:
    """The policy of instance copy-paste (Ghiasi et al. 2021, "Simple Copy-Paste") for AugmentedBatches(paste=); NOT the reference's
    loader, which pastes nothing.  With probability `prob` a sample receives 1..max_objects objects of the bank, each of a drawn
    class (uniform over the banked classes, or with stats= a LabelStats the rare-class sampler's P(c) ~ exp((1 - f_c) /
    temperature)), uniform among that class's objects, scaled by a log-uniform factor in `scale` (nearest neighbour, the object
    only), mirrored with probability 1 / 2 when flip, its centre uniform over the crop.  What differs from Ghiasi et al.: no
    large-scale jitter of the receiver beyond the loader's own, no blending of the edge, objects from the whole resident set and
    not from one other image.  Every default (prob 0.5, max_objects 3, scale (0.5, 2.0), temperature 0.01) is this project's choice.

    draw(B, h, w) builds the table from a private random.Random seeded from (seed, rank); neither the global generators nor the
    loader's crop generators are touched.  Per sample, in order, it draws the coin, the number of objects and per slot a class, an
    object, a scale, a flip coin and two positions - all 2 + 6 * max_objects values always, each ONE call of random(), so the
    stream does not depend on the outcomes."""

    DRAWS_PER_SLOT = 6

    def __init__(self, bank, prob=0.5, max_objects=3, scale=(0.5, 2.0), flip=True, stats=None, temperature=0.01, seed=0, rank=0):
        from . import ops
        lo, hi = (float(v) for v in scale)
        if not 0.0 < prob <= 1.0 or not 1 <= max_objects <= ops.PASTE_MAX_SLOTS or not 0.0 < lo <= hi or not temperature > 0:
            raise ValueError(f"CopyPaste: prob {prob} in (0, 1], max_objects {max_objects} in 1..{ops.PASTE_MAX_SLOTS}, 0 < scale {lo} <= {hi} "
                             f"and temperature {temperature} > 0 are required")
        self.bank, self.prob, self.max_objects, self.scale, self.flip = bank, float(prob), int(max_objects), (lo, hi), bool(flip)
        self.temperature, self.seed, self.rank = float(temperature), seed, rank
        self.classes = sorted(bank.by_class)
        if stats is None:
            p = np.full(len(self.classes), 1.0 / len(self.classes))
        else:
            if max(self.classes) >= stats.n_class:
                raise ValueError(f"CopyPaste: the bank holds class {max(self.classes)}, the statistics {stats.n_class} classes")
            z = (1.0 - stats.freq[self.classes].astype(np.float64)) / self.temperature
            e = np.exp(z - z.max())
            p = e / e.sum()
        self.class_prob = dict(zip(self.classes, (float(v) for v in p)))
        self._cum = np.cumsum(p)
        self._py = random.Random(f"CopyPaste {seed} {rank}")

    def draws_per_sample(self):
        """calls of random() per sample, whatever the coins show"""
        return 2 + self.DRAWS_PER_SLOT * self.max_objects

    @staticmethod
    def _pick(r, n):
        """r in [0, 1) -> an index in 0..n-1"""
        return min(int(r * n), n - 1)

    def draw(self, B, h, w):
        """-> (B, max_objects, 8) int32 slots (obj, dx, dy, ow, oh, sx, sy, flip); obj = -1 marks an empty slot"""
        from . import ops
        if B < 1 or h < 1 or w < 1:
            raise ValueError(f"CopyPaste: B {B}, h {h} and w {w} must be >= 1")
        table = np.zeros((B, self.max_objects, 8), dtype=np.int32)
        table[:, :, 0] = -1
        rnd, rec = self._py.random, self.bank.records_host
        log_lo, log_hi = np.log(self.scale[0]), np.log(self.scale[1])
        for b in range(B):
            pastes = rnd() < self.prob
            n = 1 + self._pick(rnd(), self.max_objects)
            for k in range(self.max_objects):
                r_cls, r_obj, r_s, r_flip, r_x, r_y = (rnd() for _ in range(self.DRAWS_PER_SLOT))
                if not pastes or k >= n:
                    continue
                c = self.classes[min(int(np.searchsorted(self._cum, r_cls, side="right")), len(self.classes) - 1)]
                of_c = self.bank.by_class[c]
                obj = int(of_c[self._pick(r_obj, len(of_c))])
                s = float(np.exp(log_lo + r_s * (log_hi - log_lo)))
                bw, bh = int(rec[obj, 6]), int(rec[obj, 7])
                ow = min(max(int(round(bw * s)), 1), ops.PASTE_MAX_SIZE)
                oh = min(max(int(round(bh * s)), 1), ops.PASTE_MAX_SIZE)
                sx = min(max((bw << 16) // ow, 1), ops.PASTE_MAX_STEP)
                sy = min(max((bh << 16) // oh, 1), ops.PASTE_MAX_STEP)
                dx = -(ow // 2) + self._pick(r_x, w - ow + 2 * (ow // 2) + 1)
                dy = -(oh // 2) + self._pick(r_y, h - oh + 2 * (oh // 2) + 1)
                table[b, k] = (obj, dx, dy, ow, oh, sx, sy, int(self.flip and r_flip < 0.5))
        return table


# ------------------------------------------------------------------------------------------------------------------ iterator

class AugmentedBatches:
    """Endless iterator of `(names, ir3, vis3, mask3, label)`: ir3, vis3, mask3 (B, 3, crop, crop) float32 in NCHW (ir3 and
    mask3 are STORED with three channels: they are equal inside the image and differ in the padding, as random_crop2's are),
    label (B, crop, crop) int64 with 255 in the padding.

    Order: the rank's slice (segmif_amd.dist.shard) of the data set front to back, no shuffle, the last partial batch
    dropped (train.py:137-142); when the slice is used up it starts again (train.py:211-215).

    Randomness: a private random.Random(seed + rank) and numpy RandomState(seed + rank); the global generators are not
    touched.  The distributions are the reference's.  The STREAM is not: the reference stops drawing crop candidates at the
    first accepted one, this class always draws all ten (the kernel then keeps the first accepted), so the same seed gives
    other numbers while the distribution of the results is the same.

    photometric: any subset of ("brightness", "contrast"); saturation and hue are not available.
    aug=False: every frame whole, value / 255, no resize, flip, distortion or crop.

    sampler: None, or a RareClassSampler over this rank's slice.  The frames then come from sampler.draw and a sample drawn for
    a class keeps the first crop candidate with more than floor(min_pixels * min_crop_ratio * (nw * nh) / (w * h)) pixels of
    it (else the candidate with the most); last_params[i]["want"] is (class or -1, threshold), rcs_tally() the device's count
    of drawn / hit samples per class.  NOT the reference's loader.  With None nothing changes, the random stream included.

    mix: None, or a ClassMix.  Every batch is then mixed after augment_apply (ops.class_mix: classes of one crop pasted into
    another of the same batch); the crops underneath are the ones the same seed gives without it, since the policy draws from
    a generator of its own.  last_params[i]["mix"] is (donor, force, keys), mix_tally() the device's count of samples and pixels
    pasted per class.  NOT the reference's loader.  With None nothing changes: the random stream, the launches, the batches.

    paste: None, or a CopyPaste.  Every batch then has banked objects pasted in (ops.copy_paste) after augment_apply, and after
    class_mix when mix= is given too; the crops underneath are the ones the same seed gives without it, since the policy draws from
    a generator of its own.  last_params[i]["paste"] is the sample's slots, paste_tally() the device's count of slots and pixels
    pasted per class.  NOT the reference's loader.  With None nothing changes: the random stream, the launches, the batches."""

    def __init__(self, dataset, batch, crop_size=512, rescale_range=(0.5, 2.0), fliplr=True, photometric=PHOTOMETRIC, seed=0,
                 rank=0, world=1, aug=True, sampler=None, mix=None, paste=None):
        unknown = [p for p in photometric if p not in PHOTOMETRIC]
        if unknown:
            raise ValueError(f"photometric: {unknown} not available; this loader applies {PHOTOMETRIC} only (saturation and hue go "
                             "through OpenCV's HSV conversion in the reference and are left out)")
        if batch < 1 or crop_size < 1 or crop_size % 4:
            raise ValueError("batch must be positive and crop_size a positive multiple of 4")
        if rescale_range and not 0 < rescale_range[0] <= rescale_range[1]:
            raise ValueError(f"rescale_range {rescale_range}")
        if not aug and dataset.shape[1] % 4:
            raise ValueError(f"aug=False hands over whole frames through 16-byte stores: the frame width must be a multiple of 4, "
                             f"this data set's is {dataset.shape[1]}")
        self.dataset, self.batch, self.crop = dataset, batch, crop_size
        self.rescale_range, self.fliplr, self.photometric, self.aug = rescale_range, fliplr, tuple(photometric), aug
        self.indices = list(dist.shard(len(dataset), rank, world))
        if len(self.indices) < batch:
            raise RuntimeError(f"rank {rank} of {world} holds {len(self.indices)} frames, fewer than one batch of {batch}")
        self._py, self._np = random.Random(seed + rank), np.random.RandomState(seed + rank)
        self._at = 0
        self.last_params = None
        self.sampler = sampler
        if sampler is not None:
            if not aug:
                raise ValueError("sampler: rare-class sampling picks crops, aug=False has none")
            if list(sampler.indices) != self.indices:
                raise ValueError("sampler: built over other frames than this rank's slice of the data set "
                                 "(RareClassSampler(stats, list(dist.shard(len(dataset), rank, world)), ...))")
            self._tally = torch.zeros((sampler.stats.n_class, 2), dtype=torch.int64, device=dataset.label.device)
        self.mix = mix
        if mix is not None:
            if batch < 2:
                raise ValueError(f"mix: ClassMix pastes between the samples of a batch, batch {batch} has no second one")
            if not aug:
                raise ValueError("mix: ClassMix works on augmented crops, aug=False has none")
            if mix.classes == "wanted" and sampler is None:
                raise ValueError("mix: classes='wanted' pastes the class a RareClassSampler drew the donor for: give sampler=")
            if mix.rank != rank:
                raise ValueError(f"mix: the ClassMix was seeded for rank {mix.rank}, this iterator is rank {rank}")
            self._mix_tally = torch.zeros((mix.n_class, 2), dtype=torch.int64, device=dataset.label.device)
        self.paste = paste
        if paste is not None:
            if not aug:
                raise ValueError("paste: CopyPaste works on augmented crops, aug=False has none")
            if paste.rank != rank:
                raise ValueError(f"paste: the CopyPaste was seeded for rank {paste.rank}, this iterator is rank {rank}")
            self._paste_tally = torch.zeros((paste.bank.n_class, 2), dtype=torch.int64, device=dataset.label.device)

    def __len__(self):
        """batches per pass (drop_last)"""
        return len(self.indices) // self.batch

    def __iter__(self):
        return self

    def draw(self, n):
        h, w = self.dataset.shape
        if not self.aug:
            return [identity_params(h, w) for _ in range(n)]
        return [sample_params(self._py, self._np, h, w, self.crop, self.crop, self.rescale_range, self.fliplr, self.photometric)
                for _ in range(n)]

    def rcs_tally(self):
        """-> (n_class, 2) int64 numpy array: per class the samples drawn for it so far and those of them for which a candidate
        window passed the threshold.  One readback of the device tally."""
        if self.sampler is None:
            raise RuntimeError("rcs_tally: this iterator has no sampler")
        return self._tally.cpu().numpy()

    def mix_tally(self):
        """-> (n_class, 2) int64 numpy array: per class the samples that had it pasted in so far and the pixels pasted.  One
        readback of the device tally."""
        if self.mix is None:
            raise RuntimeError("mix_tally: this iterator has no ClassMix")
        return self._mix_tally.cpu().numpy()

    def paste_tally(self):
        """-> (n_class, 2) int64 numpy array: per class the non-empty slots drawn so far and the pixels pasted.  One readback of
        the device tally."""
        if self.paste is None:
            raise RuntimeError("paste_tally: this iterator has no CopyPaste")
        return self._paste_tally.cpu().numpy()

    def _paste_arg(self, params):
        """The augment(paste=) tuple of one batch, drawn from the policy's own generator; notes it in the samples' params."""
        if self.paste is None:
            return None
        table = self.paste.draw(len(params), self.crop, self.crop)
        for p, slots in zip(params, table):
            p["paste"] = tuple(tuple(int(v) for v in slot) for slot in slots)
        return table, self.paste.bank, self.paste.bank.n_class, self._paste_tally

    def _mix_arg(self, params, wanted=None):
        """The augment(mix=) tuple of one batch, drawn from the policy's own generator; notes it in the samples' params."""
        if self.mix is None:
            return None
        table = self.mix.draw(len(params), wanted)
        for p, row in zip(params, table):
            p["mix"] = (int(row[0]), int(row[1]), tuple(int(k) for k in row[2:]))
        return table, self.mix.n_class, self.mix.min_pixels, self._mix_tally

    def _next_sampled(self):
        """One batch whose frames (and wanted classes) come from the sampler; the crop parameters are drawn as ever."""
        drawn = self.sampler.draw(self.batch)
        idx = [i for i, _ in drawn]
        self.last_params = params = self.draw(len(idx))
        h, w = self.dataset.shape
        want = np.zeros((len(idx), 2), dtype=np.int32)
        for b, ((_, c), p) in enumerate(zip(drawn, params)):
            # the crop is cut after the random rescale: the threshold scales with the frame's area
            want[b] = (c, self.sampler.crop_threshold(p["nw"] * p["nh"], w * h)) if c >= 0 else (-1, 0)
            p["want"] = (int(want[b, 0]), int(want[b, 1]))
        rec, tab = pack_records(idx, params, h, w)
        out = self.dataset.augment(rec, tab, self.crop, self.crop, pick=True, want=want, tally=self._tally,
                                   mix=self._mix_arg(params, [c for _, c in drawn]), paste=self._paste_arg(params))[:4]
        return (tuple(self.dataset.names[i] for i in idx),) + tuple(out)

    def __next__(self):
        if self.sampler is not None:
            return self._next_sampled()
        if self._at + self.batch > len(self.indices):  # drop_last, then a fresh pass
            self._at = 0
        idx = self.indices[self._at:self._at + self.batch]
        self._at += self.batch
        self.last_params = params = self.draw(len(idx))
        return (tuple(self.dataset.names[i] for i in idx),) + tuple(self._device_step(idx, params))

    def _device_step(self, idx, params):
        h, w = self.dataset.shape
        rec, tab = pack_records(idx, params, h, w)
        ch, cw = (self.crop, self.crop) if self.aug else (h, w)
        return self.dataset.augment(rec, tab, ch, cw, pick=self.aug, mix=self._mix_arg(params), paste=self._paste_arg(params))[:4]
