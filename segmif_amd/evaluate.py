"""A data set end to end: uint8 frames in, fused uint8 images, label maps, mIoU and the fusion-quality scores out
(test_fusion.py:83-126 followed by test_segmentation.py:160-195 and util/util.py:8-29, in memory and on the device).

    python -m segmif_amd.evaluate --ir DIR --vis DIR --mask DIR [--label DIR] --out DIR [--backbone mit_b3]
        [--seg-ckpt F] [--fusion-ckpt F] [--batch N] [--json F] [--structural-scores]
        [--ms-scales S [S ...]] [--flip] [--size-divisor N]
        [--boundary-scores [--boundary-width D] [--bf-tolerance T] [--boundary-ratio R] [--bf-ratio R]]
        [--calibration [--calibration-bins M] [--calibration-temperatures T [T ...]] [--calibration-thresholds TAU [TAU ...]]]
        [--object-scores [--object-connectivity {4,8}] [--object-size-edges A [B [C]]] [--object-coverage TAU]]

reads the sorted file names of --vis (TaskFusion_dataset2.py:40-48) from every folder (.npy always, .png when PIL imports),
and writes OUT/Fused/NAME, OUT/Seg/NAME (palette rendering) and a JSON of the results.  --structural-scores adds Qabf, SSIM and
VIF (utils/fusion_metrics.structural_scores; images of at least 41 x 41) to the JSON and to the summary line.  --ms-scales and
--flip (alone: scales 1.0) take the labels, and so the mIoU, from multi-scale + flip inference (segmif_amd.tta; the JSON then
names the views under "tta"); the fused images and their scores do not change.  --boundary-scores (with --label) adds the
contour scores of the label maps: Boundary IoU, the trimap-band mIoU and the boundary F-score (utils/metrics.boundary_scores;
the JSON names the widths under "boundary"); the widths follow the frame's diagonal unless --boundary-width / --bf-tolerance
give them in pixels.  --calibration (with --label) scores the softmax confidence instead of the labels: reliability table, ECE,
MCE, NLL and Brier score for a list of temperatures, coverage and precision above confidence thresholds, and the temperature of the
list with the lowest NLL (utils/calibration.calibration_scores; the JSON names the settings under "calibration").  Not with
--ms-scales / --flip.  --object-scores (with --label) adds the object-level scores of the label maps: the share of the ground
truth's connected components of each class that the prediction covers to at least --object-coverage (default 0.5), the share of the
prediction's components that the ground truth covers, their F1, and the same by size bucket (utils/objects.object_scores; the JSON
names the settings under "objects").  On seeded weights the figures mean nothing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import _lib
from .pipeline import PairForward
from .tta import TTA
from .utils.fusion_metrics import (MFNET_PALETTE, SCORE_NAMES, STRUCTURAL_SCORE_NAMES, colorize, fusion_scores, fusion_stats,
                                   structural_scores, structural_stats)
from .utils.calibration import CalibrationTable, calibration_scores, calibration_stats, table_settings
from .utils.objects import DEFAULT_SIZE_EDGES, ObjectTable, coverage_decile, object_scores, object_stats
from .utils.metrics import (_dev, _stream, boundary_scores, boundary_stats, boundary_widths, compute_results,
                            confusion_matrix)


def _dequantize(u8_nhwc):
    """(B, H, W, C) uint8 -> (B, C, H, W) fp32 = u / 255 (segmif_dequantize_u8: the loaders' float32 array / 255.0)"""
    B, H, W, C = u8_nhwc.shape
    out = torch.empty((B, C, H, W), device=u8_nhwc.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_dequantize_u8(u8_nhwc.data_ptr(), out.data_ptr(), B, C, H * W, _stream()), "segmif_dequantize_u8")
    return out


def _nanmean(x):
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


class Evaluator:
    """Accumulates the evaluation of (infrared, visible, mask) uint8 batches through PairForward(uint8_roundtrip=True,
    return_u8=True): the min-max rescale of the fused image is per call = per batch, as the reference's is.  structural=True also
    gathers Qabf, SSIM and VIF (STRUCTURAL_SCORE_NAMES) of every pair.  tta: a segmif_amd.tta.TTA - the labels (and the mIoU)
    come from multi-scale + flip inference (PairForward(tta=)); not with graph=True.  boundary: None, or a dict with any of d,
    theta (widths in pixels) and ratio, bf_ratio (utils/metrics.boundary_widths; a width not given follows the frame's
    diagonal) - the contour tables of utils/metrics.boundary_stats are then summed over every labelled batch.  calibration: None, or a
    dict with any of bins (default 15 equal ones), temperatures (default utils/calibration.DEFAULT_TEMPERATURES) and thresholds
    (default (0.968,)) - one utils/calibration.CalibrationTable is then summed over every labelled batch on the device, from the
    logits PairForward(return_logits=True) hands out; nothing is read back per batch.  Not with tta= (the vote's probabilities are
    not logits: not built).  objects: None, or a dict with any of connectivity (default 8), size_edges (default
    utils/objects.DEFAULT_SIZE_EDGES) and coverage (default 0.5) - one utils/objects.ObjectTable is then summed over every labelled
    batch on the device; nothing is read back per batch.  It reads the label maps only, so it works with graph=True and tta= alike."""

    def __init__(self, seg_net, fusion_net, n_class=9, graph=False, structural=False, tta=None, boundary=None, calibration=None,
                 objects=None):
        if tta is not None and graph:
            raise NotImplementedError("Evaluator: graph=True cannot capture the multi-size forward (tta=)")
        if calibration is not None and tta is not None:
            raise NotImplementedError("Evaluator: calibration= with tta=: the vote averages probabilities over views, which are not "
                                      "logits; calibration of the voted probabilities is not built")
        if calibration is not None and set(calibration) - {"bins", "temperatures", "thresholds"}:
            raise ValueError(f"Evaluator: calibration= takes bins, temperatures and thresholds, got {sorted(calibration)}")
        if objects is not None and set(objects) - {"connectivity", "size_edges", "coverage"}:
            raise ValueError(f"Evaluator: objects= takes connectivity, size_edges and coverage, got {sorted(objects)}")
        self.objects = None if objects is None else dict(objects)
        self._objects = None         # the ObjectTable of sums on the device, from the first labelled batch on
        if objects is not None:      # (the settings' own checks, before any batch)
            self._objects_kw = dict(n_class=n_class, connectivity=self.objects.get("connectivity", 8),
                                    size_edges=tuple(self.objects.get("size_edges", DEFAULT_SIZE_EDGES)))
            self._objects_coverage = float(self.objects.get("coverage", 0.5))
            coverage_decile(self._objects_coverage)
            ObjectTable.zeros("cpu", **self._objects_kw)
        self.calibration = None if calibration is None else dict(calibration)
        self._calibration = None     # the CalibrationTable on the device, from the first labelled batch on
        if calibration is not None:  # (the settings' own checks, before any batch)
            self._calibration_kw = table_settings(**self.calibration)
            CalibrationTable.zeros("cpu", **self._calibration_kw)
        self.pair = PairForward(seg_net, fusion_net, uint8_roundtrip=True, return_u8=True, tta=tta, return_logits=calibration is not None)
        self.tta = tta
        self._frame = None
        self.n_class = n_class
        self.graph = graph
        self._graph_shape = None
        self._conf = None
        self._scores = []
        self.structural = structural
        self._structural = []
        if boundary is not None and set(boundary) - {"d", "theta", "ratio", "bf_ratio"}:
            raise ValueError(f"Evaluator: boundary= takes d, theta, ratio and bf_ratio, got {sorted(boundary)}")
        self.boundary = None if boundary is None else dict(boundary)
        self._boundary = None        # (cls_total, trimap_total) on the device
        self._boundary_doc = None    # {"d", "theta", "frame"} of the first labelled batch

    def _boundary_update(self, labels, label):
        H, W = (int(v) for v in labels.shape[1:])
        d, theta = boundary_widths(H, W, self.boundary.get("ratio", 0.02), self.boundary.get("bf_ratio", 0.0075))
        d = d if self.boundary.get("d") is None else int(self.boundary["d"])
        theta = theta if self.boundary.get("theta") is None else int(self.boundary["theta"])
        doc = {"d": d, "theta": theta, "frame": [H, W]}
        if self._boundary_doc is None:
            self._boundary_doc = doc
            self._boundary = (torch.zeros((self.n_class, 8), device=labels.device, dtype=torch.int64),
                              torch.zeros((self.n_class, self.n_class), device=labels.device, dtype=torch.int64))
        elif doc != self._boundary_doc and (self.boundary.get("d") is None or self.boundary.get("theta") is None):
            raise RuntimeError(f"Evaluator: a batch of {H} x {W} frames after {self._boundary_doc['frame'][0]} x "
                               f"{self._boundary_doc['frame'][1]} ones, with boundary widths that follow the frame size: the scores would "
                               "mix bands; fix both widths (boundary=dict(d=, theta=), --boundary-width and --bf-tolerance)")
        boundary_stats(labels, label, self.n_class, d, theta, out=self._boundary)

    def update(self, ir_u8, vis_u8, mask_u8, label=None):
        """ir_u8 (B, H, W), vis_u8 (B, H, W, 3), mask_u8 (B, H, W) uint8 and optionally label (B, H, W) int64, all on the device
        -> (fused_u8 (B, H, W, 3) uint8, labels (B, H, W) int32) on the device.  With graph=True the first call captures the pair
        forward for its batch shape and later calls of that shape replay it."""
        ir_u8, vis_u8, mask_u8 = _dev(ir_u8, "ir_u8", torch.uint8), _dev(vis_u8, "vis_u8", torch.uint8), _dev(mask_u8, "mask_u8", torch.uint8)
        if vis_u8.dim() != 4 or vis_u8.shape[3] != 3 or ir_u8.shape != vis_u8.shape[:3] or mask_u8.shape != vis_u8.shape[:3]:
            raise RuntimeError(f"update expects ir (B, H, W), vis (B, H, W, 3), mask (B, H, W), got {tuple(ir_u8.shape)}, "
                               f"{tuple(vis_u8.shape)}, {tuple(mask_u8.shape)}")
        with torch.no_grad():
            ir = _dequantize(ir_u8.unsqueeze(3))
            vis = _dequantize(vis_u8)
            mask3 = _dequantize(mask_u8.unsqueeze(3)).repeat(1, 3, 1, 1)  # the grey plane three times (test_fusion.py:90-99)
            if self.graph:
                if self._graph_shape is None:
                    self.pair.capture(ir, vis, mask3)
                    self._graph_shape = tuple(vis.shape)
                if tuple(vis.shape) != self._graph_shape:
                    raise RuntimeError(f"the captured graph serves batches of shape {self._graph_shape}, got {tuple(vis.shape)}")
                out = self.pair.replay(ir, vis, mask3)
                labels, fused_u8 = out[1], out[2]
                fused_u8, labels = fused_u8.clone(), labels.clone()  # (the graph's output buffers are overwritten by the next replay)
                logits = out[3].clone() if self.calibration is not None else None
            else:
                out = self.pair.eager(ir, vis, mask3)
                labels, fused_u8 = out[1], out[2]
                logits = out[3] if self.calibration is not None else None
            self._frame = tuple(vis.shape[2:])
            self._scores.append(fusion_stats(fused_u8, vis_u8, ir_u8))
            if self.structural:
                self._structural.append(structural_stats(fused_u8, vis_u8, ir_u8))
            if label is not None:
                label = _dev(label, "label", torch.int64)
                self._conf = confusion_matrix(labels, label, self.n_class, out=self._conf)
                if self.boundary is not None:
                    self._boundary_update(labels.contiguous(), label.reshape(labels.shape))
                if self.calibration is not None:
                    self._calibration = calibration_stats(logits, label.reshape(labels.shape), out=self._calibration, **self._calibration_kw)
                if self.objects is not None:
                    if self._objects is None:
                        self._objects = ObjectTable.zeros(labels.device, **self._objects_kw)
                    object_stats(labels.contiguous(), label.reshape(labels.shape), out=self._objects, **self._objects_kw)
        return fused_u8, labels

    def results(self):
        """-> dict: every score of SCORE_NAMES as a per-image float64 array, 'mean' (name -> NaN-ignoring mean over the images)
        and, when labels were given, 'precision' / 'recall' / 'iou' per class (compute_results) and 'mIoU' =
        mean(nan_to_num(iou)), the figure test_segmentation.py prints for data that lack a class.  With structural=True the
        scores of STRUCTURAL_SCORE_NAMES are added in the same two places; with boundary= and labels, the keys of
        utils/metrics.boundary_scores; with calibration= and labels, the keys of utils/calibration.calibration_scores (one
        readback); with objects= and labels, the keys of utils/objects.object_scores (one readback)."""
        per = [fusion_scores(s) for s in self._scores]
        names = SCORE_NAMES
        if self.structural:
            per = [dict(p, **structural_scores(s)) for p, s in zip(per, self._structural)]
            names = SCORE_NAMES + STRUCTURAL_SCORE_NAMES
        out = {k: np.concatenate([p[k] for p in per]) if per else np.zeros(0) for k in names}
        out["mean"] = {k: _nanmean(out[k]) for k in names}
        if self._conf is not None:
            precision, recall, iou = compute_results(self._conf)
            out.update(precision=precision, recall=recall, iou=iou, mIoU=float(np.mean(np.nan_to_num(iou))))
        if self._boundary is not None:
            out.update(boundary_scores(*self._boundary))
        if self._calibration is not None:
            out.update(calibration_scores(self._calibration))
        if self._objects is not None:
            out.update(object_scores(self._objects, self._objects_coverage))
        return out

    def document(self, names, seeded_weights, res=None):
        """What the command line writes as JSON: the names, which networks ran on seeded weights, results() (or `res`, if the
        caller has them) with arrays as lists, - only with tta - its settings and the views of the last batch's frame size
        under "tta", - only with boundary= and labels - the widths and the frame size they were derived for under "boundary" and
        - only with calibration= and labels - the bins, temperatures and thresholds under "calibration" and - only with objects= and
        labels - the connectivity, size edges and coverage under "objects"."""
        doc = {"names": list(names), "seeded_weights": list(seeded_weights)}
        for k, v in (self.results() if res is None else res).items():
            doc[k] = v.tolist() if isinstance(v, np.ndarray) else v
        if self.tta is not None:
            if self._frame is None:
                raise RuntimeError("Evaluator.document: no batch has been evaluated, the views have no size yet")
            doc["tta"] = self.tta.describe(*self._frame)
        if self._boundary_doc is not None:
            doc["boundary"] = dict(self._boundary_doc)
        if self._calibration is not None:
            doc["calibration"] = self._calibration.settings()
        if self._objects is not None:
            doc["objects"] = dict(self._objects.settings(), coverage=self._objects_coverage)
        return doc


def _read(path):
    if path.endswith(".npy"):
        return np.load(path)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"{path}: reading images needs PIL; .npy arrays are always read")
    return np.array(Image.open(path))


def _write(path, arr):
    if path.endswith(".npy"):
        np.save(path, arr)
        return
    from PIL import Image
    Image.fromarray(arr).save(path)


def _names(folder):
    return sorted(f for f in os.listdir(folder) if f.lower().endswith((".npy", ".png")))


def _load_weights(net, path):
    sd = torch.load(path, map_location="cpu")
    net.load_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)


def parse_args(argv=None):
    """-> (args, tta): the parsed command line and the TTA it asks for (None without --ms-scales / --flip)."""
    ap = argparse.ArgumentParser(prog="python -m segmif_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--ir", required=True)
    ap.add_argument("--vis", required=True)
    ap.add_argument("--mask", required=True)
    ap.add_argument("--label")
    ap.add_argument("--out", required=True)
    ap.add_argument("--backbone", default="mit_b3")
    ap.add_argument("--seg-ckpt")
    ap.add_argument("--fusion-ckpt")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--json")
    ap.add_argument("--structural-scores", action="store_true",
                    help="also report Qabf, SSIM and VIF (one more device pass per batch; images of at least 41 x 41)")
    ap.add_argument("--ms-scales", type=float, nargs="+", metavar="S",
                    help="multi-scale inference: one forward per scale of the frame (SegFormer's protocol: 0.5 0.75 1.0 1.25 1.5 1.75)")
    ap.add_argument("--flip", action="store_true", help="also vote every scale's mirrored view (alone: scale 1.0)")
    ap.add_argument("--size-divisor", type=int, default=8, metavar="N", help="view sizes are rounded up to a multiple of N (default 8)")
    ap.add_argument("--boundary-scores", action="store_true",
                    help="also report Boundary IoU, the trimap-band mIoU and the boundary F-score of the label maps (needs --label)")
    ap.add_argument("--boundary-width", type=int, metavar="D", help="band half-width in pixels, 1..32 (default: --boundary-ratio x the diagonal)")
    ap.add_argument("--bf-tolerance", type=int, metavar="T", help="contour tolerance in pixels, 0..31 (default: --bf-ratio x the diagonal)")
    ap.add_argument("--boundary-ratio", type=float, metavar="R", help="band half-width as a share of the frame's diagonal (default 0.02)")
    ap.add_argument("--bf-ratio", type=float, metavar="R", help="contour tolerance as a share of the frame's diagonal (default 0.0075)")
    ap.add_argument("--calibration", action="store_true",
                    help="also score the softmax confidence: reliability table, ECE, MCE, NLL, Brier score and the temperature of lowest "
                         "NLL (needs --label; not with --ms-scales / --flip).  This project's addition, not the reference's evaluation")
    ap.add_argument("--calibration-bins", type=int, metavar="M", help="equal confidence bins, 1..32 (default 15)")
    ap.add_argument("--calibration-temperatures", type=float, nargs="+", metavar="T",
                    help="the temperatures scored, at most 16, each finite and > 0 (default: 1.0 and 15 log-spaced values over [0.5, 4])")
    ap.add_argument("--calibration-thresholds", type=float, nargs="+", metavar="TAU",
                    help="coverage and precision are reported above each, at most 8 in [0, 1] (default 0.968, self-training's)")
    ap.add_argument("--object-scores", action="store_true",
                    help="also report object-level recall, precision and F1 of the label maps' connected components, by class and by "
                         "size (needs --label).  This project's addition, not the reference's evaluation")
    ap.add_argument("--object-connectivity", type=int, choices=(4, 8), help="pixels join across edges (4) or edges and corners (8, the default)")
    ap.add_argument("--object-size-edges", type=int, nargs="+", metavar="A",
                    help="at most 3 ascending areas in pixels that separate the size buckets (default 1024 9216, COCO's)")
    ap.add_argument("--object-coverage", type=float, metavar="TAU",
                    help="an object counts as found when at least this share of it is covered: one of 0.1, 0.2 ... 1.0 (default 0.5)")
    args = ap.parse_args(argv)
    obj_given = [f for f, v in (("--object-connectivity", args.object_connectivity), ("--object-size-edges", args.object_size_edges),
                                ("--object-coverage", args.object_coverage)) if v is not None]
    if args.object_scores and not args.label:
        ap.error("--object-scores compares the label maps' objects with the ground truth's: it needs --label")
    if obj_given and not args.object_scores:
        ap.error(f"{', '.join(obj_given)} only with --object-scores")
    if args.object_scores:
        try:
            kw = object_settings(args)
            ObjectTable.zeros("cpu", 9, kw.get("connectivity", 8), kw.get("size_edges", DEFAULT_SIZE_EDGES))
            coverage_decile(kw.get("coverage", 0.5))
        except ValueError as e:
            ap.error(str(e))
    cal_given = [f for f, v in (("--calibration-bins", args.calibration_bins), ("--calibration-temperatures", args.calibration_temperatures),
                                ("--calibration-thresholds", args.calibration_thresholds)) if v is not None]
    if args.calibration and not args.label:
        ap.error("--calibration compares the confidence with the ground truth: it needs --label")
    if cal_given and not args.calibration:
        ap.error(f"{', '.join(cal_given)} only with --calibration")
    if args.calibration and (args.ms_scales is not None or args.flip):
        ap.error("--calibration with --ms-scales / --flip: the vote's probabilities are not logits; their calibration is not built")
    if args.calibration:
        try:
            CalibrationTable.zeros("cpu", **table_settings(**calibration_settings(args)))
        except ValueError as e:
            ap.error(str(e))
    given = [f for f, v in (("--boundary-width", args.boundary_width), ("--bf-tolerance", args.bf_tolerance),
                            ("--boundary-ratio", args.boundary_ratio), ("--bf-ratio", args.bf_ratio)) if v is not None]
    if args.boundary_scores and not args.label:
        ap.error("--boundary-scores compares the label maps with the ground truth: it needs --label")
    if given and not args.boundary_scores:
        ap.error(f"{', '.join(given)} only with --boundary-scores")
    tta = None
    if args.ms_scales is not None or args.flip:
        tta = TTA(tuple(args.ms_scales) if args.ms_scales is not None else (1.0,), args.flip, args.size_divisor)
        try:
            tta.plan(8, 8)  # (the settings' own checks: scales > 0, divisor >= 1, at most 16 views)
        except ValueError as e:
            ap.error(str(e))
    return args, tta


def boundary_settings(args):
    """the Evaluator's boundary= for a parsed command line: None without --boundary-scores, else the flags that were given"""
    if not args.boundary_scores:
        return None
    pairs = (("d", args.boundary_width), ("theta", args.bf_tolerance), ("ratio", args.boundary_ratio), ("bf_ratio", args.bf_ratio))
    return {k: v for k, v in pairs if v is not None}


def calibration_settings(args):
    """the Evaluator's calibration= for a parsed command line: None without --calibration, else the flags that were given"""
    if not args.calibration:
        return None
    pairs = (("bins", args.calibration_bins), ("temperatures", args.calibration_temperatures), ("thresholds", args.calibration_thresholds))
    kw = {k: (v if k == "bins" else tuple(v)) for k, v in pairs if v is not None}
    return kw


def object_settings(args):
    """the Evaluator's objects= for a parsed command line: None without --object-scores, else the flags that were given"""
    if not args.object_scores:
        return None
    pairs = (("connectivity", args.object_connectivity), ("size_edges", args.object_size_edges), ("coverage", args.object_coverage))
    return {k: (tuple(v) if k == "size_edges" else v) for k, v in pairs if v is not None}


def main(argv=None):
    args, tta = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("segmif_amd.evaluate needs the MI355X device (the HIP path has no CPU fallback)")
    from .core import Fusion_Network3_ac, Network3

    torch.manual_seed(0)
    seg, fus = Network3(args.backbone, 9, pretrained=None), Fusion_Network3_ac()
    for net, ckpt, what in ((seg, args.seg_ckpt, "segmentation"), (fus, args.fusion_ckpt, "fusion")):
        if ckpt:
            _load_weights(net, ckpt)
        else:
            print(f"[evaluate] no checkpoint for the {what} network: running on SEEDED RANDOM weights (torch.manual_seed(0))")
    seg, fus = seg.cuda().eval(), fus.cuda().eval()
    ev = Evaluator(seg, fus, structural=args.structural_scores, tta=tta, boundary=boundary_settings(args), calibration=calibration_settings(args),
                   objects=object_settings(args))
    names = _names(args.vis)
    if not names:
        raise RuntimeError(f"no .npy / .png files in {args.vis}")
    for sub in ("Fused", "Seg"):
        os.makedirs(os.path.join(args.out, sub), exist_ok=True)

    def batch_of(folder, chunk, dtype):
        return torch.from_numpy(np.stack([np.asarray(_read(os.path.join(folder, n))) for n in chunk]).astype(dtype)).cuda()

    for i in range(0, len(names), max(1, args.batch)):
        chunk = names[i:i + max(1, args.batch)]
        label = batch_of(args.label, chunk, np.int64) if args.label else None
        fused_u8, labels = ev.update(batch_of(args.ir, chunk, np.uint8), batch_of(args.vis, chunk, np.uint8),
                                     batch_of(args.mask, chunk, np.uint8), label)
        fused_h, seg_h = fused_u8.cpu().numpy(), colorize(labels, MFNET_PALETTE).cpu().numpy()
        for k, n in enumerate(chunk):
            _write(os.path.join(args.out, "Fused", n), fused_h[k])
            _write(os.path.join(args.out, "Seg", n), seg_h[k])
            print(f"[evaluate] {n}")
    res = ev.results()
    doc = ev.document(names, [w for w, c in (("seg", args.seg_ckpt), ("fusion", args.fusion_ckpt)) if not c], res)
    path = args.json or os.path.join(args.out, "results.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("[evaluate] " + "  ".join(f"{k} {res['mean'][k]:.4f}" for k in res["mean"]) + (f"  mIoU {res['mIoU']:.4f}" if "mIoU" in res else "")
          + (f"  mBIoU {res['mBIoU']:.4f}  trimap {res['trimap_mIoU']:.4f}  mBF {res['mBF']:.4f}" if "mBIoU" in res else "")
          + (f"  ECE {res['ece'][0]:.4f}  NLL {res['nll'][0]:.4f} (T {res['temperatures'][0]:g})  T* {res['best']['temperature']:.3f}"
             if res.get("best") is not None else "")
          + (f"  objR {res['mObjRecall']:.4f}  objP {res['mObjPrecision']:.4f}  objF1 {res['mObjF1']:.4f}" if "mObjF1" in res else ""))
    print(f"[evaluate] wrote {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
