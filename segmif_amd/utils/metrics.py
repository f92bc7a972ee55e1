"""Evaluation metrics and image write-out on the device.

  confusion_matrix   test_segmentation.py:176-177 (sklearn confusion_matrix(labels=[0..K-1]), accumulated)
  compute_results    util/util.py:31-55 (per-class precision / recall / IoU, NaN for empty classes)
  quantize_fused     test_fusion.py:112-120 (uint8(255 x) -> global min-max rescale -> uint8, NHWC)
"""
import ctypes

import numpy as np
import torch

from .. import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"segmif_amd: {name} must be a tensor on the MI355X device (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"segmif_amd: {name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def confusion_matrix(pred, label, n_class=9, out=None):
    """pred: int32 labels (segmif_amd.ops.argmax_nhwc / Network3.predict_labels), label: int64 ground
    truth, same number of elements.  Returns / accumulates into an (n_class, n_class) int64 device tensor:
    rows = ground truth, columns = prediction."""
    pred, label = _dev(pred, "pred", torch.int32), _dev(label, "label", torch.int64)
    if pred.numel() != label.numel():
        raise RuntimeError(f"pred has {pred.numel()} elements, label {label.numel()}")
    if out is None:
        out = torch.zeros((n_class, n_class), device=pred.device, dtype=torch.int64)
    elif tuple(out.shape) != (n_class, n_class) or out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous (n_class, n_class) int64 device tensor")
    _lib.check(_lib.load().segmif_confusion_i32(pred.data_ptr(), label.data_ptr(), out.data_ptr(), pred.numel(), n_class,
                                                _stream()), "segmif_confusion_i32")
    return out


def compute_results(conf_total):
    """-> (precision, recall, iou) per class as float64 arrays; a class with an empty denominator gets NaN.
    Host-side arithmetic on the K x K matrix (accepts a device tensor or an array)."""
    conf = conf_total.detach().cpu().numpy() if isinstance(conf_total, torch.Tensor) else np.asarray(conf_total)
    conf = conf.astype(np.float64)
    tp = np.diag(conf)
    predicted = conf.sum(axis=0)  # column sums: everything predicted as the class
    actual = conf.sum(axis=1)  # row sums: everything that is the class
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.where(predicted == 0, np.nan, tp / predicted)
        recall = np.where(actual == 0, np.nan, tp / actual)
        union = actual + predicted - tp
        iou = np.where(union == 0, np.nan, tp / union)
    return precision, recall, iou


BOUNDARY_TILE = 64  # SEGMIF_BOUNDARY_TILE of include/segmif_hip.h: the side of the kernel's output tiles
BOUNDARY_COLUMNS = ("g_band", "p_band", "band_inter", "g_contour", "p_contour", "g_matched", "p_matched", "reserved")
BOUNDARY_SCORE_NAMES = ("boundary_iou", "mBIoU", "trimap_iou", "trimap_mIoU", "bf_precision", "bf_recall", "bf", "mBF")


def boundary_widths(H, W, ratio=0.02, bf_ratio=0.0075):
    """-> (d, theta) for an H x W frame: the band half-width d = ratio x the frame's diagonal (0.02: Boundary IoU's default,
    Cheng et al. 2021) and the contour tolerance theta = bf_ratio x the diagonal (0.75 %: Csurka et al. 2013), rounded half up;
    d >= 1, theta >= 0.  16 and 6 at 480 x 640, 14 and 5 at 512 x 512."""
    diag = float(np.sqrt(float(H) * H + float(W) * W))
    return max(1, int(ratio * diag + 0.5)), max(0, int(bf_ratio * diag + 0.5))


def boundary_stats(pred, label, n_class=9, d=None, theta=None, out=None):
    """The contour tables of segmif_boundary_stats_i32 (include/segmif_hip.h has the rule).  pred (B, H, W) int32, label
    (B, H, W) int64 device tensors; d, theta: None = boundary_widths(H, W).  -> (cls (B, n_class, 8), trimap (B, n_class,
    n_class)) int64 device tensors, one table pair per frame (columns of cls: BOUNDARY_COLUMNS).  out=(cls_total (n_class, 8),
    trimap_total (n_class, n_class)): the sums over the batch are added to them on the device; nothing is read back."""
    for t, name, dtype in ((pred, "pred", torch.int32), (label, "label", torch.int64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"segmif_amd: {name} must be a tensor on the MI355X device (the HIP path has no CPU fallback)")
        if t.dtype != dtype:
            raise RuntimeError(f"segmif_amd: {name} must be {dtype}, got {t.dtype}")
        if t.dim() != 3 or not t.is_contiguous():
            raise RuntimeError(f"segmif_amd: {name} must be a contiguous (B, H, W) tensor, got shape {tuple(t.shape)}, strides {t.stride()}")
    if pred.shape != label.shape:
        raise RuntimeError(f"pred is {tuple(pred.shape)}, label {tuple(label.shape)}")
    B, H, W = pred.shape
    wd, wt = boundary_widths(H, W)
    d, theta = wd if d is None else int(d), wt if theta is None else int(theta)
    if not 1 <= d <= 32:
        raise ValueError(f"boundary_stats: a {H} x {W} frame gives the band half-width d = {d}, the kernel takes 1..32; pass d= to override it")
    if not 0 <= theta <= 31:
        raise ValueError(f"boundary_stats: a {H} x {W} frame gives the contour tolerance theta = {theta}, the kernel takes 0..31; "
                         "pass theta= to override it")
    if out is not None:
        ok = (isinstance(out, (tuple, list)) and len(out) == 2
              and all(isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.int64 and o.is_contiguous() for o in out)
              and tuple(out[0].shape) == (n_class, 8) and tuple(out[1].shape) == (n_class, n_class))
        if not ok:
            raise RuntimeError("out must be (cls_total (n_class, 8), trimap_total (n_class, n_class)), contiguous int64 device tensors")
    cls = torch.empty((B, n_class, 8), device=pred.device, dtype=torch.int64)
    trimap = torch.empty((B, n_class, n_class), device=pred.device, dtype=torch.int64)
    _lib.check(_lib.load().segmif_boundary_stats_i32(pred.data_ptr(), label.data_ptr(), B, H, W, n_class, d, theta, cls.data_ptr(),
                                                     trimap.data_ptr(), _stream()), "segmif_boundary_stats_i32")
    if out is not None:
        out[0].add_(cls.sum(dim=0))
        out[1].add_(trimap.sum(dim=0))
    return cls, trimap


def boundary_scores(cls_total, trimap_total):
    """The data set's contour scores from the summed tables (device tensors or arrays), as float64 on the host; sums first,
    ratios after, as the mIoU.  Per class, NaN for an empty denominator: boundary_iou = band_inter / (g_band + p_band -
    band_inter) (Boundary IoU), trimap_iou = compute_results(trimap_total)'s IoU (the confusion matrix of the ground truth's
    band), bf_precision = p_matched / p_contour, bf_recall = g_matched / g_contour and bf = 2 P R / (P + R), NaN when either
    contour is empty and 0 when P + R = 0.  mBIoU, trimap_mIoU and mBF = mean(nan_to_num(.)), the convention of mIoU here."""
    def host(t):
        return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)

    cls, tri = host(cls_total), host(trimap_total)
    g_band, p_band, inter, g_cont, p_cont, g_match, p_match = (cls[:, i] for i in range(7))
    with np.errstate(invalid="ignore", divide="ignore"):
        union = g_band + p_band - inter
        biou = np.where(union == 0, np.nan, inter / union)
        precision = np.where(p_cont == 0, np.nan, p_match / p_cont)
        recall = np.where(g_cont == 0, np.nan, g_match / g_cont)
        s = precision + recall
        bf = np.where(np.isnan(s), np.nan, np.where(s == 0, 0.0, 2.0 * precision * recall / s))
    tiou = compute_results(tri)[2]
    mean = lambda x: float(np.mean(np.nan_to_num(x)))
    return {"boundary_iou": biou, "mBIoU": mean(biou), "trimap_iou": tiou, "trimap_mIoU": mean(tiou), "bf_precision": precision,
            "bf_recall": recall, "bf": bf, "mBF": mean(bf)}


def quantize_fused(fused):
    """fused: (B, C, H, W) fp32 in [0, 1] (core.fuse_to_rgb output) -> (B, H, W, C) uint8 exactly as the
    reference's script writes it to disk (global min / max over the batch)."""
    fused = _dev(fused, "fused", torch.float32)
    if fused.dim() != 4:
        raise RuntimeError("quantize_fused expects (B, C, H, W)")
    B, C, H, W = fused.shape
    out = torch.empty((B, H, W, C), device=fused.device, dtype=torch.uint8)
    mm = torch.empty((2,), device=fused.device, dtype=torch.int32)
    _lib.check(_lib.load().segmif_quantize_u8(fused.data_ptr(), out.data_ptr(), mm.data_ptr(), B, C, H * W, _stream()),
               "segmif_quantize_u8")
    return out


def dequantize_fused(q):
    """(B, H, W, C) uint8 (quantize_fused output = the PNG pixels) -> (B, C, H, W) fp32 = u / 255, the image
    test_segmentation.py's loader hands to the network (TaskFusion_dataset2.py:84-88)."""
    q = _dev(q, "q", torch.uint8)
    if q.dim() != 4 or not q.is_contiguous():
        raise RuntimeError("dequantize_fused expects a contiguous (B, H, W, C) uint8 tensor")
    B, H, W, C = q.shape
    out = torch.empty((B, C, H, W), device=q.device, dtype=torch.float32)
    _lib.check(_lib.load().segmif_dequantize_u8(q.data_ptr(), out.data_ptr(), B, C, H * W, _stream()), "segmif_dequantize_u8")
    return out
