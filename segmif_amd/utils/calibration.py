"""Confidence calibration of the segmentation net's softmax, gathered on the device (csrc/calibration_stats.hip; the rule:
include/segmif_calib.h).  This project's addition, NOT the reference's evaluation, which scores labels only.

  uniform_edges        the M - 1 interior edges of M equal confidence bins, float32
  calibration_stats    the tables of one batch of quarter-resolution NHWC logits against full-resolution labels, for a list of
                       temperatures: per (temperature, bin) {n, correct, sum of conf}, per (temperature, threshold) {n, correct}
                       above it, {valid, ignored, nonfinite} and the sums of NLL and Brier score; out= adds a data set in place
  calibration_scores   one readback, float64 on the host: accuracy, mean confidence, ECE and MCE (Guo et al. 2017), NLL, Brier score,
                       the reliability rows, coverage and precision above each threshold, and the best temperature of the list
  fit_temperature      a GRID search, not an optimiser: narrows a 16-point log grid around the NLL minimum, one readback per pass

The full-resolution softmax is never written.  Nothing here says what a trained model's calibration is: that takes a data set."""
import ctypes
import math

import numpy as np
import torch

from .. import _lib

MAX_TEMPERATURES, MAX_BINS, MAX_THRESHOLDS = _lib.CALIB_MAX_TEMPERATURES, _lib.CALIB_MAX_EDGES + 1, _lib.CALIB_MAX_THRESHOLDS
# 1.0 first (the uncalibrated net), then 15 log-spaced values over [0.5, 4]
DEFAULT_TEMPERATURES = (1.0,) + tuple(float(v) for v in np.exp(np.linspace(math.log(0.5), math.log(4.0), 15)))
CONF_SCALE = 4294967296.0  # counts[..., 2] holds the sum of conf * 2^32, an exact integer


def uniform_edges(M=15):
    """-> the M - 1 interior edges k / M, k = 1..M-1, of M equal bins over [0, 1], each formed as np.float32(k) / np.float32(M)."""
    M = int(M)
    if not 1 <= M <= MAX_BINS:
        raise ValueError(f"uniform_edges: {M} bins, the kernel takes 1..{MAX_BINS}")
    return np.array([np.float32(k) / np.float32(M) for k in range(1, M)], dtype=np.float32)


def _settings(temperatures, edges, thresholds):
    """the three lists as float32 arrays, checked against the kernel's domain (what it answers SEGMIF_EINVAL to)"""
    T = np.asarray(list(temperatures), dtype=np.float32).reshape(-1)
    E = uniform_edges(15) if edges is None else np.asarray(list(edges), dtype=np.float32).reshape(-1)
    K = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    if not 1 <= T.size <= MAX_TEMPERATURES or not np.all(np.isfinite(T)) or not np.all(T > 0):
        raise ValueError(f"calibration: 1..{MAX_TEMPERATURES} temperatures, finite and > 0, got {T.tolist()} (SEGMIF_EINVAL)")
    if E.size > MAX_BINS - 1 or not np.all((E > 0) & (E < 1)) or not np.all(np.diff(E) > 0):
        raise ValueError(f"calibration: at most {MAX_BINS - 1} interior edges, strictly ascending inside (0, 1), got {E.tolist()} (SEGMIF_EINVAL)")
    if K.size > MAX_THRESHOLDS or not np.all((K >= 0) & (K <= 1)):
        raise ValueError(f"calibration: at most {MAX_THRESHOLDS} thresholds in [0, 1], got {K.tolist()} (SEGMIF_EINVAL)")
    return T, E, K


class CalibrationTable:
    """The four tensors of segmif_calibration_stats_f32 and the settings they were gathered with.  counts (NT, M, 3) int64
    {n, correct, conf_q}, above (NT, NK, 2) int64 {n, correct}, totals (3) int64 {valid, ignored, nonfinite}, sums (NT, 2) float64
    {nll, brier}; temperatures, edges (interior), thresholds: float32 arrays.  conf (NT, B, OH, OW) float32 and pred (B, OH, OW)
    int32 are the last call's own values, only with return_conf.  Device tensors from calibration_stats; calibration_scores also
    takes a table of arrays."""

    def __init__(self, counts, above, totals, sums, temperatures, edges, thresholds, conf=None, pred=None):
        self.counts, self.above, self.totals, self.sums = counts, above, totals, sums
        self.temperatures, self.edges, self.thresholds = _settings(temperatures, edges, thresholds)
        self.conf, self.pred = conf, pred
        NT, M, NK = self.temperatures.size, self.edges.size + 1, self.thresholds.size
        shapes = (tuple(counts.shape), tuple(above.shape), tuple(totals.shape), tuple(sums.shape))
        if shapes != ((NT, M, 3), (NT, NK, 2), (3,), (NT, 2)):
            raise ValueError(f"CalibrationTable: tensors of shapes {shapes} for {NT} temperatures, {M} bins and {NK} thresholds")

    @classmethod
    def zeros(cls, device, temperatures=(1.0,), edges=None, thresholds=(0.968,)):
        T, E, K = _settings(temperatures, edges, thresholds)
        return cls(torch.zeros((T.size, E.size + 1, 3), device=device, dtype=torch.int64),
                   torch.zeros((T.size, K.size, 2), device=device, dtype=torch.int64), torch.zeros((3,), device=device, dtype=torch.int64),
                   torch.zeros((T.size, 2), device=device, dtype=torch.float64), T, E, K)

    def same_settings(self, temperatures, edges, thresholds):
        T, E, K = _settings(temperatures, edges, thresholds)
        return all(a.shape == b.shape and np.array_equal(a, b) for a, b in ((T, self.temperatures), (E, self.edges), (K, self.thresholds)))

    def settings(self):
        """-> the settings as plain lists (what Evaluator.document writes under "calibration")"""
        return {"bins": int(self.edges.size + 1), "edges": [float(v) for v in self.edges],
                "temperatures": [float(v) for v in self.temperatures], "thresholds": [float(v) for v in self.thresholds]}


def table_settings(bins=15, temperatures=DEFAULT_TEMPERATURES, thresholds=(0.968,)):
    """The keywords of CalibrationTable.zeros / calibration_stats for the settings Evaluator(calibration=) and the evaluate command
    take, with their defaults: 15 equal bins, DEFAULT_TEMPERATURES, threshold 0.968."""
    return dict(temperatures=tuple(temperatures), edges=uniform_edges(bins), thresholds=tuple(thresholds))


def _descriptor(T, E, K):
    d = _lib.SegmifCalib()
    d.n_temperatures, d.n_edges, d.n_thresholds = T.size, E.size, K.size
    for i, v in enumerate(T):
        d.temperatures[i] = float(v)
    for i, v in enumerate(E):
        d.edges[i] = float(v)
    for i, v in enumerate(K):
        d.thresholds[i] = float(v)
    return d


def calibration_stats(logits_nhwc, label, temperatures=(1.0,), edges=None, thresholds=(0.968,), out=None, return_conf=False):
    """logits_nhwc (B, IH, IW, C) float32 rows view on the device, C <= 32 (Network3._segment_nhwc's output, a pitched view of it);
    label (B, OH, OW) int64, every value outside 0..C-1 ignored.  edges: None = uniform_edges(15).  -> a CalibrationTable.  out=: a
    table of the SAME settings (a ValueError otherwise) that this batch is added to on the device and that is returned; nothing is
    read back.  return_conf: the table's conf and pred hold the kernel's own per-pixel values of this call (NaN / -1 where the pixel
    is ignored or not finite) - for tests, it writes 4 (NT + 1) bytes per pixel."""
    from .. import ops
    if not isinstance(logits_nhwc, torch.Tensor) or logits_nhwc.dim() != 4:
        raise RuntimeError("calibration_stats expects (B, H, W, C) logits")
    _, C, ldx = ops.rows_view(logits_nhwc, "logits")
    if not isinstance(label, torch.Tensor) or not label.is_cuda or label.dtype != torch.int64 or label.dim() != 3 or not label.is_contiguous():
        raise RuntimeError("segmif_amd: label must be a contiguous (B, OH, OW) int64 tensor on the MI355X device")
    B, IH, IW = (int(v) for v in logits_nhwc.shape[:3])
    if label.shape[0] != B:
        raise RuntimeError(f"logits of {B} samples, labels of {label.shape[0]}")
    OH, OW = int(label.shape[1]), int(label.shape[2])
    if out is None:
        out = CalibrationTable.zeros(logits_nhwc.device, temperatures, edges, thresholds)
    elif not isinstance(out, CalibrationTable) or not out.same_settings(temperatures, edges, thresholds):
        raise ValueError("calibration_stats: out= must be a CalibrationTable gathered with the same temperatures, edges and thresholds")
    elif not all(isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() for t in (out.counts, out.above, out.totals, out.sums)):
        raise RuntimeError("calibration_stats: out= must hold contiguous device tensors")
    T, E, K = out.temperatures, out.edges, out.thresholds
    lib = _lib.load()
    nbytes = int(lib.segmif_calibration_workspace_bytes(B, OH, OW, T.size))
    if nbytes <= 0 or min(B, IH, IW, OH, OW) < 1 or not 1 <= C <= 32:
        raise ValueError(f"calibration_stats: sizes must be >= 1, C in 1..32, B and OH at most 65535; got {tuple(logits_nhwc.shape)} -> "
                         f"{OH} x {OW} (SEGMIF_EINVAL)")
    dev = logits_nhwc.device
    workspace = torch.empty((nbytes // 8,), device=dev, dtype=torch.float64)
    conf = torch.empty((T.size, B, OH, OW), device=dev, dtype=torch.float32) if return_conf else None
    pred = torch.empty((B, OH, OW), device=dev, dtype=torch.int32) if return_conf else None
    desc = _descriptor(T, E, K)
    _lib.check(lib.segmif_calibration_stats_f32(
        ctypes.byref(desc), logits_nhwc.data_ptr(), label.data_ptr(), out.counts.data_ptr(), out.above.data_ptr() if K.size else None,
        out.totals.data_ptr(), out.sums.data_ptr(), workspace.data_ptr(), conf.data_ptr() if return_conf else None,
        pred.data_ptr() if return_conf else None, B, IH, IW, OH, OW, C, ldx,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "segmif_calibration_stats_f32")
    out.conf, out.pred = conf, pred
    return out


def _host_tables(table):
    """-> (counts, above, totals, sums) as numpy arrays; ONE readback when the table lives on the device"""
    parts = (table.counts, table.above, table.totals, table.sums)
    if all(isinstance(t, torch.Tensor) and t.is_cuda for t in parts):
        flat = torch.cat([parts[0].reshape(-1), parts[1].reshape(-1), parts[2].reshape(-1), parts[3].reshape(-1).view(torch.int64)]).cpu().numpy()
        n0, n1 = parts[0].numel(), parts[1].numel()
        return (flat[:n0].reshape(parts[0].shape), flat[n0:n0 + n1].reshape(parts[1].shape), flat[n0 + n1:n0 + n1 + 3],
                flat[n0 + n1 + 3:].view(np.float64).reshape(parts[3].shape))
    host = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in parts]
    return host[0].astype(np.int64), host[1].astype(np.int64), host[2].astype(np.int64), host[3].astype(np.float64)


def calibration_scores(table):
    """The scores of a CalibrationTable, float64 on the host after one readback.  N = valid pixels.  Per temperature (arrays of
    NT): accuracy = correct / N, confidence = the mean confidence, ece = sum_m (n_m / N) |acc_m - conf_m| and mce = max_m |acc_m -
    conf_m| over the bins that hold a pixel (Guo et al. 2017), nll and brier = their sums / N; NaN throughout when N = 0.
    reliability_n / reliability_accuracy / reliability_confidence (NT, M): the reliability diagram's rows, NaN for an empty bin;
    bin_edges: the M + 1 edges with 0 and 1.  above_coverage = n / N and above_precision = correct / n (NT, NK) per threshold of
    `thresholds`, NaN for an empty denominator.  best: the temperature OF THE LIST with the lowest NLL and its own measured scores
    (None when N = 0); calibration_pixels: {valid, ignored, nonfinite}."""
    counts, above, totals, sums = _host_tables(table)
    T = np.asarray(table.temperatures, dtype=np.float64)
    n, correct = counts[:, :, 0].astype(np.float64), counts[:, :, 1].astype(np.float64)
    conf_sum = counts[:, :, 2].astype(np.float64) / CONF_SCALE
    N = float(totals[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        acc_m = np.where(n == 0, np.nan, correct / n)
        conf_m = np.where(n == 0, np.nan, conf_sum / n)
        gap = np.abs(acc_m - conf_m)
        if N > 0:
            accuracy, confidence = correct.sum(axis=1) / N, conf_sum.sum(axis=1) / N
            ece = np.where(n == 0, 0.0, (n / N) * gap).sum(axis=1)
            mce = np.nanmax(np.where(n == 0, -np.inf, gap), axis=1)
            nll, brier = sums[:, 0] / N, sums[:, 1] / N
            coverage = above[:, :, 0] / N
        else:
            accuracy = confidence = ece = mce = nll = brier = np.full(T.shape, np.nan)
            coverage = np.full(above.shape[:2], np.nan)
        precision = np.where(above[:, :, 0] == 0, np.nan, above[:, :, 1] / above[:, :, 0].astype(np.float64))
    best = None
    if N > 0 and not np.all(np.isnan(nll)):
        i = int(np.nanargmin(nll))
        best = {"index": i, "temperature": float(T[i]), "nll": float(nll[i]), "ece": float(ece[i]), "mce": float(mce[i]),
                "brier": float(brier[i]), "accuracy": float(accuracy[i]), "confidence": float(confidence[i])}
    return {"temperatures": T, "accuracy": accuracy, "confidence": confidence, "ece": ece, "mce": mce, "nll": nll, "brier": brier,
            "bin_edges": np.concatenate([[0.0], np.asarray(table.edges, dtype=np.float64), [1.0]]),
            "reliability_n": counts[:, :, 0].copy(), "reliability_accuracy": acc_m, "reliability_confidence": conf_m,
            "thresholds": np.asarray(table.thresholds, dtype=np.float64), "above_coverage": coverage, "above_precision": precision,
            "best": best, "calibration_pixels": {"valid": int(totals[0]), "ignored": int(totals[1]), "nonfinite": int(totals[2])}}


CALIBRATION_SCORE_NAMES = ("temperatures", "accuracy", "confidence", "ece", "mce", "nll", "brier", "bin_edges", "reliability_n",
                           "reliability_accuracy", "reliability_confidence", "thresholds", "above_coverage", "above_precision", "best",
                           "calibration_pixels")


def fit_temperature(logits_nhwc, label, lo=0.25, hi=8.0, passes=3):
    """A grid search for the temperature of lowest NLL on tensors that are still resident - NOT an optimiser.  Every pass gathers a
    16-point log grid over [lo, hi] in one calibration_stats call (no bins, no thresholds), reads it back once, and narrows [lo, hi]
    to the grid's neighbours of the minimum.  -> {"temperature", "nll", "passes": [{"grid", "nll"} per pass]}: the grid point of
    lowest NLL over all passes; after p passes neighbouring grid points differ by a factor
    (hi / lo) ** ((2 / 15) ** (p - 1) / 15).  ValueError without a valid pixel."""
    lo, hi, passes = float(lo), float(hi), int(passes)
    if not (0 < lo < hi and math.isfinite(hi)) or passes < 1:
        raise ValueError(f"fit_temperature: needs 0 < lo < hi and passes >= 1, got {lo}, {hi}, {passes}")
    history, best = [], None
    for _ in range(passes):
        grid = np.exp(np.linspace(math.log(lo), math.log(hi), MAX_TEMPERATURES))
        table = calibration_stats(logits_nhwc, label, temperatures=grid, edges=(), thresholds=())
        s = calibration_scores(table)
        if s["best"] is None:
            raise ValueError("fit_temperature: no valid pixel (every label ignored, or every labelled pixel not finite)")
        i = s["best"]["index"]
        history.append({"grid": [float(v) for v in table.temperatures], "nll": [float(v) for v in s["nll"]]})
        if best is None or float(s["nll"][i]) < best[1]:  # (a later grid does not contain the earlier minimum itself)
            best = (float(table.temperatures[i]), float(s["nll"][i]))
        lo, hi = float(grid[max(i - 1, 0)]), float(grid[min(i + 1, grid.size - 1)])
    return {"temperature": best[0], "nll": best[1], "passes": history}
