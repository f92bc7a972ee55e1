"""Object-level scores of the label maps, gathered on the device (csrc/objects.hip; the rule: include/segmif_objects.h).  This
project's addition, NOT the reference's evaluation, which reports the plain mIoU only.

  object_stats           the connected components of the ground truth (side 0) and of the prediction (side 1) and, per side, class
                         and size bucket, their number by coverage decile and the sums of their areas and covered areas; out= adds
                         a data set in place
  connected_components   the labeller alone: the minimum linear index of every pixel's component, and the components per frame
  object_scores          one readback, float64 on the host: object recall, precision and F1 per class at a coverage, the same by
                         size bucket, the numbers of objects, and the three means

Coverage-based detection (the Pd / false-alarm convention of IR small-target work), not a one-to-one IoU matching as panoptic
quality does: a blob that swallows three pedestrians detects all three and counts as one correct prediction."""
import ctypes

import numpy as np
import torch

from .. import _lib

DEFAULT_SIZE_EDGES = (1024, 9216)  # COCO's: small below 32^2, medium, large from 96^2 upward
MAX_EDGES, DECILES = _lib.OBJECTS_MAX_EDGES, _lib.OBJECTS_DECILES
OBJECT_SCORE_NAMES = ("obj_recall", "obj_precision", "obj_f1", "obj_recall_by_size", "obj_precision_by_size", "n_gt_objects",
                      "n_pred_objects", "mObjRecall", "mObjPrecision", "mObjF1")


def _settings(n_class, connectivity, size_edges):
    """-> (K, connectivity, edges as a tuple of ints), checked against the kernel's domain (what it answers SEGMIF_EINVAL to)"""
    K = int(n_class)
    if not 1 <= K <= 32:
        raise ValueError(f"objects: n_class {n_class}, the kernel takes 1..32 (SEGMIF_EINVAL)")
    if connectivity not in (4, 8):
        raise ValueError(f"objects: connectivity {connectivity!r}, must be 4 or 8 (SEGMIF_EINVAL)")
    edges = tuple(size_edges)
    if any(int(e) != e for e in edges):
        raise ValueError(f"objects: size_edges are pixel counts (integers), got {list(edges)}")
    edges = tuple(int(e) for e in edges)
    if len(edges) > MAX_EDGES or any(e < 1 for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"objects: at most {MAX_EDGES} size_edges, each >= 1 and strictly ascending, got {list(edges)} (SEGMIF_EINVAL)")
    return K, int(connectivity), edges


def coverage_decile(coverage):
    """-> k in 1..10 with coverage = k / 10; a ValueError for anything else"""
    k = int(round(float(coverage) * 10))
    if not 1 <= k <= 10 or abs(float(coverage) * 10 - k) > 1e-9:
        raise ValueError(f"objects: coverage {coverage!r} must be one of 0.1, 0.2 ... 1.0 (the table holds deciles)")
    return k


class ObjectTable:
    """The tensors of segmif_object_stats_i32 and the settings they were gathered with.  obj (..., 2, K, S, 11) int64: components per
    side (0 ground truth, 1 prediction), class, size bucket and coverage decile; mass (..., 2, K, S, 2) int64: {sum of area, sum of
    hit}; status (2) int32: {a loop reached its iteration cap, reserved}.  The leading axis is the batch from object_stats without
    out=, absent in a table that sums a data set (ObjectTable.zeros, out=).  root_g, root_p (B, H, W) int32: only with return_roots,
    the last call's.  Device tensors from object_stats; object_scores also takes a table of arrays."""

    def __init__(self, obj, mass, status, n_class, connectivity, size_edges, root_g=None, root_p=None):
        self.obj, self.mass, self.status = obj, mass, status
        self.n_class, self.connectivity, self.size_edges = _settings(n_class, connectivity, size_edges)
        self.root_g, self.root_p = root_g, root_p
        K, S = self.n_class, len(self.size_edges) + 1
        shapes = (tuple(obj.shape)[-4:], tuple(mass.shape)[-4:], tuple(status.shape))
        if shapes != ((2, K, S, DECILES), (2, K, S, 2), (2,)) or len(obj.shape) not in (4, 5) or len(obj.shape) != len(mass.shape):
            raise ValueError(f"ObjectTable: tensors of shapes {tuple(obj.shape)}, {tuple(mass.shape)}, {tuple(status.shape)} for {K} "
                             f"classes and {S} size buckets")

    @classmethod
    def zeros(cls, device, n_class=9, connectivity=8, size_edges=DEFAULT_SIZE_EDGES, batch=None):
        K, conn, edges = _settings(n_class, connectivity, size_edges)
        lead = () if batch is None else (int(batch),)
        return cls(torch.zeros(lead + (2, K, len(edges) + 1, DECILES), device=device, dtype=torch.int64),
                   torch.zeros(lead + (2, K, len(edges) + 1, 2), device=device, dtype=torch.int64),
                   torch.zeros((2,), device=device, dtype=torch.int32), K, conn, edges)

    def same_settings(self, n_class, connectivity, size_edges):
        return (self.n_class, self.connectivity, self.size_edges) == _settings(n_class, connectivity, size_edges)

    def settings(self):
        return {"connectivity": self.connectivity, "size_edges": list(self.size_edges)}


def _descriptor(connectivity, edges):
    d = _lib.SegmifObjects()
    d.connectivity, d.n_edges = connectivity, len(edges)
    for i, e in enumerate(edges):
        d.edges[i] = e
    return d


def _check_map(t, name, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"segmif_amd: {name} must be a tensor on the MI355X device (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"segmif_amd: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != 3 or not t.is_contiguous():
        raise RuntimeError(f"segmif_amd: {name} must be a contiguous (B, H, W) tensor, got shape {tuple(t.shape)}, strides {t.stride()}")


def object_stats(pred, label, n_class=9, connectivity=8, size_edges=DEFAULT_SIZE_EDGES, out=None, return_roots=False,
                 max_workspace_bytes=256 << 20):
    """pred (B, H, W) int32, label (B, H, W) int64 device tensors, every label outside 0..n_class-1 ignored and the prediction
    blanked there.  -> an ObjectTable with obj (B, 2, K, S, 11) and mass (B, 2, K, S, 2), one table per frame.  out=: a table of
    the SAME settings (a ValueError otherwise) holding (2, K, S, 11) / (2, K, S, 2) sums that this batch is added to on the device
    and that is returned; nothing is read back.  return_roots: the table's root_g and root_p hold this call's (B, H, W) int32 roots.
    The batch is walked in chunks of frames so that the workspace (26 bytes per pixel) stays under max_workspace_bytes; frames are
    independent, so the tables are the same bits whatever the chunking."""
    _check_map(pred, "pred", torch.int32)
    _check_map(label, "label", torch.int64)
    if pred.shape != label.shape:
        raise RuntimeError(f"pred is {tuple(pred.shape)}, label {tuple(label.shape)}")
    K, conn, edges = _settings(n_class, connectivity, size_edges)
    B, H, W = (int(v) for v in pred.shape)
    dev = pred.device
    if out is not None:
        if not isinstance(out, ObjectTable) or not out.same_settings(K, conn, edges) or out.obj.dim() != 4:
            raise ValueError("object_stats: out= must be an ObjectTable of sums gathered with the same n_class, connectivity and size_edges")
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() for t in (out.obj, out.mass, out.status)):
            raise RuntimeError("object_stats: out= must hold contiguous device tensors")
    lib = _lib.load()
    per_frame = int(lib.segmif_object_workspace_bytes(1, H, W)) if min(B, H, W) >= 1 else 0
    if per_frame <= 0:
        raise ValueError(f"object_stats: B, H and W must be >= 1 and H * W below 2^31, got {tuple(pred.shape)} (SEGMIF_EINVAL)")
    chunk = max(1, min(B, int(max_workspace_bytes) // per_frame, _lib.OBJECTS_MAX_FRAMES))
    table = ObjectTable.zeros(dev, K, conn, edges, batch=B)
    if out is not None:
        table.status = out.status
    root_g = torch.empty((B, H, W), device=dev, dtype=torch.int32) if return_roots else None
    root_p = torch.empty((B, H, W), device=dev, dtype=torch.int32) if return_roots else None
    workspace = torch.empty((int(lib.segmif_object_workspace_bytes(chunk, H, W)) // 8,), device=dev, dtype=torch.int64)
    desc = _descriptor(conn, edges)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        _lib.check(lib.segmif_object_stats_i32(
            ctypes.byref(desc), pred[b0:].data_ptr(), label[b0:].data_ptr(), table.obj[b0:].data_ptr(), table.mass[b0:].data_ptr(),
            table.status.data_ptr(), workspace.data_ptr(), root_g[b0:].data_ptr() if return_roots else None,
            root_p[b0:].data_ptr() if return_roots else None, n, H, W, K, stream), "segmif_object_stats_i32")
    if out is not None:
        out.obj += table.obj.sum(dim=0)
        out.mass += table.mass.sum(dim=0)
        table = out
    table.root_g, table.root_p = root_g, root_p
    return table


def connected_components(m, n_class, connectivity=8):
    """The labeller alone, for a (B, H, W) int32 or int64 device map: values outside 0..n_class-1 belong to no component.
    -> (root (B, H, W) int32: the smallest linear index y * W + x of the pixel's component, -1 outside every component;
    count (B,) int64: the components per frame)."""
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise RuntimeError("segmif_amd: the map must be a tensor on the MI355X device (the HIP path has no CPU fallback)")
    if m.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f"segmif_amd: the map must be torch.int32 or torch.int64, got {m.dtype}")
    label = m.to(torch.int64).contiguous()
    pred = torch.zeros(label.shape, device=m.device, dtype=torch.int32)  # (the prediction's side is not read back)
    t = object_stats(pred, label, n_class, connectivity, (), return_roots=True)
    return t.root_g, t.obj[:, 0].sum(dim=(1, 2, 3))


def _host_tables(table):
    """-> (obj, mass, status) as numpy arrays; ONE readback when the table lives on the device"""
    parts = (table.obj, table.mass, table.status)
    if all(isinstance(t, torch.Tensor) and t.is_cuda for t in parts):
        flat = torch.cat([parts[0].reshape(-1), parts[1].reshape(-1), parts[2].reshape(-1).to(torch.int64)]).cpu().numpy()
        n0, n1 = parts[0].numel(), parts[1].numel()
        return flat[:n0].reshape(parts[0].shape), flat[n0:n0 + n1].reshape(parts[1].shape), flat[n0 + n1:]
    host = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in parts]
    return host[0].astype(np.int64), host[1].astype(np.int64), host[2].astype(np.int64)


def _ratio(num, den):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0, np.nan, num / den.astype(np.float64))


def object_scores(table, coverage=0.5):
    """The scores of an ObjectTable (per-frame tables are summed first), float64 on the host after one readback.  An object counts
    as found when at least `coverage` (one of 0.1, 0.2 ... 1.0) of its pixels carry its class in the other map.  obj_recall (K):
    the found share of the ground truth's components; obj_precision (K): the same for the prediction's components; obj_f1 =
    2 P R / (P + R), NaN when either denominator is empty, 0 when P + R = 0; obj_recall_by_size, obj_precision_by_size (K, S) per
    size bucket; n_gt_objects, n_pred_objects (K, S); mObjRecall, mObjPrecision, mObjF1 = mean(nan_to_num(.)).  RuntimeError when
    the kernel reported that a loop reached its iteration cap, ValueError for a coverage the deciles cannot express."""
    k = coverage_decile(coverage)
    obj, _, status = _host_tables(table)
    if int(status[0]) != 0:
        raise RuntimeError("object_scores: the kernel reported that a find / union loop reached its iteration cap (status[0] != 0): "
                           "the tables are not to be trusted")
    if obj.ndim == 5:
        obj = obj.sum(axis=0)
    n = obj.sum(axis=3)                    # (2, K, S)
    found = obj[:, :, :, k:].sum(axis=3)   # (2, K, S)
    recall, precision = _ratio(found[0].sum(axis=1), n[0].sum(axis=1)), _ratio(found[1].sum(axis=1), n[1].sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        f1 = np.where(precision + recall == 0, 0.0, 2 * precision * recall / (precision + recall))
    f1 = np.where(np.isnan(precision) | np.isnan(recall), np.nan, f1)
    return {"obj_recall": recall, "obj_precision": precision, "obj_f1": f1,
            "obj_recall_by_size": _ratio(found[0], n[0]), "obj_precision_by_size": _ratio(found[1], n[1]),
            "n_gt_objects": n[0].copy(), "n_pred_objects": n[1].copy(),
            "mObjRecall": float(np.mean(np.nan_to_num(recall))), "mObjPrecision": float(np.mean(np.nan_to_num(precision))),
            "mObjF1": float(np.mean(np.nan_to_num(f1)))}
