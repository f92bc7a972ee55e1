"""Fusion-quality scores of a fused image against its infrared and visible sources, from statistics gathered on the device,
and the palette rendering of a label map (util/util.py:8-29).

  fusion_stats    one pass over three uint8 images per pair (csrc/fusion_stats.hip): two 256 x 256 joint histograms, the
                  squared-difference sums and the gradient sum, per image; all integers but the last
  fusion_scores   EN / MI / SD / SF / AG / CC / PSNR / SCD per image: float64 host arithmetic on those integers
  colorize        labels -> RGB through a palette (MFNET_PALETTE: the nine MFNet colours)
"""
import collections
import math

import numpy as np
import torch

from .. import _lib
from .metrics import _dev, _stream

FusionStats = collections.namedtuple("FusionStats", ["joint_fa", "joint_fv", "sums", "ag", "shape"], defaults=(None,))
FusionStats.__doc__ = """Device tensors, per image b: joint_fa[b][f][a], joint_fv[b][f][v] (B, 256, 256) int64 counts;
sums (B, 4) int64 = [sum a v, sum (f[y][x] - f[y][x-1])^2, sum (f[y][x] - f[y-1][x])^2, H W]; ag (B,) float64 =
sum over y < H-1, x < W-1 of sqrt((dx^2 + dy^2) / 2); shape = (H, W), host side.  f = L(fused), v = L(vis), a = ir,
L(R, G, B) = (299 R + 587 G + 114 B + 500) // 1000."""

SCORE_NAMES = ("EN", "MI", "SD", "SF", "AG", "CC", "PSNR", "SCD")

# 0 unlabeled, 1 car, 2 person, 3 bike, 4 curve, 5 car_stop, 6 guardrail, 7 color_cone, 8 bump (tests/golden/palette_mfnet.json)
MFNET_PALETTE = np.array([[0, 0, 0], [64, 0, 128], [64, 64, 0], [0, 128, 192], [0, 0, 192], [128, 128, 0], [64, 64, 128],
                          [192, 128, 128], [192, 64, 0]], dtype=np.uint8)


def _buffer(out, name, shape, dtype, device):
    t = None if out is None else getattr(out, name)
    if t is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise RuntimeError(f"out.{name} must be a contiguous {tuple(shape)} {dtype} device tensor")
    return t


def fusion_stats(fused_u8, vis_u8, ir_u8, out=None):
    """fused_u8, vis_u8: (B, H, W, 3) uint8 (what quantize_fused writes), ir_u8: (B, H, W) uint8, all on the device ->
    FusionStats.  A pair's statistics do not depend on what else is in the batch.  out=: a FusionStats whose buffers are
    reused (they are overwritten, not added to).  No host round trip, capturable in a graph."""
    fused_u8, vis_u8, ir_u8 = _dev(fused_u8, "fused_u8", torch.uint8), _dev(vis_u8, "vis_u8", torch.uint8), _dev(ir_u8, "ir_u8", torch.uint8)
    if fused_u8.dim() != 4 or fused_u8.shape[3] != 3 or vis_u8.shape != fused_u8.shape or tuple(ir_u8.shape) != tuple(fused_u8.shape[:3]):
        raise RuntimeError(f"fusion_stats expects (B, H, W, 3), (B, H, W, 3) and (B, H, W), got {tuple(fused_u8.shape)}, "
                           f"{tuple(vis_u8.shape)}, {tuple(ir_u8.shape)}")
    B, H, W, _ = fused_u8.shape
    dev = fused_u8.device
    lib = _lib.load()
    nbytes = lib.segmif_fusion_stats_workspace_bytes(B, H, W)
    if nbytes <= 0:
        raise RuntimeError(f"fusion_stats: unsupported size B = {B}, H = {H}, W = {W} (H, W >= 2)")
    st = FusionStats(_buffer(out, "joint_fa", (B, 256, 256), torch.int64, dev), _buffer(out, "joint_fv", (B, 256, 256), torch.int64, dev),
                     _buffer(out, "sums", (B, 4), torch.int64, dev), _buffer(out, "ag", (B,), torch.float64, dev), (H, W))
    ws = torch.empty((nbytes // 8,), device=dev, dtype=torch.int64)
    _lib.check(lib.segmif_fusion_stats_u8(fused_u8.data_ptr(), vis_u8.data_ptr(), ir_u8.data_ptr(), st.joint_fa.data_ptr(),
                                          st.joint_fv.data_ptr(), st.sums.data_ptr(), st.ag.data_ptr(), ws.data_ptr(), B, H, W, 0,
                                          _stream()), "segmif_fusion_stats_u8")
    return st


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _plogp(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, p * np.log2(p), 0.0)


def _mutual_information(joint, n):
    p = joint / n
    px, py = p.sum(axis=1), p.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(p > 0, p * np.log2(p / (px[:, None] * py[None, :])), 0.0).sum())


def _pearson(cov, var_x, var_y):
    """cov / sqrt(var_x var_y) on exact integers (central moments times n^2); NaN when a variance is zero"""
    if var_x <= 0 or var_y <= 0:
        return float("nan")
    return float(cov) / (math.sqrt(float(var_x)) * math.sqrt(float(var_y)))


def fusion_scores(stats):
    """-> dict of float64 arrays of length B, keys SCORE_NAMES (one read-back of the histograms; host arithmetic on the
    integers: the moments as exact Python integers, the rest in float64).  With f the luma of the fused image, a the infrared
    image, v the luma of the visible one and p the normalised histograms:

      EN   = - sum_i p_f(i) log2 p_f(i)   (0 log 0 = 0), p_f the marginal of joint_fa
      MI   = MI(f, a) + MI(f, v),  MI(x, y) = sum p_xy log2(p_xy / (p_x p_y)) over non-empty bins
      SD   = sqrt(sum (f - mean f)^2 / (H W))
      SF   = sqrt(RF^2 + CF^2),  RF^2 = sums[1] / (H W),  CF^2 = sums[2] / (H W)
      AG   = ag / ((H - 1)(W - 1))
      CC   = (r(f, a) + r(f, v)) / 2,  r = Pearson correlation
      PSNR = 10 log10(255^2 / ((MSE(f, a) + MSE(f, v)) / 2))   (inf when the denominator is 0)
      SCD  = r(f - v, a) + r(f - a, v)

    A correlation with a zero-variance argument is NaN (compute_results' convention for empty classes).  AG alone needs H and W
    separately: they come from stats.shape, which fusion_stats fills in.  Out of scope: Qabf, VIF, MS-SSIM (losses.ssim exists
    for SSIM)."""
    if stats.shape is None:
        raise RuntimeError("fusion_scores: stats.shape = (H, W) is missing (AG divides by (H - 1)(W - 1))")
    H, W = stats.shape
    jfa, jfv = _host(stats.joint_fa).astype(np.int64), _host(stats.joint_fv).astype(np.int64)
    sums, ag = _host(stats.sums).astype(np.int64), _host(stats.ag).astype(np.float64)
    B = jfa.shape[0]
    lev = np.arange(256, dtype=np.int64)
    out = {k: np.empty(B, dtype=np.float64) for k in SCORE_NAMES}
    for b in range(B):
        n = int(sums[b, 3])
        if n != H * W:
            raise RuntimeError(f"fusion_scores: image {b} counts {n} pixels, stats.shape says {H} x {W}")
        hf, ha, hv = jfa[b].sum(axis=1), jfa[b].sum(axis=0), jfv[b].sum(axis=0)
        s_f, s_a, s_v = int(hf @ lev), int(ha @ lev), int(hv @ lev)
        s_ff, s_aa, s_vv = int(hf @ (lev * lev)), int(ha @ (lev * lev)), int(hv @ (lev * lev))
        s_fa, s_fv, s_av = int(lev @ jfa[b] @ lev), int(lev @ jfv[b] @ lev), int(sums[b, 0])
        # central moments times n^2, exact
        v_f, v_a, v_v = n * s_ff - s_f * s_f, n * s_aa - s_a * s_a, n * s_vv - s_v * s_v
        c_fa, c_fv, c_av = n * s_fa - s_f * s_a, n * s_fv - s_f * s_v, n * s_av - s_a * s_v
        out["EN"][b] = -float(_plogp(hf / n).sum())
        out["MI"][b] = _mutual_information(jfa[b], n) + _mutual_information(jfv[b], n)
        out["SD"][b] = math.sqrt(float(v_f)) / n
        out["SF"][b] = math.sqrt((int(sums[b, 1]) + int(sums[b, 2])) / n)
        out["AG"][b] = ag[b] / ((H - 1) * (W - 1))
        out["CC"][b] = 0.5 * (_pearson(c_fa, v_f, v_a) + _pearson(c_fv, v_f, v_v))
        sq = (s_ff - 2 * s_fa + s_aa) + (s_ff - 2 * s_fv + s_vv)  # n (MSE(f, a) + MSE(f, v))
        out["PSNR"][b] = 10.0 * math.log10(255.0 ** 2 / (sq / (2 * n))) if sq > 0 else float("inf")
        out["SCD"][b] = (_pearson(c_fa - c_av, v_f - 2 * c_fv + v_v, v_a) + _pearson(c_fv - c_av, v_f - 2 * c_fa + v_a, v_v))
    return out


def colorize(labels, palette=MFNET_PALETTE):
    """labels: int32 device tensor of any shape -> (..., 3) uint8, out = palette[labels]; a label outside the palette is
    black (util/util.py:21-29 leaves unmatched pixels zero).  palette: (K, 3) uint8, K <= 256, array or device tensor."""
    labels = _dev(labels, "labels", torch.int32)
    pal = palette if isinstance(palette, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(palette, dtype=np.uint8))
    if pal.dim() != 2 or pal.shape[1] != 3 or pal.dtype != torch.uint8 or not 1 <= pal.shape[0] <= 256:
        raise RuntimeError("palette must be (K, 3) uint8 with 1 <= K <= 256")
    pal = pal.to(labels.device).contiguous()
    out = torch.empty(tuple(labels.shape) + (3,), device=labels.device, dtype=torch.uint8)
    _lib.check(_lib.load().segmif_palette_u8(labels.data_ptr(), pal.data_ptr(), out.data_ptr(), labels.numel(), pal.shape[0], _stream()),
               "segmif_palette_u8")
    return out
