"""Fusion-quality scores of a fused image against its infrared and visible sources, from statistics gathered on the device,
and the palette rendering of a label map (util/util.py:8-29).

  fusion_stats    one pass over three uint8 images per pair (csrc/fusion_stats.hip): two 256 x 256 joint histograms, the
                  squared-difference sums and the gradient sum, per image; all integers but the last
  fusion_scores   EN / MI / SD / SF / AG / CC / PSNR / SCD per image: float64 host arithmetic on those integers
  structural_stats   the local-window sums behind Qabf, SSIM and VIF of the same three planes (csrc/structural_stats.hip), fp64
  structural_scores  Qabf / SSIM / VIF per image from those sums
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

StructuralStats = collections.namedtuple("StructuralStats", ["qabf", "ssim", "vif", "shape"], defaults=(None,))
StructuralStats.__doc__ = """Device tensors, float64, per image b: qabf (B, 2) = [sum (Q_AF gA + Q_VF gV), sum (gA + gV)]; ssim (B, 2) =
the sums of the SSIM maps of (f, a) and (f, v) over the H W pixels; vif (B, 2, 4, 2) = [source a | v][scale 1 .. 4][num, den] of
the pixel-domain VIF; shape = (H, W), host side.  f, v, a as in FusionStats."""

STRUCTURAL_SCORE_NAMES = ("Qabf", "SSIM", "VIF")  # opt-in: not part of SCORE_NAMES

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


def structural_stats(fused_u8, vis_u8, ir_u8, out=None):
    """fused_u8, vis_u8: (B, H, W, 3) uint8, ir_u8: (B, H, W) uint8, all on the device, H, W >= 41 (the fourth VIF scale needs
    them) -> StructuralStats.  Bitwise reproducible, and a pair's sums do not depend on what else is in the batch.  out=: a
    StructuralStats whose buffers are reused (they are overwritten).  No host round trip, capturable in a graph."""
    fused_u8, vis_u8, ir_u8 = _dev(fused_u8, "fused_u8", torch.uint8), _dev(vis_u8, "vis_u8", torch.uint8), _dev(ir_u8, "ir_u8", torch.uint8)
    if fused_u8.dim() != 4 or fused_u8.shape[3] != 3 or vis_u8.shape != fused_u8.shape or tuple(ir_u8.shape) != tuple(fused_u8.shape[:3]):
        raise RuntimeError(f"structural_stats expects (B, H, W, 3), (B, H, W, 3) and (B, H, W), got {tuple(fused_u8.shape)}, "
                           f"{tuple(vis_u8.shape)}, {tuple(ir_u8.shape)}")
    B, H, W, _ = fused_u8.shape
    dev = fused_u8.device
    lib = _lib.load()
    nbytes = lib.segmif_structural_stats_workspace_bytes(B, H, W)
    if nbytes <= 0:
        raise RuntimeError(f"structural_stats: unsupported size B = {B}, H = {H}, W = {W} (H, W >= 41: the four VIF scales leave a "
                           "1 x 1 map at 41; B >= 1; H W <= 2^30)")
    st = StructuralStats(_buffer(out, "qabf", (B, 2), torch.float64, dev), _buffer(out, "ssim", (B, 2), torch.float64, dev),
                         _buffer(out, "vif", (B, 2, 4, 2), torch.float64, dev), (H, W))
    ws = torch.empty((nbytes // 8,), device=dev, dtype=torch.int64)
    _lib.check(lib.segmif_structural_stats_u8(fused_u8.data_ptr(), vis_u8.data_ptr(), ir_u8.data_ptr(), st.qabf.data_ptr(),
                                              st.ssim.data_ptr(), st.vif.data_ptr(), ws.data_ptr(), B, H, W, _stream()),
               "segmif_structural_stats_u8")
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
    separately: they come from stats.shape, which fusion_stats fills in.  Qabf, SSIM and VIF are separate and opt-in
    (structural_stats / structural_scores).  Out of scope: MS-SSIM."""
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


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.nan, num / np.where(den == 0, 1.0, den))


def structural_scores(stats):
    """-> dict of float64 arrays of length B: Qabf, SSIM, VIF (STRUCTURAL_SCORE_NAMES) and their parts SSIM_ir, SSIM_vis, VIF_ir,
    VIF_vis.  With f the luma of the fused image, a the infrared image and v the luma of the visible one, all integers 0 .. 255:

      Qabf  Xydeas-Petrovic with L = 1.  sx = x * [[-1,0,1],[-2,0,2],[-1,0,1]], sy = x * [[1,2,1],[0,0,0],[-1,-2,-1]] ("same"
            true convolutions, zero padding), g = sqrt(sx^2 + sy^2), alpha = pi/2 where sx == 0, else atan(sy / sx).  For a
            source S: G = gF / gS if gS > gF, gF if gS == gF (a magnitude, as the published code has it), else gS / gF;
            A = 1 - |alphaS - alphaF| / (pi/2); Q_SF = 0.9994 / (1 + exp(-15 (G - 0.5))) * 0.9879 / (1 + exp(-22 (A - 0.8))).
            Qabf = sum (Q_AF gA + Q_VF gV) / sum (gA + gV); NaN when the denominator is 0 (three flat images).
      SSIM  = (SSIM_ir + SSIM_vis) / 2 - the MEAN of the two, where some toolkits print the sum.  SSIM_ir / SSIM_vis = the
            mean over the H W pixels of pytorch_ssim's map for (f / 255, a / 255) and (f / 255, v / 255): 11 x 11 Gaussian,
            sigma 1.5, zero padding of 5, C1 = 0.01^2, C2 = 0.03^2.
      VIF   = VIF_ir + VIF_vis, each vifp(source, f) in the pixel domain with sigma_nsq = 2 on the 0 .. 255 values: scales
            1 .. 4 with N = 17, 9, 5, 3, "valid" N x N Gaussians of sd = N / 5, for scale > 1 both images filtered and every
            second row and column kept; s1, s2 clipped at 0, g = s12 / (s1 + 1e-10), sv = s2 - g s12, then in this order
            s1 < 1e-10: g = 0, sv = s2, s1 = 0; s2 < 1e-10: g = 0, sv = 0; g < 0: sv = s2, g = 0; sv <= 1e-10: sv = 1e-10;
            vifp = sum log10(1 + g^2 s1 / (sv + 2)) / sum log10(1 + s1 / 2) over the four scales; NaN when the denominator is 0
            (a black source).

    Qabf and VIF follow these formulas, not an external implementation.  VIF of a plane that is constant but not zero is
    undefined: the rounding noise of its local variances (5e-11 for an all-255 plane) sits at the 1e-10 thresholds, so another
    summation order can cross them."""
    if stats.shape is None:
        raise RuntimeError("structural_scores: stats.shape = (H, W) is missing (SSIM divides by H W)")
    H, W = stats.shape
    qabf, ssim, vif = (_host(t).astype(np.float64) for t in (stats.qabf, stats.ssim, stats.vif))
    B = qabf.shape[0]
    if qabf.shape != (B, 2) or ssim.shape != (B, 2) or vif.shape != (B, 2, 4, 2):
        raise RuntimeError(f"structural_scores: expected (B, 2), (B, 2) and (B, 2, 4, 2), got {qabf.shape}, {ssim.shape}, {vif.shape}")
    out = {"Qabf": _ratio(qabf[:, 0], qabf[:, 1]), "SSIM_ir": ssim[:, 0] / (H * W), "SSIM_vis": ssim[:, 1] / (H * W)}
    out["SSIM"] = 0.5 * (out["SSIM_ir"] + out["SSIM_vis"])
    for s, name in enumerate(("VIF_ir", "VIF_vis")):
        num, den = np.zeros(B), np.zeros(B)
        for k in range(4):
            num, den = num + vif[:, s, k, 0], den + vif[:, s, k, 1]
        out[name] = _ratio(num, den)
    out["VIF"] = out["VIF_ir"] + out["VIF_vis"]
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
