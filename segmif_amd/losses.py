"""Fusion losses used by the reference's train_fusion (core/loss.py:459-476 Fusionloss3, :506-517
Fusionloss_grad3, :634-650 Sobelxy; pytorch_ssim/__init__.py:8-43) and LapLoss2 (lap_loss.py:100-118).

On the GPU both objectives are fused HIP kernels, forward and backward (csrc/losses.hip + the separable blur of
csrc/rowops.hip; autograd.FusionLossGrad3Fn / FusionLoss3Fn): SURVEY §8(f) N1.  Device tensors the kernels do not cover
(non-fp32, more than one channel, mismatched shapes) are REFUSED like everywhere else in the package - there is no torch /
MIOpen fallback on the GPU.  The torch formulations below run on CPU tensors only: they are what the CPU tests pin against
the reference (tests/golden/losses.npz).

fusion_objective is the general form behind the remaining objectives of core/loss.py: a table of up to 8 terms
mean rho(w (L(gen) - t)) and a function combining their means; one HIP kernel pair (csrc/fusion_objective.hip) serves every table.

SegObjective is the segmentation phase's counterpart: cross entropy with class weights / label smoothing, the focal loss, and the
three reductions (mean over valid pixels, mean over all pixels, OHEM) of core/loss.py:342-383 on one HIP kernel pair
(csrc/seg_objective.hip).  Device float32 logits only: there is no torch formulation of it in the package.

RegionObjective adds the region objectives - Lovasz-Softmax and soft Dice (csrc/region_objective.hip) - and SegLossSum adds one of
them to a per-pixel criterion on the same logits.  Neither is the reference's.

DistillObjective is the distillation term between a student's and a frozen teacher's logits - per-pixel KD or channel-wise
distillation (csrc/distill_objective.hip) - that segmif_amd.distill.DistillStep adds to the supervised loss.  Not the reference's.
"""
import math
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def _gaussian_window(size=11, sigma=1.5, device=None, dtype=torch.float32):
    g = torch.tensor([math.exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)], dtype=dtype)
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).to(device)[None, None]


def ssim(img1, img2, window_size=11):
    """Gaussian-window SSIM averaged over the image (single channel per group).  On the GPU the five
    window convolutions (and their backward) run in the separable HIP blur kernel."""
    C = img1.shape[1]
    if img1.is_cuda:
        if window_size != 11 or img1.dtype != torch.float32 or img2.dtype != torch.float32 or not img2.is_cuda:
            raise RuntimeError("segmif_amd.losses.ssim: the HIP blur kernel is the 11-tap float32 one (no torch fallback on the GPU)")
        from . import autograd as ag
        blur = ag.gauss_blur11
    else:
        w = _gaussian_window(window_size, 1.5, img1.device, img1.dtype).expand(C, 1, window_size, window_size).contiguous()
        pad = window_size // 2
        blur = lambda t: F.conv2d(t, w, padding=pad, groups=C)
    mu1, mu2 = blur(img1), blur(img2)
    s11 = blur(img1 * img1) - mu1 * mu1
    s22 = blur(img2 * img2) - mu2 * mu2
    s12 = blur(img1 * img2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()


def _hip_ok(generate_img, *others):
    """True: the fused HIP kernels take it; False: CPU tensors (the torch formulation, test infrastructure); a device
    tensor the kernels do not cover raises - no library-convolution fallback on the GPU."""
    ts = (generate_img,) + others
    if not any(t.is_cuda for t in ts):
        return False
    if all(t.is_cuda and t.dtype == torch.float32 and t.shape == generate_img.shape for t in ts) and generate_img.shape[1] == 1:
        return True
    raise RuntimeError("segmif_amd.losses: the fused loss kernels take float32 single-channel device tensors of one shape, got "
                       + ", ".join(f"{tuple(t.shape)} {t.dtype} {t.device.type}" for t in ts) + " (no torch fallback on the GPU)")


def fusion_loss_grad3(generate_img, mask):
    """MSE(mask_0, fused) + 1.1 * (1 - SSIM(fused, mask_0))  — the round >= 2 intensity term."""
    m = mask[:, :1]
    if _hip_ok(generate_img, m):
        from . import autograd as ag
        return ag.FusionLossGrad3Fn.apply(generate_img, m.detach())
    return F.mse_loss(m, generate_img) + 1.1 * (1 - ssim(generate_img, m))


def sobel_xy(x):
    """|Sobel_x| + |Sobel_y| with zero padding (core/loss.py:634-650), written as shifted differences so
    that neither the forward nor the backward goes through a library convolution."""
    p = F.pad(x, (1, 1, 1, 1))
    top, mid, bot = p[:, :, :-2], p[:, :, 1:-1], p[:, :, 2:]
    gx = (top[..., 2:] + 2 * mid[..., 2:] + bot[..., 2:]) - (top[..., :-2] + 2 * mid[..., :-2] + bot[..., :-2])
    gy = (top[..., :-2] + 2 * top[..., 1:-1] + top[..., 2:]) - (bot[..., :-2] + 2 * bot[..., 1:-1] + bot[..., 2:])
    return gx.abs() + gy.abs()


def fusion_loss3(generate_img, mask):
    """L1(mask_0, fused) + L1(Sobel(mask_0), Sobel(fused))  — the round-1 objective."""
    m = mask[:, :1]
    if _hip_ok(generate_img, m):
        from . import autograd as ag
        return ag.FusionLoss3Fn.apply(generate_img, m.detach())
    return F.l1_loss(m, generate_img) + F.l1_loss(sobel_xy(m), sobel_xy(generate_img))


def _lap_window(size, sigma=2.0, device=None, dtype=torch.float32):
    """lap_loss.py:39-80 `smoothing`: the normalised size x size Gaussian (zero padding size // 2 at the call site)."""
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2.0
    g = torch.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * sigma ** 2))
    return (g / g.sum()).to(dtype).to(device)[None, None]


def lap_loss2(generate_img, ir, vis):
    """LapLoss2.forward (lap_loss.py:100-118): d_k(img) = img - G_k * img for the 3 / 5 / 7-tap sigma-2 Gaussians;
    10 (L1_3 + L1_5) + L1_7 with L1_k = mean |d_k(gen) - max(d_k(ir), d_k(vis))|.  Fusionloss_grad3 builds one and never
    evaluates it (core/loss.py:509); FusionTrainer(report_lap=True) reports it beside the loss (BASELINE config[2])."""
    if _hip_ok(generate_img, ir, vis):
        from . import autograd as ag
        return ag.LapLoss2Fn.apply(generate_img, ir.detach(), vis.detach())
    C = generate_img.shape[1]
    total = 0.0
    for size, coef in ((3, 10.0), (5, 10.0), (7, 1.0)):
        w = _lap_window(size, 2.0, generate_img.device, generate_img.dtype).expand(C, 1, size, size).contiguous()
        d = [t - F.conv2d(t, w, padding=size // 2, groups=C) for t in (generate_img, ir, vis)]
        total = total + coef * F.l1_loss(d[0], torch.maximum(d[1], d[2]))
    return total


def ssim_loss(generate_img, mask):
    """1 - SSIM(fused, mask) alone (the last term of Fusionloss_grad2, core/loss.py:504)."""
    if _hip_ok(generate_img, mask):
        from . import autograd as ag
        return ag.SsimFn.apply(generate_img, mask.detach())
    return 1 - ssim(generate_img, mask)


# ---- the table-driven objectives (csrc/fusion_objective.hip; core/loss.py:386-397, :423-457, :479-505, :518-603) ------------------
OBJ_OPS, OBJ_TARGETS, OBJ_WEIGHTS, OBJ_RHOS = ("identity", "sobel"), ("linear", "max"), ("one", "mask", "inv_mask"), ("abs", "square")
OBJ_MAX_TERMS = 8


class ObjTerm(NamedTuple):
    """mean over pixels (and, for a weighted term, mask channels) of rho(w * (L(gen) - t)):
    op      L: "identity" | "sobel" (sobel_xy)
    target  t: "linear" = L(a_ir ir + a_vis vis + a_mask mask[:, :1]) | "max" = max(L(ir), L(vis))
    weight  w: "one" | "mask" | "inv_mask" = |1 - mask|, broadcast over every channel of the mask
    rho     "abs" | "square" """
    op: str = "identity"
    target: str = "linear"
    weight: str = "one"
    rho: str = "abs"
    a_ir: float = 0.0
    a_vis: float = 0.0
    a_mask: float = 0.0


def objective_needs(terms):
    """(ir, vis, mask): which of the data planes the terms read"""
    ir = any(t.target == "max" or t.a_ir != 0 for t in terms)
    vis = any(t.target == "max" or t.a_vis != 0 for t in terms)
    mask = any(t.weight != "one" or (t.target == "linear" and t.a_mask != 0) for t in terms)
    return ir, vis, mask


def _check_terms(terms, ir, vis, mask):
    if not 1 <= len(terms) <= OBJ_MAX_TERMS:
        raise ValueError(f"fusion_objective takes 1..{OBJ_MAX_TERMS} terms, got {len(terms)}")
    for t in terms:
        if t.op not in OBJ_OPS or t.target not in OBJ_TARGETS or t.weight not in OBJ_WEIGHTS or t.rho not in OBJ_RHOS:
            raise ValueError(f"fusion_objective: unknown entry in {t}")
    for name, need, given in zip(("ir", "vis", "mask"), objective_needs(terms), (ir, vis, mask)):
        if need and given is None:
            raise ValueError(f"fusion_objective: a term reads {name}, which is None")


def objective_means(terms, gen, ir=None, vis=None, mask=None):
    """The terms' means as a 1-D tensor, written with torch ops in gen's dtype (float64-capable): what CPU tensors get, and what
    the tests hold the HIP kernel against."""
    out = []
    for t in terms:
        L = sobel_xy if t.op == "sobel" else (lambda z: z)
        if t.target == "max":
            tgt = torch.maximum(L(ir), L(vis))
        else:
            lin = torch.zeros_like(gen)
            for a, src in ((t.a_ir, ir), (t.a_vis, vis), (t.a_mask, mask[:, :1] if mask is not None else None)):
                if a != 0:
                    lin = lin + a * src
            tgt = L(lin)
        e = L(gen) - tgt
        if t.weight == "mask":
            e = mask * e
        elif t.weight == "inv_mask":
            e = (1 - mask).abs() * e
        out.append(e.abs().mean() if t.rho == "abs" else (e * e).mean())
    return torch.stack(out)


def _objective_hip_ok(terms, gen, ir, vis, mask):
    need_ir, need_vis, need_mask = objective_needs(terms)
    planes = [p for p, need in ((ir, need_ir), (vis, need_vis)) if need]
    ts = [gen] + planes + ([mask] if need_mask else [])
    if not any(t.is_cuda for t in ts):
        return False
    ok = _hip_ok(gen, *planes)  # (raises for what the kernels do not cover)
    if need_mask and not (mask.is_cuda and mask.dtype == torch.float32 and mask.dim() == 4 and 1 <= mask.shape[1] <= 4
                          and mask.shape[:1] + mask.shape[2:] == gen.shape[:1] + gen.shape[2:]):
        raise RuntimeError("segmif_amd.losses: the fusion-objective kernel takes a float32 device mask of 1..4 channels at the fused "
                           f"image's size, got {tuple(mask.shape)} {mask.dtype} {mask.device.type} for a fused image "
                           f"{tuple(gen.shape)} (no torch fallback on the GPU)")
    if not ok:  # only the mask is on the device
        raise RuntimeError("segmif_amd.losses: the fusion-objective kernel takes device tensors only (no torch fallback on the GPU)")
    return True


def fusion_objective(terms, combine, gen, ir=None, vis=None, mask=None):
    """combine(means) for the table `terms` (ObjTerm entries; means: their 1-D tensor) - the general form of the objectives of
    core/loss.py.  gen, ir, vis: (B, 1, H, W); mask: (B, 1..4, H, W), its channel 0 is what a_mask reads.  On the GPU: one HIP
    launch for all the sums and one for the gradient (autograd.FusionObjectiveFn); ir, vis and mask are data."""
    terms = tuple(terms)
    _check_terms(terms, ir, vis, mask)
    if _objective_hip_ok(terms, gen, ir, vis, mask):
        from . import autograd as ag
        return ag.FusionObjectiveFn.apply(gen, terms, combine, ir, vis, mask)
    return combine(objective_means(terms, gen, ir, vis, mask))


# ---- the segmentation objectives (csrc/seg_objective.hip; core/loss.py:342-383) ------------------------------------------------------
SEG_REDUCTIONS = ("mean", "mean_all", "ohem")


class SegObjective(nn.Module):
    """Per-pixel loss l over softmax(logits) and its reduction, forward and backward in csrc/seg_objective.hip:
        gamma == 0   cross entropy with class weights `weight` and label smoothing, torch's F.cross_entropy definition
        gamma > 0    the focal loss -w_y (1 - p_y)^gamma log p_y of SoftmaxFocalLoss (no label smoothing)
        reduction    "mean": sum l / sum of w_y over valid pixels (nn.CrossEntropyLoss / nn.NLLLoss) | "mean_all": sum l / pixels
                     (NormalLoss) | "ohem": OhemCELoss - the mean of the l above -log(ohem_thresh) when there are at least
                     ohem_n_min of them, else the mean of the ohem_n_min largest l (ignored pixels' zeros among them).
    ohem_thresh is a probability, as in the reference.  Pixels labelled ignore_index (or outside [0, C)) have l = 0 and no gradient.
    No host synchronisation: it runs inside GraphedSegTrainStep's capture.  weight is a buffer (it moves with .cuda())."""

    def __init__(self, gamma=0.0, label_smoothing=0.0, weight=None, ignore_index=255, reduction="mean", ohem_thresh=None,
                 ohem_n_min=None):
        super().__init__()
        gamma, label_smoothing = float(gamma), float(label_smoothing)
        if not (math.isfinite(gamma) and gamma >= 0.0):
            raise ValueError(f"SegObjective: gamma must be finite and >= 0, got {gamma}")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"SegObjective: label_smoothing must lie in [0, 1), got {label_smoothing}")
        if gamma > 0.0 and label_smoothing > 0.0:
            raise ValueError("SegObjective: the focal loss (gamma > 0) takes no label smoothing")
        if reduction not in SEG_REDUCTIONS:
            raise ValueError(f"SegObjective: reduction must be one of {', '.join(SEG_REDUCTIONS)}, got {reduction!r}")
        self.ohem_t, self.ohem_n_min = 0.0, 0
        if reduction == "ohem":
            if ohem_thresh is None or ohem_n_min is None:
                raise ValueError("SegObjective: reduction 'ohem' needs ohem_thresh and ohem_n_min")
            # -log(thresh) in float32, as OhemCELoss.__init__ forms it
            t = float(-torch.log(torch.tensor(float(ohem_thresh), dtype=torch.float)))
            if not math.isfinite(t):
                raise ValueError(f"SegObjective: -log(ohem_thresh) must be finite, got ohem_thresh = {ohem_thresh}")
            if int(ohem_n_min) != ohem_n_min or int(ohem_n_min) < 1:
                raise ValueError(f"SegObjective: ohem_n_min must be an integer >= 1, got {ohem_n_min}")
            self.ohem_t, self.ohem_n_min = t, int(ohem_n_min)
        elif ohem_thresh is not None or ohem_n_min is not None:
            raise ValueError("SegObjective: ohem_thresh / ohem_n_min belong to reduction 'ohem'")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone()
            if weight.dim() != 1 or not 1 <= weight.numel() <= 32:
                raise ValueError(f"SegObjective: weight must hold one value per class (1..32), got shape {tuple(weight.shape)}")
            if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError("SegObjective: class weights must be finite and >= 0")
        self.register_buffer("weight", weight)
        self.gamma, self.label_smoothing, self.ignore_index, self.reduction = gamma, label_smoothing, int(ignore_index), reduction

    @classmethod
    def from_criterion(cls, criterion):
        """The SegObjective that computes what an nn.CrossEntropyLoss (mean reduction) does: the explicit opt-in for torch's class,
        which seg_criterion_loss otherwise leaves to torch's kernels when it carries weights or smoothing."""
        if not isinstance(criterion, nn.CrossEntropyLoss):
            raise TypeError(f"SegObjective.from_criterion takes an nn.CrossEntropyLoss, got {type(criterion).__name__}")
        if criterion.reduction != "mean":
            raise ValueError(f"SegObjective.from_criterion: reduction {criterion.reduction!r} has no counterpart (mean only)")
        return cls(label_smoothing=getattr(criterion, "label_smoothing", 0.0), weight=criterion.weight,
                   ignore_index=criterion.ignore_index)

    def extra_repr(self):
        s = f"gamma={self.gamma}, label_smoothing={self.label_smoothing}, ignore_index={self.ignore_index}, reduction={self.reduction!r}"
        return s + (f", ohem_t={self.ohem_t:.6f}, ohem_n_min={self.ohem_n_min}" if self.reduction == "ohem" else "")

    def forward_nhwc(self, logits_nhwc, labels, pixel_weight=None, sample_weight=None):
        """logits_nhwc: (..., C) float32 device rows (a channel slice of a wider buffer is fine); labels: one per row.
        pixel_weight (B, H, W) or (rows,), sample_weight (B,): float32 device DATA (no gradient) that multiply the per-pixel loss and
        leave the reduction's denominator alone (self-training; not the reference's objective).  Both None: the path as it was."""
        from . import autograd as ag
        if (pixel_weight is not None or sample_weight is not None) and self.reduction == "ohem":
            raise TypeError("SegObjective: the 'ohem' reduction takes no pixel_weight / sample_weight (that combination is not built)")
        return ag.seg_objective(logits_nhwc, labels, gamma=self.gamma, label_smoothing=self.label_smoothing, weight=self.weight,
                                ignore_index=self.ignore_index, reduction=self.reduction, ohem_t=self.ohem_t,
                                ohem_n_min=self.ohem_n_min, pixel_weight=pixel_weight, sample_weight=sample_weight)

    def forward(self, logits, labels, pixel_weight=None, sample_weight=None):
        """logits: logical (B, C, H, W), contiguous or channels-last in memory (what ops.as_nchw returns); the gradient comes back
        in the same layout."""
        from . import autograd as ag
        return self.forward_nhwc(ag.nhwc_rows_of(logits), labels, pixel_weight, sample_weight)


class SegObjectiveLoss(nn.Module):
    """Base of the reference-named segmentation losses of core/loss.py: holds a SegObjective and calls it."""

    def __init__(self, objective):
        super().__init__()
        self.objective = objective

    def forward(self, logits, labels):
        return self.objective(logits, labels)  # (the reference's signature; the weights of self-training go through forward_nhwc)

    def forward_nhwc(self, logits_nhwc, labels, pixel_weight=None, sample_weight=None):
        return self.objective.forward_nhwc(logits_nhwc, labels, pixel_weight, sample_weight)


# ---- the region objectives (csrc/region_objective.hip) ----------------------------------------------------------------------------------
REGION_KINDS = ("lovasz", "dice")
REGION_CLASSES = ("present", "all")


class RegionObjective(nn.Module):
    """A region objective over softmax(logits), forward and backward in csrc/region_objective.hip; not the reference's.  A pixel is
    valid when its label lies in [0, C) and is not ignore_index; fg_ic = [y_i == c]; sums over the valid pixels of the whole batch:
        kind "lovasz"  Lovasz-Softmax (Berman et al. 2018, per_image=False): per class the errors e_i = |fg_ic - p_ic| sorted in
                       descending order (bit-equal float32 errors by ascending pixel index), G = sum fg, F_k the foreground pixels
                       among the first k, J_k = 1 - (G - F_k) / (G + k - F_k), loss_c = sum_k e_(k) (J_k - J_{k-1})
        kind "dice"    D_c = 1 - (2 sum p_ic fg_ic + smooth) / (sum p_ic + sum fg_ic + smooth)
        classes        "present": the mean over the classes that have a pixel | "all": over all C (an absent class's Lovasz term
                       is max_i p_ic).  With nothing to average the value is 0 and so is the gradient.
    No host synchronisation: it runs inside GraphedSegTrainStep's capture.  Device float32 logits only."""

    def __init__(self, kind="lovasz", classes="present", ignore_index=255, smooth=1.0):
        super().__init__()
        if kind not in REGION_KINDS:
            raise ValueError(f"RegionObjective: kind must be one of {', '.join(REGION_KINDS)}, got {kind!r}")
        if classes not in REGION_CLASSES:
            raise ValueError(f"RegionObjective: classes must be one of {', '.join(REGION_CLASSES)}, got {classes!r}")
        smooth = float(smooth)
        if not (math.isfinite(smooth) and smooth >= 0.0):
            raise ValueError(f"RegionObjective: smooth must be finite and >= 0, got {smooth}")
        self.kind, self.classes, self.ignore_index, self.smooth = kind, classes, int(ignore_index), smooth

    def extra_repr(self):
        s = f"kind={self.kind!r}, classes={self.classes!r}, ignore_index={self.ignore_index}"
        return s + (f", smooth={self.smooth}" if self.kind == "dice" else "")

    def forward_nhwc(self, logits_nhwc, labels):
        """logits_nhwc: (..., C) float32 device rows (a channel slice of a wider buffer is fine); labels: one per row"""
        from . import autograd as ag
        return ag.region_objective(logits_nhwc, labels, kind=self.kind, classes=self.classes, ignore_index=self.ignore_index,
                                   smooth=self.smooth)

    def forward(self, logits, labels):
        """logits: logical (B, C, H, W), contiguous or channels-last in memory; the gradient comes back in the same layout"""
        from . import autograd as ag
        return self.forward_nhwc(ag.nhwc_rows_of(logits), labels)


class SegLossSum(nn.Module):
    """base(logits, labels) + region_weight * region(logits, labels) on the SAME NHWC logits.  base: an nn.CrossEntropyLoss that the
    softmax-CE kernel covers (mean reduction, no class weights, no label smoothing: it stays on autograd.softmax_ce, the bits it
    has on its own), a SegObjective or a SegObjectiveLoss; region: a RegionObjective."""

    def __init__(self, base, region, region_weight=1.0):
        super().__init__()
        if isinstance(base, nn.CrossEntropyLoss):
            if base.weight is not None or base.reduction != "mean" or getattr(base, "label_smoothing", 0.0) != 0.0:
                raise ValueError("SegLossSum: an nn.CrossEntropyLoss base must have mean reduction, no class weights and no label "
                                 "smoothing (SegObjective.from_criterion covers the rest)")
        elif not isinstance(base, (SegObjective, SegObjectiveLoss)):
            raise TypeError(f"SegLossSum: base must be an nn.CrossEntropyLoss, a SegObjective or a SegObjectiveLoss, got "
                            f"{type(base).__name__}")
        if not isinstance(region, RegionObjective):
            raise TypeError(f"SegLossSum: region must be a RegionObjective, got {type(region).__name__}")
        region_weight = float(region_weight)
        if not (math.isfinite(region_weight) and region_weight > 0.0):
            raise ValueError(f"SegLossSum: region_weight must be finite and > 0, got {region_weight}")
        self.base, self.region, self.region_weight = base, region, region_weight

    def extra_repr(self):
        return f"region_weight={self.region_weight}"

    def base_nhwc(self, logits_nhwc, labels):
        if isinstance(self.base, nn.CrossEntropyLoss):
            from . import autograd as ag
            return ag.softmax_ce(logits_nhwc, labels.type(torch.long), self.base.ignore_index)
        return self.base.forward_nhwc(logits_nhwc, labels)

    def forward_nhwc(self, logits_nhwc, labels):
        return self.base_nhwc(logits_nhwc, labels) + self.region_weight * self.region.forward_nhwc(logits_nhwc, labels)

    def forward(self, logits, labels):
        from . import autograd as ag
        return self.forward_nhwc(ag.nhwc_rows_of(logits), labels)


# ---- the distillation objectives (csrc/distill_objective.hip; include/segmif_distill.h) ------------------------------------------------
DISTILL_KINDS = ("channel", "pixel")
DISTILL_TEMPERATURES = {"channel": 4.0, "pixel": 1.0}  # this project's choice; the CWD paper's logit setting is quoted from memory


class DistillObjective(nn.Module):
    """The distillation term between a student's and a frozen teacher's logits at the same resolution, forward and backward in
    csrc/distill_objective.hip; this project's addition, NOT the reference's objective.  With z = logits / T and lse the
    log-sum-exp over the stated axis:
        kind "pixel"    per-pixel KD (Hinton et al. 2015): softmax over the classes of a pixel,
                        T^2 * mean over pixels of KL(softmax(zt) || softmax(zs))
        kind "channel"  channel-wise distillation (CWD, Shu et al., ICCV 2021) on the logit maps: softmax over the h * w positions of
                        a sample's class map, T^2 * sum of the (B, C) KL terms / (B C)
    temperature None: 4.0 for "channel", 1.0 for "pixel" (this project's choice).  The teacher is data: it gets no gradient, and a
    teacher tensor that requires grad is refused.  No weights, no ignore mask.  No host synchronisation.  Device float32 logits
    only: there is no torch formulation of it in the package."""

    def __init__(self, kind="channel", temperature=None):
        super().__init__()
        if kind not in DISTILL_KINDS:
            raise ValueError(f"DistillObjective: kind must be one of {', '.join(DISTILL_KINDS)}, got {kind!r}")
        temperature = DISTILL_TEMPERATURES[kind] if temperature is None else float(temperature)
        if not (math.isfinite(temperature) and temperature > 0.0):
            raise ValueError(f"DistillObjective: temperature must be finite and > 0, got {temperature}")
        self.kind, self.temperature = kind, temperature

    def extra_repr(self):
        return f"kind={self.kind!r}, temperature={self.temperature}"

    def forward_nhwc(self, student_nhwc, teacher_nhwc):
        """(B, h, w, C) float32 device rows, the same shape for both (a channel slice of a wider buffer is fine)"""
        from . import autograd as ag
        return ag.distill_objective(student_nhwc, teacher_nhwc, kind=self.kind, temperature=self.temperature)

    def forward(self, student, teacher):
        """logical (B, C, h, w), contiguous or channels-last in memory; the student's gradient comes back in its layout"""
        from . import autograd as ag
        if isinstance(student, torch.Tensor) and isinstance(teacher, torch.Tensor):
            if student.shape != teacher.shape:
                raise RuntimeError(f"DistillObjective: student logits {tuple(student.shape)} and teacher logits {tuple(teacher.shape)} "
                                   "differ in shape")
            if teacher.requires_grad:
                raise RuntimeError("DistillObjective: the teacher logits require grad, but the teacher is data and receives no gradient")
        return self.forward_nhwc(ag.nhwc_rows_of(student), ag.nhwc_rows_of(teacher))
