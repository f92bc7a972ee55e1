"""The fusion objectives of the reference's core/loss.py, which its train.py pulls in with a star-import (train.py:111-112).

On the reference's executed path are Fusionloss3 (round 1, core/loss.py:459-476), Fusionloss_grad3 (rounds >= 2, :506-517), Sobelxy
(:634-650) and RGB2YCrCb; they wrap the dedicated kernels of segmif_amd.losses.  The other fusion objectives of the file - Fusionloss,
Fusionloss2, Fusionloss4, Fusionloss6, Fusionloss_add, Fusionloss_grad, Fusionloss_grad2, new_loss_sobel, Total_fusion_loss,
Total_fusion_loss2, Total_fusion_loss3 (:386-397, :423-457, :479-505, :518-603) - are never instantiated by the reference's scripts; here
each is a table of losses.ObjTerm entries evaluated by one HIP kernel pair (losses.fusion_objective), plus LapLoss2 / SSIM where the
reference adds them.  Constructor and forward signatures, argument orders and the `[:, :1]` slices are the reference's; every forward
argument defaults to None and a call without tensors raises NotImplementedError (device tensors the kernels do not cover raise
RuntimeError, as everywhere in the package).

OhemCELoss, SoftmaxFocalLoss and NormalLoss (:342-383) are the segmentation phase's: each holds a losses.SegObjective, whose forward
and backward are one HIP kernel pair (csrc/seg_objective.hip) - OHEM without the sort and without its host synchronisation, so it runs
inside GraphedSegTrainStep.  They take device tensors only.

Left out: IQALoss (:605-633; needs core/Entropy.py) and the detection losses (:1-340).
"""
import torch
import torch.nn as nn

from .. import losses
from ..losses import ObjTerm
from .model_fusion import RGB2YCrCb  # noqa: F401

__all__ = ["Sobelxy", "Fusionloss3", "Fusionloss_grad3", "LapLoss2", "RGB2YCrCb", "Total_fusion_loss", "Total_fusion_loss2",
           "Fusionloss", "Fusionloss_add", "Fusionloss2", "Fusionloss4", "Fusionloss6", "Fusionloss_grad", "Fusionloss_grad2",
           "Total_fusion_loss3", "new_loss_sobel", "OhemCELoss", "SoftmaxFocalLoss", "NormalLoss"]


class Sobelxy(nn.Module):
    def forward(self, x):
        return losses.sobel_xy(x)


class Fusionloss3(nn.Module):
    """L1(mask_0, fused) + L1(Sobel(mask_0), Sobel(fused)); image_ir / image_vis are accepted and unused,
    as in the reference."""

    def __init__(self):
        super().__init__()
        self.sobelconv = Sobelxy()

    def forward(self, image_ir, image_vis, generate_img, mask):
        return losses.fusion_loss3(generate_img, mask)


class LapLoss2(nn.Module):
    """lap_loss.py:100-118: three Gaussian-difference levels (3 / 5 / 7 taps, sigma 2) of the fused image against the
    pixel-wise maximum of the same levels of the two sources; the `device` argument is accepted for signature
    compatibility (the windows are constants of the HIP kernel)."""

    def __init__(self, max_levels=3, channels=1, device=None):
        super().__init__()
        if max_levels != 3 or channels != 1:
            raise NotImplementedError("LapLoss2 is built for the reference's only use: 3 levels, single-channel images")
        self.max_levels = max_levels

    def forward(self, input, ir, vis):
        return losses.lap_loss2(input, ir, vis)


class Fusionloss_grad3(nn.Module):
    """MSE(mask_0, fused) + 1.1 * (1 - SSIM(fused, mask_0)).  Like the reference (core/loss.py:509) it owns a LapLoss2
    that its forward never evaluates; segmif_amd.train.FusionTrainer(report_lap=True) reports that term beside the loss."""

    def __init__(self):
        super().__init__()
        self.lap = LapLoss2()

    def forward(self, image_ir, image_vis, generate_img, mask):
        return losses.fusion_loss_grad3(generate_img, mask)


# ---- the table-driven objectives ---------------------------------------------------------------------------------------------------
_IN_MAX = ObjTerm("identity", "max")                    # L1(max(ir, y), gen)
_GRAD_MAX = ObjTerm("sobel", "max")                     # L1(max(S ir, S y), S gen)
_IN_MASK = ObjTerm("identity", "linear", a_mask=1.0)    # L1(mask_0, gen)
# new_loss_sobel's four means A, B, C, D (see the class)
_NLS = (ObjTerm("identity", "linear", "mask", "square", a_ir=1.0), ObjTerm("identity", "linear", "inv_mask", "square", a_vis=1.0),
        ObjTerm("sobel", "linear", "one", "square", a_ir=1.0), ObjTerm("sobel", "linear", "one", "square", a_vis=1.0))


def _nls_combine(m):
    A, B, C, D = m[0], m[1], m[2], m[3]
    return (B + B * B * D) + 0.85 * (A + A * A * C)


def _tensors(name, accepted, *args):
    if not all(torch.is_tensor(a) for a in args):
        raise NotImplementedError(f"core.{name}.forward takes torch tensors ({accepted}), got "
                                  + ", ".join(type(a).__name__ for a in args))


class _Objective(nn.Module):
    """forward(image_ir, image_vis, generate_img, mask) of the reference's 4-argument objectives: the Y plane of image_vis, channel
    0 of image_ir and of the mask (core/loss.py's `[:, :1]` slices), then the class's table."""
    TERMS, ARGS = (), "image_ir, image_vis, generate_img, mask"

    def __init__(self):
        super().__init__()
        self.sobelconv = Sobelxy()

    @staticmethod
    def combine(m):
        raise NotImplementedError

    def forward(self, image_ir=None, image_vis=None, generate_img=None, mask=None):
        _tensors(type(self).__name__, self.ARGS, image_ir, image_vis, generate_img, mask)
        return losses.fusion_objective(self.TERMS, self.combine, generate_img, image_ir[:, :1], image_vis[:, :1], mask[:, :1])


class _Objective3(_Objective):
    """the reference's 3-argument objectives; a fourth argument (FusionTrainer's hook passes the mask) is accepted and not read"""
    ARGS = "image_ir, image_vis, generate_img"

    def forward(self, image_ir=None, image_vis=None, generate_img=None, mask=None):
        _tensors(type(self).__name__, self.ARGS, image_ir, image_vis, generate_img)
        return losses.fusion_objective(self.TERMS, self.combine, generate_img, image_ir[:, :1], image_vis[:, :1])


class Fusionloss(_Objective3):
    """core/loss.py:423-440: L1(max(ir, y), gen) + 8 L1(max(S ir, S y), S gen) - the max-intensity + max-gradient loss."""
    TERMS = (_IN_MAX, _GRAD_MAX)
    combine = staticmethod(lambda m: m[0] + 8 * m[1])


class Fusionloss_add(_Objective3):
    """core/loss.py:555-572: 1.5 L1(0.4 y + 0.6 ir, gen) + 5 L1(max(S ir, S y), S gen)."""
    TERMS = (ObjTerm("identity", "linear", a_ir=0.6, a_vis=0.4), _GRAD_MAX)
    combine = staticmethod(lambda m: 1.5 * m[0] + 5 * m[1])


class Fusionloss2(_Objective):
    """core/loss.py:441-457: L1(mask_0, gen)."""
    TERMS = (_IN_MASK,)
    combine = staticmethod(lambda m: m[0])


class Fusionloss4(_Objective):
    """core/loss.py:538-553: L1((y + ir) / 2, gen) + 4 L1(S((y + ir) / 2), S gen); the mask is accepted and not read."""
    TERMS = (ObjTerm("identity", "linear", a_ir=0.5, a_vis=0.5), ObjTerm("sobel", "linear", a_ir=0.5, a_vis=0.5))
    combine = staticmethod(lambda m: m[0] + 4 * m[1])


class Fusionloss6(_Objective):
    """core/loss.py:518-537: 0.5 L1(mask_0, gen) + 0.5 L1(y + ir, gen) + 6 L1(max(S ir, S y), S gen)."""
    TERMS = (_IN_MASK, ObjTerm("identity", "linear", a_ir=1.0, a_vis=1.0), _GRAD_MAX)
    combine = staticmethod(lambda m: 0.5 * m[0] + 0.5 * m[1] + 6 * m[2])


class Fusionloss_grad(_Objective):
    """core/loss.py:479-490: L1(mask_0, gen) + 0.8 LapLoss2(gen, ir, y)."""
    TERMS = (_IN_MASK,)
    combine = staticmethod(lambda m: m[0])

    def __init__(self):
        super().__init__()
        self.lap = LapLoss2()

    def forward(self, image_ir=None, image_vis=None, generate_img=None, mask=None):
        loss_in = super().forward(image_ir, image_vis, generate_img, mask)
        return loss_in + 0.8 * self.lap(generate_img, image_ir[:, :1], image_vis[:, :1])


class Fusionloss_grad2(_Objective):
    """core/loss.py:492-505: L1(mask_0, gen) + 0.1 LapLoss2(gen, y, ir) + 1.1 (1 - SSIM(gen, mask_0)) - LapLoss2's sources in the
    order the reference passes them there (the maximum is symmetric in them)."""
    TERMS = (_IN_MASK,)
    combine = staticmethod(lambda m: m[0])

    def __init__(self):
        super().__init__()
        self.lap = LapLoss2()

    def forward(self, image_ir=None, image_vis=None, generate_img=None, mask=None):
        loss_in = super().forward(image_ir, image_vis, generate_img, mask)
        return (loss_in + 0.1 * self.lap(generate_img, image_vis[:, :1], image_ir[:, :1])
                + 1.1 * losses.ssim_loss(generate_img, mask[:, :1]))


class new_loss_sobel(nn.Module):
    """core/loss.py:386-397, as upstream COMPUTES it: lines 393-394 rebind mask_ir and mask_vis to the two scalar losses
        A = MSE(m gen, m ir),  B = MSE(|1 - m| gen, |1 - m| vis)          (m: every channel of the mask)
    before lines 395-396 use those names as the weights of the gradient terms, which are therefore MSE(A S gen, A S ir) = A^2 C
    and B^2 D with C = MSE(S gen, S ir), D = MSE(S gen, S vis).  Result: (B + B^2 D) + 0.85 (A + A^2 C).  No slices here: ir, vis
    and fused_img are single-channel, the mask has 1..4 channels."""
    TERMS = _NLS
    combine = staticmethod(_nls_combine)

    def __init__(self):
        super().__init__()
        self.sobel = Sobelxy()

    def forward(self, ir=None, vis=None, mask_ir=None, fused_img=None):
        _tensors(type(self).__name__, "ir, vis, mask_ir, fused_img", ir, vis, mask_ir, fused_img)
        return losses.fusion_objective(self.TERMS, self.combine, fused_img, ir, vis, mask_ir)


class _Total(nn.Module):
    """forward(image_ir, image_vis, mask, generate_img) - the reference's order for these three - on channel 0 of image_ir and
    image_vis and the whole mask."""
    TERMS = ()

    @staticmethod
    def combine(m):
        raise NotImplementedError

    def forward(self, image_ir=None, image_vis=None, mask=None, generate_img=None):
        _tensors(type(self).__name__, "image_ir, image_vis, mask, generate_img", image_ir, image_vis, mask, generate_img)
        return losses.fusion_objective(self.TERMS, self.combine, generate_img, image_ir[:, :1], image_vis[:, :1], mask)


class Total_fusion_loss(_Total):
    """core/loss.py:573-582: 1.2 Fusionloss + 0.85 new_loss_sobel: six terms, one launch."""
    TERMS = (_IN_MAX, _GRAD_MAX) + _NLS
    combine = staticmethod(lambda m: 1.2 * (m[0] + 8 * m[1]) + 0.85 * _nls_combine(m[2:]))

    def __init__(self):
        super().__init__()
        self.nls, self.fl = new_loss_sobel(), Fusionloss()


class Total_fusion_loss2(_Total):
    """core/loss.py:585-593: new_loss_sobel."""
    TERMS = _NLS
    combine = staticmethod(_nls_combine)

    def __init__(self):
        super().__init__()
        self.nls = new_loss_sobel()


class Total_fusion_loss3(_Total):
    """core/loss.py:595-603: 3 Fusionloss; the mask is accepted and not read."""
    TERMS = (_IN_MAX, _GRAD_MAX)
    combine = staticmethod(lambda m: 3 * (m[0] + 8 * m[1]))

    def __init__(self):
        super().__init__()
        self.fl = Fusionloss()


# ---- the segmentation objectives (core/loss.py:342-383) ------------------------------------------------------------------------------
class OhemCELoss(losses.SegObjectiveLoss):
    """core/loss.py:342-358: per-pixel CE; the mean of the losses above -log(thresh) when at least n_min of them are, else the mean
    of the n_min largest (ignored pixels' zeros included).  self.thresh is -log(thresh) in float32, as in the reference."""

    def __init__(self, thresh, n_min, ignore_lb=255, *args, **kwargs):
        super().__init__(losses.SegObjective(ignore_index=ignore_lb, reduction="ohem", ohem_thresh=thresh, ohem_n_min=n_min))
        self.thresh, self.n_min, self.ignore_lb = self.objective.ohem_t, self.objective.ohem_n_min, ignore_lb


class SoftmaxFocalLoss(losses.SegObjectiveLoss):
    """core/loss.py:361-373: NLLLoss(ignore_lb) of (1 - softmax)^gamma * log_softmax, mean over the valid pixels."""

    def __init__(self, gamma, ignore_lb=255, *args, **kwargs):
        if not gamma > 0:
            raise ValueError(f"SoftmaxFocalLoss: gamma must be > 0 (gamma = 0 is cross entropy: NormalLoss or nn.CrossEntropyLoss), got {gamma}")
        super().__init__(losses.SegObjective(gamma=gamma, ignore_index=ignore_lb))
        self.gamma = gamma


class NormalLoss(losses.SegObjectiveLoss):
    """core/loss.py:375-383: torch.mean of CrossEntropyLoss(ignore_lb, reduction='none') - ignored pixels count in the mean."""

    def __init__(self, ignore_lb=255, *args, **kwargs):
        super().__init__(losses.SegObjective(ignore_index=ignore_lb, reduction="mean_all"))
