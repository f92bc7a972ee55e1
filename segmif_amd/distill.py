"""Knowledge distillation of the segmentation net: a frozen large teacher supervises a small student in the segmentation phase -
this project's addition, NOT the reference's training, which trains one net on labels alone.

  FrozenTeacher   a Network3 in eval mode whose parameters take no gradient; logits() runs it under no_grad through
                  Network3._segment_nhwc, i.e. on the guarded inference path
  DistillStep     one optimizer step on a labelled batch: ONE student forward, the supervised loss on its logits plus `weight` times
                  a losses.DistillObjective between those logits and the teacher's (csrc/distill_objective.hip), one backward

The two objectives are per-pixel KD (Hinton et al. 2015) and channel-wise distillation on the logit maps (CWD, Shu et al., ICCV
2021); both compare the two nets' quarter-resolution outputs, so no bilinear step is involved.  What differs from the papers: the
temperatures and the weight are this project's defaults (losses.DISTILL_TEMPERATURES, weight 3.0), there is no feature-map term (the
channel counts differ between backbones), no ignore mask or weights on the distillation term, and the teacher sees the very batch
the student sees.  Nothing here says what distillation does to a data set's mIoU: that takes a run on a data set."""
import math

import torch

from . import losses


class FrozenTeacher:
    """module: a Network3 (any backbone) with its weights loaded.  It is put in eval mode and its parameters are set to
    requires_grad_(False); nothing is copied.  The teacher is kept as it is for the whole run: it has no refresh()."""

    def __init__(self, module):
        if not hasattr(module, "_segment_nhwc"):
            raise TypeError(f"FrozenTeacher: module must be a Network3 (it is run through _segment_nhwc), got {type(module).__name__}")
        self.module = module.eval()
        for p in self.module.parameters():
            p.requires_grad_(False)

    @torch.no_grad()
    def logits(self, images):
        """(B, 3, H, W) -> the teacher's NHWC quarter-resolution logits (Network3._segment_nhwc, inside its guarded scope)"""
        self.module.eval()
        return self.module._segment_nhwc(images)


class DistillStep:
    """One optimizer step of the student on a labelled batch (x, y):
        1. seg = student._segment_nhwc(x)                        - the ONE student forward
        2. loss_sup = seg_criterion_loss(seg, y, criterion)      - whatever path `criterion` takes in seg_train_step
        3. loss_kd = objective.forward_nhwc(seg, teacher.logits(x))
        4. one backward of loss_sup + weight * loss_kd; reducer.finish() where there is a reducer; one optimizer.step()
    step() returns (loss_sup, loss_kd) detached.  objective: a losses.DistillObjective; weight: finite and > 0 (3.0 is this
    project's default).  Not graph-captured."""

    def __init__(self, student, teacher, optimizer, criterion, objective, weight=3.0, reducer=None):
        if not isinstance(teacher, FrozenTeacher):
            raise TypeError(f"DistillStep: teacher must be a FrozenTeacher, got {type(teacher).__name__}")
        if not isinstance(objective, losses.DistillObjective):
            raise TypeError(f"DistillStep: objective must be a losses.DistillObjective, got {type(objective).__name__}")
        weight = float(weight)
        if not (math.isfinite(weight) and weight > 0.0):
            raise ValueError(f"DistillStep: weight must be finite and > 0, got {weight}")
        self.student, self.teacher, self.opt, self.crit = student, teacher, optimizer, criterion
        self.objective, self.weight, self.reducer = objective, weight, reducer

    def step(self, x, y):
        from .core.model_fusion import seg_criterion_loss
        from .train import _zero_grads
        _zero_grads(self.opt, self.reducer)
        seg = self.student._segment_nhwc(x)
        loss_sup = seg_criterion_loss(seg, y, self.crit)
        loss_kd = self.objective.forward_nhwc(seg, self.teacher.logits(x))
        (loss_sup + self.weight * loss_kd).backward()
        if self.reducer is not None:
            self.reducer.finish()
        self.opt.step()
        return loss_sup.detach(), loss_kd.detach()
