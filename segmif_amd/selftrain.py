"""Self-training of the segmentation net on unlabelled pairs, DAFormer style (Hoyer et al. 2022; the mean teacher of Tarvainen &
Valpola 2017; ClassMix, Olsson et al. 2021) - this project's addition, NOT the reference's training, which uses labelled frames only.

  EmaTeacher        the student's weight average (FusedAdamW(ema_decay=...) / WeightEMA) as a network of its own that SHARES the
                    average's storage: nothing is copied per step
  cross_mix_table   the ClassMix table of a labelled half pasted into an unlabelled half
  cross_mix         that mix on the existing ops.class_mix, the confidence weight riding as a plane
  SelfTrainingStep  teacher logits -> ops.pseudo_label (csrc/pseudo_label.hip) -> optional mix -> optional strong augmentation of
                    the student's input (ops.strong_augment, csrc/strong_augment.hip) -> supervised loss + weighted
                    mean-over-all-pixels CE on the pseudo-labels (csrc/seg_objective.hip's weighted entries) -> one optimizer step

What differs from DAFormer: no feature-distance loss, one domain (the unlabelled frames are more frames of the same sensor pair),
and the teacher's BatchNorm buffers are copied from the student rather than averaged.  DAFormer trains its student on a strongly
augmented copy of the (mixed) image while the teacher labels the clean one; here that is opt-in (strong=, a data.StrongAugment):
without it the student sees the teacher's pixels, and with it the colour jitter's four operations run in one fixed order
(brightness, contrast, saturation, hue; a random order is not built), the blur's support follows sigma (DAFormer's kernel size
follows the image's), and neither the labelled batch nor the geometry of the student's input is touched.  Nothing here says
what it does to mIoU."""
import copy
import math

import numpy as np
import torch

from . import losses, ops
from .utils.optimizer import _bump_versions


class EmaTeacher:
    """source: a FusedAdamW(ema_decay=...) or a WeightEMA over the student's parameters.  The teacher is a deep copy of `student` in
    eval mode, run under no_grad, whose parameters SHARE STORAGE with the averages' `hi` tensors (the float32 rounding of the
    average, what ema_state_dict hands out): the EMA kernel's writes are the teacher's new weights, nothing is copied
    (ema_weights() costs two full copies of the weights per use and is meant for validation).  A parameter that has no average yet
    - the average begins at a parameter's first gradient - reads the student's own tensor, so before the first step the teacher
    is the student, as in DAFormer.

    refresh(), after every optimizer.step(): binds the parameters whose average has appeared since the last call, copies the
    student's buffers (BatchNorm's running statistics; DAFormer averages them) and raises the teacher parameters' version
    counters - the EMA kernel writes through raw pointers, and core/_util.PackedCache would go on serving the packed weights of
    the step before."""

    def __init__(self, source, student):
        if not hasattr(source, "ema_tensors"):
            raise TypeError(f"EmaTeacher: source must be a FusedAdamW(ema_decay=...) or a WeightEMA, got {type(source).__name__}")
        source.ema_tensors()  # (raises for an optimizer that keeps no average)
        self.source, self.student = source, student
        self.module = copy.deepcopy(student).eval()
        self._pairs = list(zip(self.module.parameters(), student.parameters()))
        for t, _ in self._pairs:
            t.requires_grad_(False)
        self._bound = [None] * len(self._pairs)  # the storage each teacher parameter reads
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        avg = self.source.ema_tensors()
        for i, (t, s) in enumerate(self._pairs):
            src = avg[s][0] if s in avg else s.detach()
            if self._bound[i] is None or self._bound[i].data_ptr() != src.data_ptr():
                t.data = src  # (shares the storage; the teacher parameter keeps its own version counter)
                self._bound[i] = src
        for tb, sb in zip(self.module.buffers(), self.student.buffers()):
            tb.copy_(sb)
        _bump_versions([t for t, _ in self._pairs])

    @torch.no_grad()
    def logits(self, images):
        """(B, 3, H, W) -> the teacher's NHWC quarter-resolution logits (Network3._segment_nhwc, inside its guarded scope)"""
        self.module.eval()
        return self.module._segment_nhwc(images)


def cross_mix_table(B, policy):
    """The ClassMix table of a batch of 2B = [labelled half | unlabelled half]: rows 0..B-1 (labelled) have donor == self; receiver
    B + i (unlabelled) takes labelled sample i as its donor with the probability, keys and force that `policy` (a data.ClassMix,
    classes="half") draws for row i from its private generator, whose stream per call is that of policy.draw - the donor it draws
    inside its own batch is not used.  -> (2B, 2 + n_class) int32."""
    if policy.classes != "half":
        raise ValueError(f"cross_mix_table: the cross-set mix pastes half of the donor's classes, the policy has classes={policy.classes!r}")
    if B < 1:
        raise ValueError(f"cross_mix_table: B {B} < 1")
    drawn = policy.draw(max(B, 2))[:B]  # (a policy draws for at least two samples)
    n = policy.n_class
    table = np.empty((2 * B, 2 + n), dtype=np.int32)
    table[:B, 0], table[:B, 1], table[:B, 2:] = np.arange(B), -1, np.arange(n)
    mixes = drawn[:, 0] != np.arange(B)
    table[B:, 0] = np.where(mixes, np.arange(B), np.arange(B, 2 * B))
    table[B:, 1:] = drawn[:, 1:]
    return table


def cross_mix(xL, yL, xU, yU, qU, table, n_class=9, min_pixels=0, tally=None):
    """DAFormer's mix on ops.class_mix: the labelled half (xL (B, 3, h, w), yL (B, h, w) int64) and the unlabelled half (xU, pseudo-
    labels yU, per-sample weight qU (B,) float32) are concatenated; `table` is cross_mix_table's.  The weight rides as the third
    plane - 1.0 for the labelled half, q_b broadcast for the unlabelled one - so the result's weight is 1 where a labelled pixel
    was pasted and q_b elsewhere, copied bit for bit.  -> (xM, yM, uM (B, h, w), pasted (B,) int64): the second half of the result."""
    B = xL.shape[0]
    if xU.shape != xL.shape or yL.shape != yU.shape or qU.shape != (B,):
        raise RuntimeError(f"cross_mix: halves of {tuple(xL.shape)} / {tuple(xU.shape)} images, {tuple(yL.shape)} / {tuple(yU.shape)} labels "
                           f"and {tuple(qU.shape)} weights do not make one batch")
    x = torch.cat([xL, xU])
    y = torch.cat([yL.long(), yU.long()])
    w = torch.cat([torch.ones_like(qU), qU])[:, None, None, None].expand(2 * B, 3, *x.shape[2:]).contiguous()
    _, xm, wm, ym, _, pasted = ops.class_mix(x, x, w, y, table, n_class, min_pixels, tally)
    return xm[B:], ym[B:], wm[B:, 0], pasted[B:]


class SelfTrainingStep:
    """One optimizer step on a labelled batch and an unlabelled batch:
        1. teacher logits of xU                             4. loss = criterion(student(xL), yL)
        2. ops.pseudo_label (tau, below) and q_b                     + unsup_weight * CE_mean_all(student(xM), yM; u)
        3. with mix (a data.ClassMix): cross_mix            5. one optimizer.step()   6. teacher.refresh()
           with strong (a data.StrongAugment): the student's unlabelled input is ops.strong_augment(xM or xU, strong.draw(B)),
           after the mix; labels, pixel weights and sample weights are unchanged and the teacher still sees the clean xU.
           last_strong keeps the drawn table.  With strong=None the launches and the bits are what they are without it.
    The labelled term keeps whatever path `criterion` takes in seg_train_step.  The unlabelled term is cross entropy averaged over
    ALL pixels (SEGMIF_SEG_MEAN_ALL, what DAFormer computes: (loss * weight).mean()) with u = q_b per sample, or the mixed weight
    plane.  Two student forwards and backwards, gradients accumulated (under a reducer: one backward of the sum).  step() returns
    (loss_sup, loss_unsup) detached; the last count of confident pixels stays on the device: confident_share() reads it back, once
    per log line.  teacher_temperature T (utils/calibration.fit_temperature measures one): the teacher's logits are multiplied by
    float32(1 / T) before ops.pseudo_label, so tau tests the softmax at temperature T; the argmax does not change.  Not
    graph-captured."""

    def __init__(self, student, teacher, optimizer, criterion, tau=0.968, below="keep", unsup_weight=1.0, mix=None, reducer=None,
                 ignore_index=255, teacher_temperature=1.0, strong=None):
        if not 0.0 <= float(tau) <= 1.0:
            raise ValueError(f"SelfTrainingStep: tau {tau} outside [0, 1]")
        if below not in ops.PSEUDO_BELOW:
            raise ValueError(f"SelfTrainingStep: below must be one of {', '.join(ops.PSEUDO_BELOW)}, got {below!r}")
        if not float(unsup_weight) > 0.0:
            raise ValueError(f"SelfTrainingStep: unsup_weight {unsup_weight} must be > 0")
        self.student, self.teacher, self.opt, self.crit = student, teacher, optimizer, criterion
        self.tau, self.below, self.unsup_weight, self.mix, self.reducer = float(tau), below, float(unsup_weight), mix, reducer
        self.ignore_index = int(ignore_index)
        self.unsup = losses.SegObjective(reduction="mean_all", ignore_index=self.ignore_index)
        self.strong = strong
        self.teacher_temperature = float(teacher_temperature)
        if not (math.isfinite(self.teacher_temperature) and self.teacher_temperature > 0.0):
            raise ValueError(f"SelfTrainingStep: teacher_temperature {teacher_temperature} must be finite and > 0")
        self.last_count, self.last_pixels, self.last_table, self.last_strong = None, 0, None, None

    def pseudo(self, xU):
        """-> (pseudo-labels (B, H, W) int64, q (B,) float32) of the teacher on xU; keeps the count"""
        H, W = xU.shape[2:]
        logits = self.teacher.logits(xU)
        if self.teacher_temperature != 1.0:  # (at 1.0 no operation is added: the bits are what they were)
            logits = logits * float(np.float32(1.0) / np.float32(self.teacher_temperature))
        labels, count = ops.pseudo_label(logits, H, W, tau=self.tau, below=self.below, ignore_index=self.ignore_index)
        self.last_count, self.last_pixels = count, H * W
        return labels, ops.pseudo_weight(count, H, W)

    def step(self, xL, yL, xU):
        from .train import _zero_grads
        yU, q = self.pseudo(xU)
        pixel_weight, sample_weight, xM, yM = None, q, xU, yU
        if self.mix is not None:
            self.last_table = cross_mix_table(xL.shape[0], self.mix)
            xM, yM, pixel_weight, _ = cross_mix(xL, yL, xU, yU, q, self.last_table, self.mix.n_class, self.mix.min_pixels)
            sample_weight = None
        if self.strong is not None:
            self.last_strong = self.strong.draw(xM.shape[0])
            xM = ops.strong_augment(xM, self.last_strong)
        _zero_grads(self.opt, self.reducer)
        loss_sup = self.student._loss(xL, yL, self.crit)
        if self.reducer is None:  # one graph alive at a time; the gradients accumulate
            loss_sup.backward()
        loss_unsup = self.student._loss(xM, yM, self.unsup, pixel_weight=pixel_weight, sample_weight=sample_weight)
        if self.reducer is None:
            (self.unsup_weight * loss_unsup).backward()
        else:  # (a GradAllReducer launches a bucket at a parameter's first gradient: one backward of the sum)
            (loss_sup + self.unsup_weight * loss_unsup).backward()
            self.reducer.finish()
        self.opt.step()
        self.teacher.refresh()
        return loss_sup.detach(), loss_unsup.detach()

    def confident_share(self):
        """the share of the last unlabelled batch's pixels whose teacher confidence was above tau (one readback)"""
        if self.last_count is None:
            raise RuntimeError("confident_share(): no step yet")
        return float(self.last_count.sum()) / (self.last_count.numel() * self.last_pixels)
