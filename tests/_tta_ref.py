"""Restatement of multi-scale + flip inference in torch operators (float64 by default): the yardstick of test_gpu_tta.py.
The reference project evaluates a single view (test_segmentation.py:169-174), so there is nothing of its to compare with:
    F.interpolate(bilinear, align_corners=False) -> softmax(1) -> flip(3) -> mean over the views -> argmax.
Every function computes in the dtype of what it is given (the tests also run it in float32 to measure the error class)."""
import torch
import torch.nn.functional as F


def vote(views_nhwc, flips, OH, OW):
    """views_nhwc: list of (B, ih, iw, C) logits; flips: one flag per view -> mean probabilities (B, OH, OW, C), summed in
    list order."""
    total = None
    for x, f in zip(views_nhwc, flips):
        p = F.interpolate(x.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=False).softmax(1)
        if f:
            p = p.flip(3)
        total = p if total is None else total + p
    return (total / len(views_nhwc)).permute(0, 2, 3, 1)


def top2_margin(probs):
    """(B, H, W, C) -> (B, H, W): the winner's lead over the runner-up."""
    top = probs.topk(2, dim=3).values
    return top[..., 0] - top[..., 1]


def resize_flip(x_nchw, h, w, flip):
    y = F.interpolate(x_nchw, size=(h, w), mode="bilinear", align_corners=False)
    return y.flip(3) if flip else y


def stand_in_segment(weight):
    """A cheap 'network' for the composition test: quarter-resolution logits einsum(avg_pool2d(x, 4) - 0.5, W) as NHWC; weight
    (classes, 3)."""
    def segment(x_nchw):
        return torch.einsum("bkhw,ck->bhwc", F.avg_pool2d(x_nchw, 4) - 0.5, weight.to(x_nchw.dtype).to(x_nchw.device)).contiguous()
    return segment


def chain(fused_nchw, plan, segment, OH, OW):
    """predict_labels_tta restated: every view's input resized (and mirrored) from `fused`, segmented, voted -> mean
    probabilities (B, OH, OW, C)."""
    views = [segment(resize_flip(fused_nchw, h, w, f)) for h, w, f in plan]
    return vote(views, [f for _, _, f in plan], OH, OW)
