"""Float64 restatement of the self-training pieces, written from the rules of include/segmif_hip.h and not from the kernels:
segmif_pseudo_label_f32 (bilinear resize with align_corners = False, argmax, softmax maximum, threshold, count) and the weighted
segmentation objective (segmif_seg_objective_weighted_f32: u_i l_i over a denominator WITHOUT u).  The per-pixel loss l_i is
tests/_seg_objective_ref.py's, imported and left as it is.  Shared by tests/test_self_training_host.py and the GPU tests; it
launches nothing."""
import numpy as np
import torch

import _seg_objective_ref as seg_ref


def _axis(n_in, n_out):
    """source coordinate max(0, s (dst + 0.5) - 0.5), s = in / out -> (i0, i1, l, h) of every output index"""
    f = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.floor(f).astype(np.int64)
    i0 = np.minimum(i0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l = f - i0
    return i0, i1, l, 1.0 - l


def resize(x, OH, OW):
    """x (B, h, w, C) -> float64 (B, OH, OW, C): hy (hx p00 + lx p01) + ly (hx p10 + lx p11)"""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly, hy = _axis(x.shape[1], OH)
    x0, x1, lx, hx = _axis(x.shape[2], OW)
    lx, hx = lx[None, None, :, None], hx[None, None, :, None]
    ly, hy = ly[None, :, None, None], hy[None, :, None, None]
    top = hx * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = hx * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    return hy * top + ly * bot


def pseudo_label(x, OH, OW, tau, below="keep", ignore_index=255):
    """-> dict(label (B, OH, OW) int64, argmax, p_max float64, gap = float64 top-2 gap of the resized logits (inf for C = 1),
    confident bool, count (B,) int64).  Ties go to the lowest index (numpy's argmax); a NaN p_max is not confident."""
    v = resize(x, OH, OW)
    arg = np.argmax(v, axis=-1).astype(np.int64)  # (a NaN wins numpy's argmax: NaN inputs are checked on their own in the tests)
    vmax = np.max(v, axis=-1)
    with np.errstate(invalid="ignore"):
        p_max = 1.0 / np.exp(v - vmax[..., None]).sum(-1)
        confident = p_max > tau
    if v.shape[-1] > 1:
        s = np.sort(v, axis=-1)
        gap = s[..., -1] - s[..., -2]
    else:
        gap = np.full(arg.shape, np.inf)
    label = arg if below == "keep" else np.where(confident, arg, ignore_index)
    return dict(label=label, argmax=arg, p_max=p_max, gap=gap, confident=confident, count=confident.reshape(len(v), -1).sum(1).astype(np.int64))


def row_weights(rows, pixel_weight=None, sample_weight=None):
    """u_i = pixel_weight[i] * sample_weight[i / rows_per_sample] as float64 (rows,); a missing weight is 1"""
    u = torch.ones(rows, dtype=torch.float64)
    if pixel_weight is not None:
        u = u * pixel_weight.detach().double().reshape(-1).cpu()
    if sample_weight is not None:
        sw = sample_weight.detach().double().reshape(-1).cpu()
        assert rows % sw.numel() == 0
        u = u * sw.repeat_interleave(rows // sw.numel())
    return u


def weighted_objective(logits, labels, pixel_weight=None, sample_weight=None, gamma=0.0, eps=0.0, weight=None, ignore_index=255,
                       reduction="mean"):
    """logits (..., C) classes last, labels (...): sum_i u_i l_i / (sum_valid w_y for "mean", rows for "mean_all")"""
    C = logits.shape[-1]
    l, w_y, _ = seg_ref.pixel_losses(logits.reshape(-1, C), labels.reshape(-1), gamma, eps, weight, ignore_index)
    u = row_weights(l.numel(), pixel_weight, sample_weight).to(l.dtype)
    if reduction == "mean":
        return (u * l).sum() / w_y.sum()
    if reduction == "mean_all":
        return (u * l).sum() / l.numel()
    raise ValueError(f"the weighted objective has the reductions mean and mean_all, not {reduction!r}")


def weighted_value_and_grad(logits, labels, **kw):
    """float64 value and gradient w.r.t. the logits (classes last)"""
    x = logits.detach().double().cpu().clone().requires_grad_(True)
    if kw.get("weight") is not None:
        kw = dict(kw, weight=kw["weight"].double().cpu())
    v = weighted_objective(x, labels.cpu(), **kw)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g
