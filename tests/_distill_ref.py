"""A torch restatement, in the dtype of its inputs (float64 in the tests), of the two distillation objectives of
include/segmif_distill.h, written from their definitions: no blocks, no staged maxima, no statistics table.  Inputs are NHWC logits
(B, h, w, C); z = x / T, lse the log-sum-exp over the stated axis.

    pixel    k_i  = sum_c p_ic ((zt_ic - lse_t,i) - (zs_ic - lse_s,i)) over the classes of a pixel;    loss = T^2 sum_i k_i / (B h w)
    channel  k_bc = sum_j p_bcj ((zt - lse_t,bc) - (zs - lse_s,bc)) over the positions of a class map;  loss = T^2 sum k_bc / (B C)

grad() is the stated derivative, not autograd's: (T / n) (softmax(zs) - softmax(zt)), n = B h w or B C."""
import torch


def _axis(kind, x):
    """(B, h, w, C) -> (groups, n) with the softmax axis last"""
    B, h, w, C = x.shape
    if kind == "pixel":
        return x.reshape(B * h * w, C)
    if kind == "channel":
        return x.reshape(B, h * w, C).transpose(1, 2).reshape(B * C, h * w)
    raise ValueError(kind)


def _back(kind, g, shape):
    B, h, w, C = shape
    if kind == "pixel":
        return g.reshape(B, h, w, C)
    return g.reshape(B, C, h * w).transpose(1, 2).reshape(B, h, w, C)


def _logsoftmax(z):
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    return z - lse


def loss(kind, student, teacher, T):
    zs, zt = _axis(kind, student) / T, _axis(kind, teacher) / T
    ls, lt = _logsoftmax(zs), _logsoftmax(zt)
    p = torch.exp(lt)
    k = (p * (lt - ls)).sum(dim=1)
    return T * T * k.sum() / k.numel()


def grad(kind, student, teacher, T):
    zs, zt = _axis(kind, student) / T, _axis(kind, teacher) / T
    q, p = torch.exp(_logsoftmax(zs)), torch.exp(_logsoftmax(zt))
    return _back(kind, (T / zs.shape[0]) * (q - p), student.shape)


def torch_ops(kind, student, teacher, T):
    """the same objective composed from torch operators the way a user would, in the inputs' dtype and on their device: softmax,
    log-softmax, multiply and sum (the float32 baseline of the GPU tests' gates and of tools/distill_bench.py)"""
    zs, zt = _axis(kind, student) / T, _axis(kind, teacher) / T
    ls, lt = torch.log_softmax(zs, dim=1), torch.log_softmax(zt, dim=1)
    k = (torch.softmax(zt, dim=1) * (lt - ls)).sum()
    return T * T * k / zs.shape[0]
