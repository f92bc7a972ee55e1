"""A torch restatement, in float64, of the two region objectives csrc/region_objective.hip computes, written from their definitions
(include/segmif_hip.h): Lovasz-Softmax over the batch as one set and soft Dice.  Rows are the pixels (N, C); a row is valid when its
label lies in [0, C) and is not ignore_index.  The Lovasz sort is a stable descending one: ties by ascending row index.  The
gradient is autograd's (g, built from integers, is a constant of the graph).  Shared by tests/test_region_objectives_host.py and
tests/test_gpu_region_objectives.py; it launches nothing.

`order` lets a caller re-evaluate the Lovasz objective under another permutation of the rows than the one its own float64 errors
give: order(e, c) -> the descending permutation for class c, given the class's float64 errors.  The GPU tests use it to keep only
inputs whose gradient does not depend on how float32 rounding orders nearly equal errors (order_sensitivity)."""
import torch


def valid_rows(logits, labels, ignore_index=255):
    return (labels != ignore_index) & (labels >= 0) & (labels < logits.shape[1])


def class_errors(logits, labels):
    """valid rows only: (e (P, C) with e_ic = |fg_ic - p_ic|, fg (P, C) bool); the labelled class's 1 - p_y is formed as
    sum_{k != y} exp / sum exp, without the cancellation"""
    ex = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
    fg = torch.zeros_like(ex, dtype=torch.bool)
    fg[torch.arange(len(labels)), labels] = True
    total = ex.sum(1, keepdim=True)
    p = ex / total
    q = torch.where(fg, torch.zeros_like(ex), ex).sum(1, keepdim=True) / total
    return torch.where(fg, q.expand_as(p), p), fg


def stable_descending(e, c=None):
    return torch.sort(e, descending=True, stable=True).indices


def jaccard_increments(fg_sorted):
    """g_k = J_k - J_{k-1}, J_k = 1 - (G - F_k) / (G + k - F_k), J_0 = 0, from the sorted foreground flags"""
    G = fg_sorted.sum().double()
    F = torch.cumsum(fg_sorted.double(), 0)
    k = torch.arange(1, len(fg_sorted) + 1, dtype=torch.float64)
    J = 1.0 - (G - F) / (G + k - F)
    return J - torch.cat([J.new_zeros(1), J[:-1]])


def lovasz(logits, labels, classes="present", ignore_index=255, order=stable_descending):
    """logits (N, C), labels (N,) -> the scalar"""
    v = valid_rows(logits, labels, ignore_index)
    x, y = logits[v], labels[v]
    if len(y) == 0:
        return logits.sum() * 0.0
    e, fg = class_errors(x, y)
    terms = []
    for c in range(x.shape[1]):
        if classes == "present" and not bool(fg[:, c].any()):
            continue
        perm = order(e[:, c].detach(), c)
        terms.append((e[perm, c] * jaccard_increments(fg[perm, c])).sum())
    return torch.stack(terms).mean() if terms else logits.sum() * 0.0


def dice(logits, labels, classes="present", ignore_index=255, smooth=1.0):
    v = valid_rows(logits, labels, ignore_index)
    x, y = logits[v], labels[v]
    if len(y) == 0:
        return logits.sum() * 0.0
    p = torch.softmax(x, dim=1)
    fg = torch.nn.functional.one_hot(y, x.shape[1]).to(p.dtype)
    I, S, G = (p * fg).sum(0), p.sum(0), fg.sum(0)
    D = 1.0 - (2.0 * I + smooth) / (S + G + smooth)
    keep = G > 0 if classes == "present" else torch.ones_like(G, dtype=torch.bool)
    return D[keep].mean() if bool(keep.any()) else logits.sum() * 0.0


def objective(logits, labels, kind="lovasz", **kw):
    """logits (..., C) with the classes LAST, labels (...)"""
    C = logits.shape[-1]
    return (lovasz if kind == "lovasz" else dice)(logits.reshape(-1, C), labels.reshape(-1), **kw)


def value_and_grad(logits, labels, kind="lovasz", **kw):
    """float64 value and gradient w.r.t. the logits (classes last), evaluated at the values the input holds (float32 in the tests)"""
    x = logits.detach().double().clone().requires_grad_(True)
    v = objective(x, labels, kind, **kw)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


# ---- the orders a float32 evaluation may legitimately take ---------------------------------------------------------------------------
def _ties_descending(e, c=None):
    """stable descending sort with ties by DESCENDING row index"""
    n = len(e)
    return (n - 1) - torch.sort(e.flip(0), descending=True, stable=True).indices


def _moved(e, ulps_even, ulps_odd):
    """the float32 image of e with its bit pattern moved by the given ulps on even / odd rows (clamped at 0)"""
    bits = e.float().view(torch.int32)
    step = torch.where(torch.arange(len(e)) % 2 == 0, ulps_even, ulps_odd).to(torch.int32)
    return (bits + step).clamp_(min=0).view(torch.float32)


def alternative_orders(tie_directions=True):
    orders = {"float32": lambda e, c: stable_descending(e.float()),
              "+2/-2 ulp": lambda e, c: stable_descending(_moved(e, 2, -2)),
              "-2/+2 ulp": lambda e, c: stable_descending(_moved(e, -2, 2))}
    if tie_directions:
        orders["ties descending"] = _ties_descending
        orders["float32, ties descending"] = lambda e, c: _ties_descending(e.float())
    return orders


def order_sensitivity(logits, labels, classes="present", ignore_index=255, tie_directions=True):
    """The largest change of a float64 Lovasz gradient element, as a fraction of the gradient's largest magnitude, when the rows
    are ordered by their float32-rounded errors, with either tie direction, or with the errors moved by +-2 float32 ulps in
    alternating row parity.  Inputs for which this is far below the gradient gate can be compared element by element."""
    _, g0 = value_and_grad(logits, labels, "lovasz", classes=classes, ignore_index=ignore_index)
    worst = 0.0
    for order in alternative_orders(tie_directions).values():
        _, g = value_and_grad(logits, labels, "lovasz", classes=classes, ignore_index=ignore_index, order=order)
        worst = max(worst, float((g - g0).abs().max() / g0.abs().max()))
    return worst


def make_inputs(seed, shape, C, rare=5, ignore_frac=0.10, dominant=0.6, scale=1.0, boost=2.0, ignore_index=255):
    """NHWC logits (B, H, W, C) float32 and labels (B, H, W) imbalanced like MFNet's: class 0 takes `dominant` of the pixels, class
    C - 1 exactly `rare` of them, the others share the rest; about ignore_frac are ignore_index; on half the rows the labelled
    logit is raised by `boost`, so that the prediction is correlated with the label"""
    B, H, W = shape
    n = B * H * W
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g, dtype=torch.float32) * scale
    mid = max(C - 2, 1)
    y = torch.where(torch.rand(n, generator=g) < dominant, torch.zeros(n, dtype=torch.int64),
                    1 + torch.randint(0, mid, (n,), generator=g)).clamp_(max=C - 1)
    if C > 2:
        y[torch.randperm(n, generator=g)[:rare]] = C - 1
    ign = torch.rand(n, generator=g) < ignore_frac
    hit = (torch.rand(n, generator=g) < 0.5).nonzero()[:, 0]
    x[hit, y[hit]] += boost
    y[ign] = ignore_index
    return x.view(B, H, W, C), y.view(B, H, W)
