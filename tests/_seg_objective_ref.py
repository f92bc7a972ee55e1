"""A torch restatement, in the dtype of its input (float64 in the tests), of what csrc/seg_objective.hip computes: the per-pixel
losses and the three reductions.  OHEM is written with torch.sort and its host branch, as the reference's OhemCELoss has it.
Shared by tests/test_seg_objectives_host.py and tests/test_gpu_seg_objectives.py; it launches nothing."""
import torch
import torch.nn.functional as F


def ohem_t(thresh):
    """-log(thresh) in float32, as OhemCELoss.__init__ forms it"""
    return float(-torch.log(torch.tensor(float(thresh), dtype=torch.float)))


def pixel_losses(logits, labels, gamma=0.0, eps=0.0, weight=None, ignore_index=255):
    """logits (N, C) rows, labels (N,) -> (l (N,), w_y (N,), valid (N,)); ignored pixels have l = 0 and w_y = 0"""
    N, C = logits.shape
    valid = (labels != ignore_index) & (labels >= 0) & (labels < C)
    y = torch.where(valid, labels, torch.zeros_like(labels))
    w = torch.ones(C, dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    logp = F.log_softmax(logits, dim=1)
    logp_y = logp.gather(1, y[:, None])[:, 0]
    w_y = w[y]
    if gamma > 0:
        e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        q = (e.sum(1) - e.gather(1, y[:, None])[:, 0]) / e.sum(1)  # 1 - p_y without the cancellation
        l = -w_y * q ** gamma * logp_y
    else:
        l = (1 - eps) * (-w_y * logp_y) + (eps / C) * (-(w[None, :] * logp).sum(1))
    zero = torch.zeros_like(l)
    return torch.where(valid, l, zero), torch.where(valid, w_y, zero), valid


def reduce_losses(l, w_y, reduction="mean", t=None, n_min=None):
    if reduction == "mean":
        return l.sum() / w_y.sum()
    if reduction == "mean_all":
        return l.mean()
    if reduction != "ohem":
        raise ValueError(reduction)
    s, _ = torch.sort(l, descending=True)
    if s[n_min - 1] > t:
        return s[s > t].mean()
    return s[:n_min].mean()


def objective(logits, labels, gamma=0.0, eps=0.0, weight=None, ignore_index=255, reduction="mean", thresh=None, n_min=None):
    """logits (..., C) with the classes LAST, labels (...): the scalar a SegObjective of these settings computes"""
    C = logits.shape[-1]
    l, w_y, _ = pixel_losses(logits.reshape(-1, C), labels.reshape(-1), gamma, eps, weight, ignore_index)
    return reduce_losses(l, w_y, reduction, None if thresh is None else ohem_t(thresh), n_min)


def value_and_grad(logits, labels, **kw):
    """float64 value and gradient w.r.t. the logits (classes last), whatever the input's dtype"""
    x = logits.detach().double().clone().requires_grad_(True)
    if kw.get("weight") is not None:
        kw = dict(kw, weight=kw["weight"].double())
    v = objective(x, labels, **kw)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def selection_margin(logits, labels, thresh=None, n_min=None, **kw):
    """The float64 gaps that decide OHEM's selection: (smallest |l - t| over all pixels, gap between the n_min-th and the
    (n_min + 1)-th sorted losses; inf where it does not apply).  A float32 evaluation selects the same pixels as a float64 one
    only if its rounding stays below them."""
    C = logits.shape[-1]
    l, _, _ = pixel_losses(logits.double().reshape(-1, C), labels.reshape(-1), **kw)
    at_t = float((l - ohem_t(thresh)).abs().min()) if thresh is not None else float("inf")
    at_k = float("inf")
    if n_min is not None and n_min < l.numel():
        s, _ = torch.sort(l, descending=True)
        at_k = float(s[n_min - 1] - s[n_min])
    return at_t, at_k


def make_inputs(seed, shape, C, ignore_frac=0.15, scale=2.0, ignore_index=255):
    """the recipe of tools/make_golden_seg_objectives.py: logits (B, C, H, W) = randn * scale, labels uniform in [0, C) with
    about ignore_frac of them set to ignore_index"""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g, dtype=torch.float32) * scale
    labels = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64)
    labels[torch.rand(B, H, W, generator=g) < ignore_frac] = ignore_index
    return logits, labels
