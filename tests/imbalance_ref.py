"""The fp64 torch oracle of the class-imbalance criteria (``sp_tloss_*``: Tversky, focal Tversky, focal cross entropy and their sums),
written literally from the formulas of ``include/stroke_amd.h``, with ``clamp_min`` where the kernels clamp.

The Tversky gradient is autograd's.  The focal gradient is the analytic ``fl'``: autograd is infinite at a saturated output (o = 0 or
1), where ``torch.nn.BCELoss`` -- and the kernels -- are finite by construction."""
import torch

EPS = 1e-7


def focal_term(o, t, gamma, alpha):
    """fl(o, t) = -alpha t (1 - o)^gamma lo - (1 - alpha) (1 - t) o^gamma l1, the logarithms clamped at -100"""
    lo, l1 = torch.log(o).clamp_min(-100.0), torch.log(1 - o).clamp_min(-100.0)
    return -alpha * t * (1 - o) ** gamma * lo - (1 - alpha) * (1 - t) * o ** gamma * l1


def focal_grad(o, t, gamma, alpha):
    """d fl / d o with the divisions clamped at 1e-12; the gamma x^(gamma - 1) terms are absent at gamma = 0"""
    lo, l1 = torch.log(o).clamp_min(-100.0), torch.log(1 - o).clamp_min(-100.0)
    a = -(1 - o) ** gamma / o.clamp_min(1e-12)
    b = o ** gamma / (1 - o).clamp_min(1e-12)
    if gamma != 0:
        a = a + gamma * (1 - o) ** (gamma - 1) * lo
        b = b - gamma * o ** (gamma - 1) * l1
    return alpha * t * a + (1 - alpha) * (1 - t) * b


def tversky_loss(o, t, w, fp, fn, gamma, eps=EPS):
    """sum_c w_c max(1 - (TP + eps) / (TP + fp (So - TP) + fn (St - TP) + eps), 1e-12)^(1 / gamma), sums over batch and volume"""
    dims = [d for d in range(o.dim()) if d != 1]
    tp, so, st = (o * t).sum(dims), o.sum(dims), t.sum(dims)
    base = 1 - (tp + eps) / (tp + fp * (so - tp) + fn * (st - tp) + eps)
    return (torch.as_tensor(w, dtype=torch.float64) * base.clamp_min(1e-12) ** (1.0 / gamma)).sum()


def oracle(o, t, w_tversky, w_focal, fp=0.3, fn=0.7, tversky_gamma=1.0, focal_gamma=2.0, focal_alpha=0.25, upstream=1.0, eps=EPS):
    """fp64 on the CPU of fp32 (B, C, ...) inputs: per-channel sums (C, 4) = (sum o t, sum o, sum t, sum fl), the loss, the
    coefficients (C, 3) = (ca, c0, c3) and the gradient of upstream * loss.  Either weight list may be None = the term is absent."""
    o64, t64 = o.double().requires_grad_(True), t.double()
    C = o.shape[1]
    dims = [d for d in range(o.dim()) if d != 1]
    count = o.numel() // C
    view = [1, C] + [1] * (o.dim() - 2)
    fl = focal_term(o64.detach(), t64, focal_gamma, focal_alpha)
    sums = torch.stack([(o64 * t64).sum(dims), o64.sum(dims), t64.sum(dims), fl.sum(dims)], 1).detach()
    loss = torch.zeros((), dtype=torch.float64)
    grad = torch.zeros_like(t64)
    coef = torch.zeros(C, 3, dtype=torch.float64)
    if w_tversky is not None:
        w = torch.tensor(w_tversky, dtype=torch.float64)
        term = tversky_loss(o64, t64, w, fp, fn, tversky_gamma, eps)
        grad = grad + torch.autograd.grad(term, o64)[0]
        loss = loss + term.detach()
        tp, so, st = sums[:, 0], sums[:, 1], sums[:, 2]
        n, d = tp + eps, tp + fp * (so - tp) + fn * (st - tp) + eps
        base = 1 - n / d
        k = torch.where(base >= 1e-12, -(w / tversky_gamma) * base.clamp_min(1e-300) ** (1.0 / tversky_gamma - 1.0), torch.zeros_like(base))
        coef[:, 0] = k * (1 / d - n * (1 - fp - fn) / d ** 2)
        coef[:, 1] = -k * n * fp / d ** 2
    if w_focal is not None:
        w4 = torch.tensor(w_focal, dtype=torch.float64)
        loss = loss + (w4 * sums[:, 3] / count).sum()
        coef[:, 2] = w4 / count
        grad = grad + coef[:, 2].view(view) * focal_grad(o64.detach(), t64, focal_gamma, focal_alpha)
    return sums, float(loss), coef, grad * upstream
