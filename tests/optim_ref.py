"""A restatement of the four update rules of csrc/sp_optim.hip (ADAM, ADAMW, SGD, SGD_NESTEROV) with the global-norm clip
coefficient, on torch CPU tensors of any floating type.  tests/test_optim_host.py pins it to ``torch.optim.Adam`` / ``AdamW`` /
``SGD`` + ``clip_grad_norm_`` in float64; the GPU tests use its float64 run as their oracle."""
import math

import torch

KINDS = ("adam", "adamw", "sgd", "nesterov")


def grad_norm(grads, grad_scale=1.0):
    """grad_scale * sqrt(sum over every tensor of g^2), accumulated in float64"""
    return float(grad_scale) * math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def clip_coef(norm, max_grad_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); 1 where clipping is off (None or <= 0)"""
    if max_grad_norm is None or max_grad_norm <= 0:
        return 1.0
    return min(1.0, max_grad_norm / (norm + 1e-6))


class RefOptimizer:
    """``step(grads)`` updates ``params`` (a list of tensors, changed in place) by the rule of ``kind``; ``hyper`` may be edited
    between steps.  State: ``m`` (exp_avg or the momentum buffer) and ``v`` (exp_avg_sq) per tensor, ``steps``, ``last_norm``."""

    def __init__(self, kind, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0, grad_scale=1.0,
                 max_grad_norm=None):
        assert kind in KINDS
        self.kind, self.params, self.grad_scale = kind, params, grad_scale
        self.hyper = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum=momentum, max_grad_norm=max_grad_norm)
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.steps = 0
        self.last_norm = None

    def step(self, grads):
        h = self.hyper
        lr, wd, (b1, b2), eps, mom = h["lr"], h["weight_decay"], h["betas"], h["eps"], h["momentum"]
        self.last_norm = grad_norm(grads, self.grad_scale)
        coef = clip_coef(self.last_norm, h["max_grad_norm"])
        self.steps += 1
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            gi = g.to(p.dtype) * self.grad_scale * coef
            if self.kind in ("adam", "adamw"):
                if self.kind == "adam":
                    gi = gi + wd * p
                else:
                    p.mul_(1 - lr * wd)
                m.mul_(b1).add_(gi, alpha=1 - b1)
                v.mul_(b2).add_(gi * gi, alpha=1 - b2)
                bc1, bc2 = 1 - b1 ** self.steps, 1 - b2 ** self.steps
                p.sub_(lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps))
            else:
                gi = gi + wd * p
                m.mul_(mom).add_(gi)
                p.sub_(lr * (gi + mom * m if self.kind == "nesterov" else m))
