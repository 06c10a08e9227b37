"""The oracle of the boundary (signed-distance) criteria: scipy's exact Euclidean distance transform in fp64 per volume for the map,
fp64 torch autograd on that map for the loss and its gradient.  Used by the host tests (against a brute-force distance) and by the
GPU tests."""
import numpy as np
import torch

EPS = 1e-7


def signed_distance_volume(mask):
    """phi of ONE boolean volume, fp64: outside the mask the distance to its nearest voxel, inside -(distance to the nearest voxel
    outside - 1), zero everywhere for an empty or a full mask (one_hot2dist of Kervadec et al.'s code)"""
    from scipy.ndimage import distance_transform_edt as edt
    mask = np.asarray(mask, dtype=bool)
    if not mask.any() or mask.all():
        return np.zeros(mask.shape, dtype=np.float64)
    neg = ~mask
    return edt(neg) * neg - (edt(mask) - 1) * mask


def signed_distance_batch(targets):
    """(B, C, D, H, W) fp32 tensor of the maps of ``targets > 0.5``: fp64 per volume, cast once to fp32"""
    t = targets.detach().cpu().numpy()
    out = np.zeros(t.shape, dtype=np.float32)
    for b in range(t.shape[0]):
        for c in range(t.shape[1]):
            out[b, c] = signed_distance_volume(t[b, c] > 0.5).astype(np.float32)
    return torch.from_numpy(out)


def brute_force_volume(mask):
    """the same map by the O(n^2) definition: every voxel against every voxel of the other class"""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(mask.shape, dtype=np.float64)
    if not mask.any() or mask.all():
        return out
    idx = np.argwhere(np.ones(mask.shape, dtype=bool)).astype(np.float64)
    flat = mask.reshape(-1)
    inside, outside = idx[flat], idx[~flat]
    res = out.reshape(-1)
    for k, p in enumerate(idx):
        if flat[k]:
            res[k] = -(np.sqrt(((outside - p) ** 2).sum(1).min()) - 1.0)
        else:
            res[k] = np.sqrt(((inside - p) ** 2).sum(1).min())
    return out


def loss_oracle(o, t, phi, w_dice, w_boundary, scale, upstream=1.0, eps=EPS):
    """fp64 on the CPU from fp32 (o, t, phi): per-channel sums (C, 4) = (sum o t, sum o o, sum t t, sum o phi), the magnitude
    sum |o phi| per channel (C), loss, coefficients (C, 3) = (ca, cb, cd) and the gradient of upstream * loss.
    loss = [w_dice: 1 - sum_c wd_c (2 I_c + eps) / (O_c + T_c + eps)] + sum_c wb_c * scale * P_c / count"""
    o64, t64, p64 = o.detach().cpu().double().requires_grad_(True), t.detach().cpu().double(), phi.detach().cpu().double()
    C = o.shape[1]
    dims = [d for d in range(o.dim()) if d != 1]
    I, O_, T, P = (o64 * t64).sum(dims), (o64 * o64).sum(dims), (t64 * t64).sum(dims), (o64 * p64).sum(dims)
    mag = (o64 * p64).abs().sum(dims).detach()
    count = o.numel() // C
    loss = torch.zeros((), dtype=torch.float64)
    coef = torch.zeros(C, 3, dtype=torch.float64)
    if w_dice is not None:
        wd = torch.tensor(w_dice, dtype=torch.float64)
        num, den = 2 * I + eps, O_ + T + eps
        loss = loss + 1 - (wd * num / den).sum()
        coef[:, 0], coef[:, 1] = (-2 * wd / den).detach(), (2 * wd * num / den ** 2).detach()
    wb = torch.tensor(w_boundary, dtype=torch.float64) * float(scale)
    loss = loss + (wb * P / count).sum()
    coef[:, 2] = wb / count
    grad, = torch.autograd.grad(loss * upstream, o64)
    return torch.stack([I, O_, T, P], 1).detach(), mag, float(loss.detach()), coef, grad


def boundary_slack(mag, w_boundary, scale, count):
    """the absolute error the boundary term of a loss may carry: 1e-5 * sum_c |wb_c scale| * sum |o phi|_c / count (the moment can
    cancel to near zero, so its error is bounded against the magnitude of what was added up)"""
    wb = torch.tensor(w_boundary, dtype=torch.float64).abs() * abs(float(scale))
    return 1e-5 * float((wb * mag).sum()) / count
