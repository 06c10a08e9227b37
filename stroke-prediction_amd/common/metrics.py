"""Loss and evaluation measures (reference ``common/metrics.py``).

``BatchDiceLoss`` (metrics.py:8-28) keeps its constructor and call signature; on GPU tensors the three
whole-batch reductions and the backward run as two fused HIP kernels (``sp_dice_sums``, ``sp_dice_bwd``)
instead of six torch reductions plus temporaries.  The binary measures (metrics.py:31-62: Dice, precision,
sensitivity, specificity, Hausdorff distance and ASSD as ``medpy.metric.binary`` 0.3.0 defines them) run on the device:
``sp_confusion_counts`` and ``sp_surface_distances`` (border extraction + exact Euclidean distance transform), or -- T results
against one target, the points of a time-to-treatment curve -- ``sp_binary_measures_many`` in one enqueue.  There is
no host implementation here; the checker is ``oracle/measures.py``.

``BCELoss`` and ``DiceBCELoss`` -- the ``# nn.BCELoss()`` the reference's training scripts name beside their Dice criterion -- run on
``sp_vloss_sums`` / ``_finalize_clear`` / ``_bwd``, take the same fused routes as ``BatchDiceLoss`` (``mean_of_channel_losses``,
``cae_reconstruction_loss``) and are picked by name with ``make_criterion``.

``BoundaryLoss`` and ``DiceBoundaryLoss`` -- the boundary loss of Kervadec et al. (MIDL 2019), mean(o * phi(t)) with phi the signed
Euclidean distance map of the label, alone or added to Dice with a weight that can grow over the epochs -- compute phi per sample
and channel on the device (``sp_signed_distance_batch``) and run on ``sp_bloss_sums`` / ``_finalize_clear`` / ``_bwd``; they take the
``mean_of_channel_losses`` route, and the CAE learners compose them literally.

``TverskyLoss`` (Salehi et al., MLMI 2017; with ``gamma = 4/3`` the focal Tversky loss of Abraham & Khan, ISBI 2019), ``FocalBCELoss``
(the focal cross entropy of Lin et al., ICCV 2017) and ``TverskyFocalBCELoss``, their sum -- the criteria for lesions that fill a
fraction of a percent of a patch: false negatives weighed against false positives, easy background voxels down-weighted -- run on
``sp_tloss_sums`` / ``_finalize_clear`` / ``_bwd``; they take the ``mean_of_channel_losses`` route, and the CAE learners compose them
literally.

All eight criteria are ONE autograd function, ``_CriterionFn``, driven by a record per kernel family (``_FAMILIES``: ``sp_dice_*``,
``sp_vloss_*``, ``sp_bloss_*``, ``sp_tloss_*``), with one registry of accumulators, ``_CRIT_SUMS``.
"""
import collections

import numpy
import torch
from torch.nn.modules.loss import _Loss as LossModule

from common.dto.MetricMeasuresDto import BinaryMeasuresDto


_W_CACHE = {}


def _weights_on(device, weights):
    key = (str(device), weights)
    if key not in _W_CACHE:
        _W_CACHE[key] = torch.tensor(weights, dtype=torch.float32, device=device)
    return _W_CACHE[key]


def _batch_strided(x):
    """(tensor, batch stride in elements) for a (B, C, ...) fp32 tensor that is contiguous within each sample --
    channel-slice views such as ``dto.outputs.core`` qualify and are read in place; anything else is copied."""
    x = x if x.dtype == torch.float32 else x.float()
    inner = 1
    ok = True
    for size, stride in zip(reversed(x.shape[1:]), reversed(x.stride()[1:])):
        if size != 1 and stride != inner:
            ok = False
            break
        inner *= size
    if not ok or (x.shape[0] > 1 and x.stride(0) < inner):
        x = x.contiguous()
        return x, inner
    return x, (x.stride(0) if x.shape[0] > 1 else inner)


class _GlobalMeanFn(torch.autograd.Function):
    """mean over the GLOBAL batch in the exact data-parallel mode: local sum, all-reduce, / (elements x world); the backward
    hands every local element 1 / (elements x world) of the upstream gradient -- the local backward then yields this rank's
    share of the gradient of the global mean, and the SUM of the flat gradient buffers is the whole-batch gradient."""

    @staticmethod
    def forward(ctx, t, world):
        from stroke_prediction_amd.runtime.layers import _allreduce
        s = t.sum(dtype=torch.float64).reshape(1)
        _allreduce(s)
        ctx.n, ctx.shape = t.numel() * world, t.shape
        return (s[0] / ctx.n).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return (g / ctx.n).expand(ctx.shape), None


def batch_mean(t):
    """``torch.mean`` of a per-sample tensor as the reference's single process sees it (the loss recipes of
    CaeReconstructionLearner.py:58-67 average over the whole batch): the global mean when the exact data-parallel mode is on
    (parallel.DataParallelSync(mode="exact")), the plain mean otherwise."""
    from stroke_prediction_amd.runtime.layers import SYNC
    if SYNC["on"] and SYNC["world"] > 1:
        return _GlobalMeanFn.apply(t, SYNC["world"])
    return torch.mean(t)


_Family = collections.namedtuple("_Family", "sums finalize bwd pitch ncoef select fourth phi sums_scalars finalize_scalars bwd_scalars",
                                 defaults=(lambda extra: (),) * 3)
# The kernel families of the per-channel criteria, one record each: the three entry points; the accumulator's row pitch (doubles) for C
# channels; the coefficients per channel; ``select``: the integer the sums call takes behind DHW; ``fourth``: there is a fourth moment --
# finalize takes a second weight vector and the element count; ``phi``: the signed-distance map of the targets is a third operand of
# sums and backward, and finalize takes the device scalar that scales the fourth moment's weights; ``*_scalars``: the host scalars a
# call takes out of the criterion's ``extra`` tuple -- sums behind ``select``, finalize in front of eps, backward behind upstream.
_FAMILIES = {
    "dice": _Family("sp_dice_sums", "sp_dice_finalize_clear", "sp_dice_bwd", lambda L, C: (3 * C + 15) // 16 * 16, 2,
                    lambda L, w_dice, w4: (), False, False),
    "vloss": _Family("sp_vloss_sums", "sp_vloss_finalize_clear", "sp_vloss_bwd", lambda L, C: L.SP_VLOSS_PITCH(C), 3,
                     lambda L, w_dice, w4: ((L.SP_VLOSS_DICE if w_dice is not None else 0) | (L.SP_VLOSS_BCE if w4 is not None else 0),),
                     True, False),
    "bloss": _Family("sp_bloss_sums", "sp_bloss_finalize_clear", "sp_bloss_bwd", lambda L, C: L.SP_BLOSS_PITCH(C), 3,
                     lambda L, w_dice, w4: (0 if w_dice is None else 1,), True, True),
    # extra = (fp_weight, fn_weight, tversky_gamma, focal_gamma, focal_alpha); w_dice: the Tversky weights, w4: the focal ones
    "tloss": _Family("sp_tloss_sums", "sp_tloss_finalize_clear", "sp_tloss_bwd", lambda L, C: L.SP_TLOSS_PITCH(C), 3,
                     lambda L, w_dice, w4: ((L.SP_TLOSS_TVERSKY if w_dice is not None else 0) | (L.SP_TLOSS_FOCAL if w4 is not None else 0),),
                     True, False, lambda extra: extra[3:5], lambda extra: extra[0:3], lambda extra: extra[3:5]),
}
_CRIT_SUMS = {}      # (family, device, C, stream) -> [replica rows of that family's sums (zero between calls), busy]


class _CriterionFn(torch.autograd.Function):
    """loss = [1 - sum_c wd_c (2 I_c + eps) / (O_c + T_c + eps)] + [sum_c w4_c * scale * mean_c X], either bracket absent when its
    weights are None; sums and means over batch and volume per channel.  ``family`` names the kernels: "dice" (the first bracket only),
    "vloss" (X = bce(o, t) with torch.nn.BCELoss semantics) or "bloss" (X = o * phi, phi = signed_distance_batch(targets), scale a
    one-float device tensor read by the finalize kernel: a captured step follows its schedule).  Family "tloss" has other brackets:
    [sum_c wd_c max(1 - TI_c, 1e-12)^(1/tversky_gamma)] + [sum_c w4_c mean_c fl(o, t)], TI the Tversky index on first moments and fl the
    focal cross entropy, their scalars in ``extra`` = (fp_weight, fn_weight, tversky_gamma, focal_gamma, focal_alpha).  Two HIP launches forward (sums,
    finalize) behind the signed-distance ones, and one backward; the scalar algebra never leaves the device.  In the exact
    data-parallel mode the sums are all-reduced and the element count is the global one: the local backward yields this rank's share
    of the whole-batch gradient (as _GlobalMeanFn); phi is local."""

    @staticmethod
    def forward(ctx, family, outputs, targets, w_dice, w4, scale, eps, extra):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        from stroke_prediction_amd.runtime.layers import SYNC, _allreduce
        fam = _FAMILIES[family]
        o, obs = _batch_strided(outputs)
        t, tbs = _batch_strided(targets)
        B, C = o.shape[0], o.shape[1]
        dhw = o.numel() // (B * C)
        phi = [signed_distance_batch(t)] if fam.phi else []
        # ONE accumulator per (family, device, C), zeroed once: finalize_clear leaves it zero again (no fill launch per call -- 5 us of a
        # captured step's dependent chain).  ``busy``: a call that died between the two launches left sums behind -> zero them here.
        key = (family, o.device, C, int(torch.cuda.current_stream(o.device).cuda_stream))      # (per stream: launches of one stream are ordered)
        ent = _CRIT_SUMS.get(key)
        if ent is None or ent[1]:
            ent = _CRIT_SUMS[key] = [torch.zeros(L.SP_REDUCE_ROWS, fam.pitch(L, C), dtype=torch.float64, device=o.device), False]
        sums = ent[0]   # replica rows
        ent[1] = True
        L.call(fam.sums, O.ptr(o), obs, O.ptr(t), tbs, *[O.ptr(p) for p in phi], B, C, dhw, *fam.select(L, w_dice, w4), *fam.sums_scalars(extra),
               O.ptr(sums), O.stream())
        count = float(B * dhw)
        if SYNC["on"]:                  # ratios and means of WHOLE-batch sums (metrics.py:24-27): make them global
            _allreduce(sums)
            count *= SYNC["world"]
        # cached weights: no host->device copy inside a (graph-captured) step
        ws = [None if w is None else O.ptr(_weights_on(o.device, w)) for w in ((w_dice, w4) if fam.fourth else (w_dice,))]
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        coef = torch.empty(fam.ncoef * C, dtype=torch.float32, device=o.device)
        L.call(fam.finalize, O.ptr(sums), *ws, *([O.ptr(scale)] if fam.phi else []), *fam.finalize_scalars(extra), float(eps),
               *([count] if fam.fourth else []), C, O.ptr(loss), O.ptr(coef), O.stream())
        ent[1] = False
        ctx.save_for_backward(o, t, *phi, coef)
        ctx.family, ctx.strides, ctx.extra = family, (obs, tbs), extra
        return loss

    @staticmethod
    def backward(ctx, gloss):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        o, t, *phi, coef = ctx.saved_tensors
        obs, tbs = ctx.strides
        B, C = o.shape[0], o.shape[1]
        up = gloss if (gloss.dtype == torch.float32 and gloss.is_contiguous()) else gloss.float().contiguous()
        d = torch.empty(o.shape, dtype=torch.float32, device=o.device)
        fam = _FAMILIES[ctx.family]
        L.call(fam.bwd, O.ptr(o), obs, O.ptr(t), tbs, *[O.ptr(p) for p in phi], O.ptr(coef), O.ptr(up), *fam.bwd_scalars(ctx.extra), B, C,
               o.numel() // (B * C), O.ptr(d), O.stream())
        return None, d, None, None, None, None, None, None


class BatchDiceLoss(LossModule):
    def __init__(self, label_weights, epsilon=0.0000001, dim=1):
        super(BatchDiceLoss, self).__init__()
        self._epsilon = epsilon
        self._dim = dim
        self._label_weights = label_weights
        print("DICE Loss weights classes' output by", label_weights)

    def forward(self, outputs, targets):
        assert targets.shape[self._dim] == len(self._label_weights), \
            'Ground truth number of labels does not match with label weight vector'
        assert outputs.shape == targets.shape
        if not outputs.is_cuda or self._dim != 1:
            raise RuntimeError("BatchDiceLoss (stroke_prediction_amd) runs on the GPU with channel dim 1 only")
        return _CriterionFn.apply("dice", outputs, targets, tuple(float(w) for w in self._label_weights), None, None, float(self._epsilon), None)


def _check_voxel_loss_inputs(name, outputs, targets, label_weights):
    assert label_weights is None or targets.shape[1] == len(label_weights), \
        'Ground truth number of labels does not match with label weight vector'
    assert outputs.shape == targets.shape
    if not outputs.is_cuda:
        raise RuntimeError("%s (stroke_prediction_amd) runs on the GPU with channel dim 1 only" % name)


class BCELoss(LossModule):
    """``torch.nn.BCELoss()`` on (B, C, ...) GPU tensors (channel dim 1): sum_c w_c mean_c bce.  The default weights, 1 / C each, are
    the mean over everything."""

    def __init__(self, label_weights=None):
        super(BCELoss, self).__init__()
        self._label_weights = label_weights
        self._dim = 1

    def weights(self, C):
        if self._label_weights is None:
            return (1.0 / C,) * C
        return tuple(float(w) for w in self._label_weights)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("BCELoss", outputs, targets, self._label_weights)
        return _CriterionFn.apply("vloss", outputs, targets, None, self.weights(outputs.shape[1]), None, 0.0, None)


class DiceBCELoss(LossModule):
    """``BatchDiceLoss(label_weights, epsilon)(o, t) + bce_weight * BCELoss()(o, t)`` in one sums / finalize / backward set."""

    def __init__(self, label_weights, bce_weight=1.0, epsilon=0.0000001):
        super(DiceBCELoss, self).__init__()
        self._label_weights = label_weights
        self._bce_weight = bce_weight
        self._epsilon = epsilon
        self._dim = 1

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("DiceBCELoss", outputs, targets, self._label_weights)
        C = outputs.shape[1]
        return _CriterionFn.apply("vloss", outputs, targets, tuple(float(w) for w in self._label_weights),
                                  (float(self._bce_weight) / C,) * C, None, float(self._epsilon), None)


def signed_distance_workspace_floats(B, C, D, H, W):
    """floats of workspace ``sp_signed_distance_batch`` needs: 4 B C D H W + 64 B C"""
    import ctypes as CT
    from stroke_prediction_amd.runtime import lib as L
    n = CT.c_int64(0)
    L.call("sp_signed_distance_batch_workspace", int(B), int(C), int(D), int(H), int(W), CT.byref(n))
    return int(n.value)


def signed_distance_batch(targets):
    """phi (B, C, D, H, W) fp32 of a (B, C, D, H, W) GPU label tensor (channel-slice views are read in place): per volume the signed
    Euclidean distance map of ``targets > 0.5`` -- positive outside, -(distance - 1) inside, zero for an empty or a full mask.  Five
    launches at most whatever B and C, no host read; the map and the workspace come from torch's allocator (the graph pool under
    capture)."""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    if not targets.is_cuda or targets.dim() != 5:
        raise RuntimeError("signed_distance_batch (stroke_prediction_amd) runs on the GPU on (B, C, D, H, W) tensors")
    t, tbs = _batch_strided(targets)
    B, C, D, H, W = t.shape
    phi = torch.empty((B, C, D, H, W), dtype=torch.float32, device=t.device)
    nws = signed_distance_workspace_floats(B, C, D, H, W)
    ws = torch.empty(nws, dtype=torch.float32, device=t.device)
    L.call("sp_signed_distance_batch", O.ptr(t), tbs, B, C, D, H, W, O.ptr(phi), O.ptr(ws), nws, O.stream())
    return phi


class _ScheduledBoundaryWeight(object):
    """The boundary term's scalar: a Python value and its copy in a persistent one-float device tensor (made on first use, per device)
    that the finalize kernel reads.  ``set_boundary_weight`` / ``adapt`` run between steps; a captured step is not re-captured."""

    def _init_schedule(self, weight, ramp=0.0):
        self._boundary_weight0 = float(weight)
        self._boundary_ramp = float(ramp)
        self._boundary_weight = float(weight)
        self._scale_dev = {}

    def boundary_weight(self):
        return self._boundary_weight

    def set_boundary_weight(self, w):
        """host value and every device copy (one host -> device copy each); call it outside the step"""
        self._boundary_weight = float(w)
        for dev_scale in self._scale_dev.values():
            dev_scale.copy_(torch.tensor([self._boundary_weight], dtype=torch.float32))

    def set_boundary_schedule(self, weight, ramp=0.0):
        """weight at epoch 0 and its growth per epoch (``adapt``)"""
        self._boundary_weight0 = float(weight)
        self._boundary_ramp = float(ramp)
        self.set_boundary_weight(weight)

    def adapt(self, epoch):
        """min(1.0, w0 + ramp * epoch): the rebalancing schedule of the paper (ramp 0.01); Learner.adapt_criterion calls it"""
        self.set_boundary_weight(min(1.0, self._boundary_weight0 + self._boundary_ramp * epoch))

    def _scale_on(self, device):
        key = str(device)
        if key not in self._scale_dev:
            self._scale_dev[key] = torch.tensor([self._boundary_weight], dtype=torch.float32, device=device)
        return self._scale_dev[key]


class BoundaryLoss(LossModule, _ScheduledBoundaryWeight):
    """``weight * sum_c w_c mean_c(o * phi_c(t))`` on (B, C, D, H, W) GPU tensors (channel dim 1), phi the signed distance map of
    ``t > 0.5`` per sample and channel (``signed_distance_batch``).  The default channel weights, 1 / C each, are the mean over
    everything.  No gradient goes to the targets."""

    def __init__(self, label_weights=None, weight=1.0):
        super(BoundaryLoss, self).__init__()
        self._label_weights = label_weights
        self._dim = 1
        self._init_schedule(weight)

    def weights(self, C):
        if self._label_weights is None:
            return (1.0 / C,) * C
        return tuple(float(w) for w in self._label_weights)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("BoundaryLoss", outputs, targets, self._label_weights)
        return _CriterionFn.apply("bloss", outputs, targets, None, self.weights(outputs.shape[1]), self._scale_on(outputs.device), 0.0, None)


class DiceBoundaryLoss(LossModule, _ScheduledBoundaryWeight):
    """``BatchDiceLoss(label_weights, epsilon)(o, t) + boundary_weight * BoundaryLoss()(o, t)`` in one signed-distance set and one
    sums / finalize / backward set; ``adapt(epoch)`` moves boundary_weight along its ramp."""

    def __init__(self, label_weights, boundary_weight=0.01, epsilon=0.0000001):
        super(DiceBoundaryLoss, self).__init__()
        self._label_weights = label_weights
        self._epsilon = epsilon
        self._dim = 1
        self._init_schedule(boundary_weight)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("DiceBoundaryLoss", outputs, targets, self._label_weights)
        C = outputs.shape[1]
        return _CriterionFn.apply("bloss", outputs, targets, tuple(float(w) for w in self._label_weights), (1.0 / C,) * C,
                                  self._scale_on(outputs.device), float(self._epsilon), None)


def _check_tversky(name, fp_weight, fn_weight, gamma):
    if not (fp_weight >= 0.0 and fn_weight >= 0.0):
        raise ValueError("%s: fp_weight and fn_weight are at least 0 (got %r, %r)" % (name, fp_weight, fn_weight))
    if not gamma >= 1.0:
        raise ValueError("%s: the Tversky gamma is at least 1 (got %r)" % (name, gamma))


def _check_focal(name, gamma, alpha):
    if not (gamma == 0.0 or gamma >= 1.0):
        raise ValueError("%s: the focal gamma is 0 or at least 1 (got %r)" % (name, gamma))
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("%s: alpha lies in [0, 1] (got %r)" % (name, alpha))


class TverskyLoss(LossModule):
    """``sum_c w_c (1 - TI_c)^(1/gamma)`` on (B, C, ...) GPU tensors (channel dim 1), TI = (TP + eps) / (TP + fp_weight FP +
    fn_weight FN + eps) with the soft counts TP = sum o t, FP = sum o (1 - t), FN = sum (1 - o) t over batch and volume.  fp_weight =
    fn_weight = 0.5 is the Dice index on first moments; fn_weight > fp_weight favours recall.  ``gamma = 4/3`` is the focal Tversky loss.
    A channel with TI = 1 (a perfect or an empty one) has a finite loss and no gradient."""

    def __init__(self, label_weights, fp_weight=0.3, fn_weight=0.7, gamma=1.0, epsilon=0.0000001):
        super(TverskyLoss, self).__init__()
        self._label_weights = label_weights
        self._fp_weight = fp_weight
        self._fn_weight = fn_weight
        self._gamma = gamma
        self._epsilon = epsilon
        self._dim = 1
        self.check()

    def check(self):
        _check_tversky("TverskyLoss", self._fp_weight, self._fn_weight, self._gamma)

    def extra(self):
        return float(self._fp_weight), float(self._fn_weight), float(self._gamma), 2.0, 0.25      # (no focal term: its scalars are not read)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("TverskyLoss", outputs, targets, self._label_weights)
        return _CriterionFn.apply("tloss", outputs, targets, tuple(float(w) for w in self._label_weights), None, None, float(self._epsilon),
                                  self.extra())


class FocalBCELoss(LossModule):
    """``sum_c w_c mean_c fl(o, t)``, fl = -alpha t (1 - o)^gamma log o - (1 - alpha) (1 - t) o^gamma log(1 - o) with the logarithms
    clamped at -100 as ``torch.nn.BCELoss`` clamps them, on (B, C, ...) GPU tensors (channel dim 1).  The default weights, 1 / C each, are
    the mean over everything; ``gamma = 0, alpha = 0.5`` is half of ``BCELoss()``.  gamma is 0 or at least 1."""

    def __init__(self, label_weights=None, gamma=2.0, alpha=0.25):
        super(FocalBCELoss, self).__init__()
        self._label_weights = label_weights
        self._gamma = gamma
        self._alpha = alpha
        self._dim = 1
        self.check()

    def check(self):
        _check_focal("FocalBCELoss", self._gamma, self._alpha)

    def weights(self, C):
        if self._label_weights is None:
            return (1.0 / C,) * C
        return tuple(float(w) for w in self._label_weights)

    def extra(self):
        return 0.0, 0.0, 1.0, float(self._gamma), float(self._alpha)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("FocalBCELoss", outputs, targets, self._label_weights)
        return _CriterionFn.apply("tloss", outputs, targets, None, self.weights(outputs.shape[1]), None, 0.0, self.extra())


class TverskyFocalBCELoss(LossModule):
    """``TverskyLoss(label_weights, fp_weight, fn_weight, tversky_gamma, epsilon)(o, t) + focal_weight * FocalBCELoss(None, focal_gamma,
    focal_alpha)(o, t)`` in one sums / finalize / backward set."""

    def __init__(self, label_weights, focal_weight=1.0, fp_weight=0.3, fn_weight=0.7, tversky_gamma=1.0, focal_gamma=2.0, focal_alpha=0.25,
                 epsilon=0.0000001):
        super(TverskyFocalBCELoss, self).__init__()
        self._label_weights = label_weights
        self._focal_weight = focal_weight
        self._fp_weight = fp_weight
        self._fn_weight = fn_weight
        self._tversky_gamma = tversky_gamma
        self._focal_gamma = focal_gamma
        self._focal_alpha = focal_alpha
        self._epsilon = epsilon
        self._dim = 1
        self.check()

    def check(self):
        _check_tversky("TverskyFocalBCELoss", self._fp_weight, self._fn_weight, self._tversky_gamma)
        _check_focal("TverskyFocalBCELoss", self._focal_gamma, self._focal_alpha)

    def extra(self):
        return float(self._fp_weight), float(self._fn_weight), float(self._tversky_gamma), float(self._focal_gamma), float(self._focal_alpha)

    def forward(self, outputs, targets):
        _check_voxel_loss_inputs("TverskyFocalBCELoss", outputs, targets, self._label_weights)
        C = outputs.shape[1]
        return _CriterionFn.apply("tloss", outputs, targets, tuple(float(w) for w in self._label_weights),
                                  (float(self._focal_weight) / C,) * C, None, float(self._epsilon), self.extra())


def _single_label_imbalance_terms(criterion):
    """(Tversky weight or None, focal weight or None, eps, extra) of a TverskyLoss / FocalBCELoss / TverskyFocalBCELoss that weighs ONE
    label class -- what ``mean_of_channel_losses`` evaluates per channel --, or None for anything else."""
    if getattr(criterion, "_dim", None) != 1:
        return None
    if isinstance(criterion, TverskyLoss) and len(criterion._label_weights) == 1:
        return float(criterion._label_weights[0]), None, float(criterion._epsilon), criterion.extra()
    if isinstance(criterion, FocalBCELoss) and (criterion._label_weights is None or len(criterion._label_weights) == 1):
        return None, criterion.weights(1)[0], 0.0, criterion.extra()
    if isinstance(criterion, TverskyFocalBCELoss) and len(criterion._label_weights) == 1:
        return float(criterion._label_weights[0]), float(criterion._focal_weight), float(criterion._epsilon), criterion.extra()
    return None


def _single_label_boundary_terms(criterion):
    """(Dice weight or None, boundary channel weight, eps) of a BoundaryLoss / DiceBoundaryLoss that weighs ONE label class -- what
    ``mean_of_channel_losses`` evaluates per channel --, or None for anything else."""
    if getattr(criterion, "_dim", None) != 1:
        return None
    if isinstance(criterion, BoundaryLoss) and (criterion._label_weights is None or len(criterion._label_weights) == 1):
        return None, criterion.weights(1)[0], 0.0
    if isinstance(criterion, DiceBoundaryLoss) and len(criterion._label_weights) == 1:
        return float(criterion._label_weights[0]), 1.0, float(criterion._epsilon)
    return None


def _single_label_terms(criterion):
    """(Dice weight or None, BCE weight or None, eps) of a criterion that weighs ONE label class -- what the fused routes below
    evaluate per channel / per reconstruction --, or None for anything else."""
    if getattr(criterion, "_dim", None) != 1:
        return None
    if isinstance(criterion, BatchDiceLoss) and len(criterion._label_weights) == 1:
        return float(criterion._label_weights[0]), None, float(criterion._epsilon)
    if isinstance(criterion, BCELoss) and (criterion._label_weights is None or len(criterion._label_weights) == 1):
        return None, criterion.weights(1)[0], 0.0
    if isinstance(criterion, DiceBCELoss) and len(criterion._label_weights) == 1:
        return float(criterion._label_weights[0]), float(criterion._bce_weight), float(criterion._epsilon)
    return None


def make_criterion(name):
    """The training scripts' ``--criterion``: ``dice`` (the reference's choice), ``bce`` (the one its comment names), ``dicebce``,
    ``boundary`` (the signed-distance loss), ``diceboundary`` (Dice + boundary weight * boundary loss) and the class-imbalance
    criteria ``tversky``, ``focaltversky`` (Tversky with gamma 4/3), ``focalbce`` and ``tverskyfocalbce`` (Tversky + focal weight * focal
    cross entropy)."""
    if name == "dice":
        return BatchDiceLoss([1.0])
    if name == "bce":
        return BCELoss()
    if name == "dicebce":
        return DiceBCELoss([1.0])
    if name == "boundary":
        return BoundaryLoss()
    if name == "diceboundary":
        return DiceBoundaryLoss([1.0])
    if name == "tversky":
        return TverskyLoss([1.0])
    if name == "focaltversky":
        return TverskyLoss([1.0], gamma=4.0 / 3.0)
    if name == "focalbce":
        return FocalBCELoss()
    if name == "tverskyfocalbce":
        return TverskyFocalBCELoss([1.0])
    raise ValueError("criterion %r: one of dice, bce, dicebce, boundary, diceboundary, tversky, focaltversky, focalbce, tverskyfocalbce" % (name,))


def configure_criterion(criterion, args):
    """Apply the training scripts' ``--boundaryweight`` / ``--boundaryramp`` to a criterion that has a boundary term, and
    ``--tverskyfp`` / ``--tverskyfn`` / ``--tverskygamma`` / ``--focalgamma`` / ``--focalalpha`` / ``--focalweight`` (None = the
    criterion's own value) to one that has the matching term; any other criterion is returned as it is."""
    if isinstance(criterion, (BoundaryLoss, DiceBoundaryLoss)):
        criterion.set_boundary_schedule(getattr(args, "boundaryweight", criterion.boundary_weight()), getattr(args, "boundaryramp", 0.0))
    fields = {TverskyLoss: dict(tverskyfp="_fp_weight", tverskyfn="_fn_weight", tverskygamma="_gamma"),
              FocalBCELoss: dict(focalgamma="_gamma", focalalpha="_alpha"),
              TverskyFocalBCELoss: dict(tverskyfp="_fp_weight", tverskyfn="_fn_weight", tverskygamma="_tversky_gamma", focalgamma="_focal_gamma",
                                        focalalpha="_focal_alpha", focalweight="_focal_weight")}.get(type(criterion))
    if fields is not None:
        for flag, field in fields.items():
            if getattr(args, flag, None) is not None:
                setattr(criterion, field, float(getattr(args, flag)))
        criterion.check()
    return criterion


class _CaeLossFn(torch.autograd.Function):
    """CaeReconstructionLearner.loss_step (reference :52-70) as three HIP launches (sp_cae_loss_crit_fwd / _bwd) instead of ~60 torch and
    criterion kernels: [ mean(|p-i|-(p-i)) + mean(|p-c|-(p-c)) + crit(c) + crit(p) + crit(l) + f mean|zi - zl| ] / (5 + f), crit =
    BatchDiceLoss, BCELoss or DiceBCELoss.  The four gradients come back as consecutive slices of ONE tensor in the order the
    reconstructions lie in memory, so that a decoder call that produced them stacked on the batch axis (Cae3D._StackManyFn) takes the
    buffer as it is."""

    @staticmethod
    def forward(ctx, c, p, l, i, tc, tp, tl, zi, zl, factor, weight, eps, bce_weight=None):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        recs = [_batch_strided(t) for t in (c, p, l, i)]
        gts = [_batch_strided(t) for t in (tc, tp, tl)]
        zi_, zl_ = zi.contiguous().float(), zl.contiguous().float()
        B = c.shape[0]
        dhw = c.numel() // B
        dev = c.device
        sums = torch.zeros(L.SP_REDUCE_ROWS, 16, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(11, dtype=torch.float32, device=dev)
        args = []
        for t, bs in recs + gts:
            args += [O.ptr(t), bs]
        # weight / bce_weight None = no Dice / no BCE term
        terms = (L.SP_VLOSS_DICE if weight is not None else 0) | (L.SP_VLOSS_BCE if bce_weight is not None else 0)
        L.call("sp_cae_loss_crit_fwd", *args, B, dhw, O.ptr(zi_), O.ptr(zl_), zi_.numel(), float(weight or 0.0), float(bce_weight or 0.0), terms,
               float(eps), float(factor), O.ptr(sums), O.ptr(loss), O.ptr(coef), O.stream())
        ctx.save_for_backward(*[t for t, _ in recs + gts], zi_, zl_, coef)
        ctx.strides = [bs for _, bs in recs + gts]
        ctx.shapes = (tuple(c.shape), tuple(zi.shape), tuple(zl.shape))
        return loss

    @staticmethod
    def backward(ctx, gloss):
        from stroke_prediction_amd.runtime import lib as L, ops as O
        *ts, zi_, zl_, coef = ctx.saved_tensors
        B = ts[0].shape[0]
        dhw = ts[0].numel() // B
        up = gloss if (gloss.dtype == torch.float32 and gloss.is_contiguous()) else gloss.float().contiguous()
        # slot k of the gradient buffer for the reconstruction that lies k-th in memory (equal spacing = slices of one stacked tensor)
        order = sorted(range(4), key=lambda k: ts[k].data_ptr())
        dall = torch.empty((4 * B,) + ctx.shapes[0][1:], dtype=torch.float32, device=ts[0].device)
        d = [None] * 4
        for slot, k in enumerate(order):
            d[k] = dall[slot * B:(slot + 1) * B]
        dzi, dzl = torch.empty_like(zi_), torch.empty_like(zl_)
        args = []
        for t, bs in zip(ts, ctx.strides):
            args += [O.ptr(t), bs]
        L.call("sp_cae_loss_crit_bwd", *args, B, dhw, O.ptr(coef), O.ptr(up), O.ptr(d[0]), O.ptr(d[1]),
               O.ptr(d[2]), O.ptr(d[3]), O.ptr(zi_), O.ptr(zl_), zi_.numel(), O.ptr(dzi), O.ptr(dzl), O.stream())
        return d[0], d[1], d[2], d[3], None, None, None, dzi.view(ctx.shapes[1]), dzl.view(ctx.shapes[2]), None, None, None, None


def cae_reconstruction_loss(rec, gt, lat, factor, criterion):
    """The loss of CaeReconstructionLearner.loss_step on the fused kernels, or None when they do not apply (host tensors, the
    exact data-parallel mode -- its means and Dice sums are global --, several label classes): the caller composes it then."""
    import os
    from stroke_prediction_amd.runtime.layers import SYNC
    ts = (rec.core, rec.penu, rec.lesion, rec.interpolation, gt.core, gt.penu, gt.lesion)
    terms = _single_label_terms(criterion)       # BatchDiceLoss, BCELoss or DiceBCELoss of one label class
    if os.environ.get("SP_CAE_FUSED_LOSS", "1") == "0" or SYNC["on"] or terms is None or any(t is None or not t.is_cuda or t.dim() != 5 or t.shape[1] != 1 or t.shape != ts[0].shape for t in ts) \
            or lat.interpolation is None or lat.lesion is None or lat.interpolation.shape != lat.lesion.shape:
        return None
    w_dice, w_bce, eps = terms
    return _CaeLossFn.apply(rec.core, rec.penu, rec.lesion, rec.interpolation, gt.core.float(), gt.penu.float(), gt.lesion.float(),
                            lat.interpolation, lat.lesion, float(factor), w_dice, eps, w_bce)


def _stacked_base(parts):
    """The (B, n, ...) fp32 tensor whose consecutive channel slices are exactly ``parts`` (each (B, 1, ...)), or None."""
    base = getattr(parts[0], "_base", None)
    n = len(parts)
    if base is None or base.dtype != torch.float32 or not base.is_contiguous() or base.dim() != parts[0].dim() \
            or base.shape[1] != n or base.shape[0] != parts[0].shape[0] or tuple(base.shape[2:]) != tuple(parts[0].shape[2:]):
        return None
    per = base[0, 0].numel()
    for i, p in enumerate(parts):
        if getattr(p, "_base", None) is not base or p.shape[1] != 1 or p.dtype != torch.float32 \
                or p.data_ptr() != base.data_ptr() + 4 * i * per or _batch_strided(p)[1] != n * per:
            return None
    return base


def mean_of_channel_losses(criterion, outputs, targets):
    """mean_i criterion(outputs[i], targets[i]) -- the reference's ``(Dice(core) + Dice(penu)) / 2``
    (learner/UnetSegmentationLearner.py:21-28).  When the criterion is a single-label BatchDiceLoss and the pairs are the
    consecutive channel slices of one segmentation tensor and one label tensor (what Unet3D.forward / UnetInference
    produce), this is BatchDiceLoss over n channels with weights w/n: evaluated in one sums / finalize / backward
    launch on the base tensors, and the gradient lands on the segmentation directly (no slice-backward zero-fill,
    copy and add per channel).  A single-label BCELoss (weights 1/n) or DiceBCELoss (Dice weights w/n, BCE weights
    bce_weight/n) takes the same route on the sp_vloss_* kernels, a single-label BoundaryLoss / DiceBoundaryLoss on
    sp_signed_distance_batch and the sp_bloss_* kernels (one signed-distance set for all n channels), a single-label TverskyLoss /
    FocalBCELoss / TverskyFocalBCELoss on the sp_tloss_* kernels (Tversky weights w/n, focal weights w/n).  Anything else: the literal
    sum of calls."""
    n = len(outputs)
    family, terms, extra = "bloss", _single_label_boundary_terms(criterion), None
    imbalance = _single_label_imbalance_terms(criterion)
    if imbalance is not None:
        family, terms, extra = "tloss", imbalance[:3], imbalance[3]
    if terms is None:
        terms = _single_label_terms(criterion)
        family = "dice" if terms is not None and terms[1] is None else "vloss"
    if terms is not None and n > 1 and outputs[0].is_cuda and (family != "bloss" or outputs[0].dim() == 5):
        ob, tb = _stacked_base(outputs), _stacked_base(targets)
        if ob is not None and tb is not None:
            w_dice, w4, eps = terms
            return _CriterionFn.apply(family, ob, tb, None if w_dice is None else (w_dice / n,) * n, None if w4 is None else (w4 / n,) * n,
                                      criterion._scale_on(ob.device) if family == "bloss" else None, eps, extra)
    total = criterion(outputs[0], targets[0])
    for o, t in zip(outputs[1:], targets[1:]):
        total = total + criterion(o, t)
    return total / n


# ---------------------------------------------------------------------------------------------- evaluation measures

def _measures_from_counts(tp, fp, fn, tn):
    size = (tp + fp) + (tp + fn)
    return BinaryMeasuresDto(2.0 * tp / size if size > 0 else 0.0, numpy.inf, numpy.inf,
                             tp / (tp + fp) if tp + fp > 0 else 0.0,
                             tp / (tp + fn) if tp + fn > 0 else 0.0,
                             tn / (tn + fp) if tn + fp > 0 else 0.0)


def binary_measures_numpy(result, target, binary_threshold=0.5, distances=True):
    """``metrics.py:31-46`` of the reference for host arrays: uploaded once and measured on the device like
    ``binary_measures_torch`` (there is no CPU implementation in this package; MedPy, which the reference calls, is
    restated only as the test oracle ``oracle/measures.py``)."""
    if not torch.cuda.is_available():
        raise RuntimeError("binary_measures_numpy (stroke_prediction_amd) measures on the GPU: no CUDA device available")
    r = torch.from_numpy(numpy.ascontiguousarray(result, dtype=numpy.float32)).cuda()
    t = torch.from_numpy(numpy.ascontiguousarray(target, dtype=numpy.float32)).cuda()
    return binary_measures_torch(r, t, True, binary_threshold=binary_threshold, distances=distances)


DISTANCE_METRICS = True      # Hausdorff / ASSD as the reference's batch metrics report them (metrics.py:42-44)


_SD_WS = {}


def _surface_distances_launch(r, t, threshold):
    """Enqueue sp_surface_distances; returns the fp64[6] result tensor (no synchronisation)."""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    dims = torch.tensor(list(r.shape), dtype=torch.int32)            # host array: read by the launcher, not the kernels
    key = (r.device, r.numel())
    if key not in _SD_WS:
        _SD_WS.clear()                                               # one workspace (4 volumes) alive at a time
        _SD_WS[key] = torch.empty(4 * r.numel(), dtype=torch.float32, device=r.device)
    out = torch.zeros(6, dtype=torch.float64, device=r.device)
    L.call("sp_surface_distances", O.ptr(r), O.ptr(t), float(threshold), r.dim(), dims.data_ptr(), O.ptr(_SD_WS[key]), O.ptr(out),
           O.stream())
    return out


def _surface_metrics_device(r, t, threshold):
    """(hd, assd) of two CUDA fp32 tensors of equal shape (rank <= 5), medpy semantics -- see sp_surface_distances."""
    mx_rt, sm_rt, n_r, mx_tr, sm_tr, n_t = _surface_distances_launch(r, t, threshold).tolist()
    return float(numpy.sqrt(max(mx_rt, mx_tr))), 0.5 * (sm_rt / n_r + sm_tr / n_t)


def binary_measures_torch(result, target, cuda, binary_threshold=0.5, distances=None):
    """``metrics.py:48-62`` of the reference.  Tensors on the GPU: the four confusion counts come from one HIP reduction
    (``sp_confusion_counts``, 32 bytes to the host); the volumes are copied to the host only for the surface distances,
    and only when ``distances`` (default: module flag ``DISTANCE_METRICS``) asks for them."""
    distances = DISTANCE_METRICS if distances is None else distances
    if isinstance(result, torch.Tensor) and isinstance(target, torch.Tensor) and result.is_cuda and target.is_cuda:
        from stroke_prediction_amd.runtime import lib as L, ops as O
        r = result.detach().float().contiguous()
        t = target.detach().float().contiguous()
        counts = torch.zeros(4, dtype=torch.int64, device=r.device)
        L.call("sp_confusion_counts", O.ptr(r), O.ptr(t), float(binary_threshold), r.numel(), O.ptr(counts), O.stream())
        if distances and r.dim() > 5:
            raise ValueError("surface distances: tensors of rank <= 5 (got %d)" % r.dim())
        sd = _surface_distances_launch(r, t, binary_threshold) if distances else None    # enqueued before the one sync below
        tp, fp, fn, tn = (float(v) for v in counts.tolist())
        out = _measures_from_counts(tp, fp, fn, tn)
        if distances and tp + fp > 0 and tp + fn > 0:
            mx_rt, sm_rt, n_r, mx_tr, sm_tr, n_t = sd.tolist()
            out.hd, out.assd = float(numpy.sqrt(max(mx_rt, mx_tr))), 0.5 * (sm_rt / n_r + sm_tr / n_t)
        return out
    # host tensors / arrays: same measures, on the device
    result = result.detach().cpu().numpy() if isinstance(result, torch.Tensor) else result
    target = target.detach().cpu().numpy() if isinstance(target, torch.Tensor) else target
    return binary_measures_numpy(result, target, binary_threshold=binary_threshold, distances=distances)


_MANY_WS = {}


def measures_many_workspace_floats(T, nvox):
    """floats of workspace ``sp_binary_measures_many`` needs for T results of nvox voxels each: 2 * (T + 1) * nvox"""
    import ctypes as C
    from stroke_prediction_amd.runtime import lib as L
    n = C.c_int64(0)
    L.call("sp_binary_measures_many_workspace", int(T), int(nvox), C.byref(n))
    return int(n.value)


def binary_measures_many_torch(results, target, cuda, binary_threshold=0.5, distances=None):
    """``binary_measures_torch(results[t:t+1], target, ...)`` for every leading entry t of ``results`` -- a (T, 1, D, H, W) tensor or
    a list of (1, 1, D, H, W) tensors -- against ONE ``target`` (1, 1, D, H, W), as a list of ``BinaryMeasuresDto``: the points of
    the time-to-treatment curve, all measured against the same follow-up lesion.  One enqueue (``sp_binary_measures_many``: the
    target's border and distance transform once, the T results' in the same launches) and one device -> host read for all T."""
    distances = DISTANCE_METRICS if distances is None else distances
    stride = None
    if not isinstance(results, torch.Tensor):
        parts = [r.detach() for r in results]
        step = parts[1].data_ptr() - parts[0].data_ptr() if len(parts) > 1 else 0
        if len(parts) > 1 and step >= 4 * parts[0].numel() and step % 4 == 0 and all(
                p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.shape == parts[0].shape and p.shape[0] == 1
                and p.data_ptr() == parts[0].data_ptr() + k * step for k, p in enumerate(parts)):
            # equally spaced in memory (slices of one tensor, as inference_curve returns them): measured where they lie
            results, stride = parts[0].expand((len(parts),) + tuple(parts[0].shape[1:])), step // 4
        else:
            results = torch.cat([p.float() for p in parts], 0)
    if not (results.is_cuda and isinstance(target, torch.Tensor) and target.is_cuda):
        raise RuntimeError("binary_measures_many_torch (stroke_prediction_amd) measures tensors on the GPU")
    from stroke_prediction_amd.runtime import lib as L, ops as O
    r = results if stride is not None else results.detach().float().contiguous()     # (with a stride: only shape and pointer are used)
    t = target.detach().float().contiguous()
    T = r.shape[0]
    if T < 1 or t.shape[0] != 1 or tuple(r.shape[1:]) != tuple(t.shape[1:]):
        raise ValueError("binary_measures_many_torch: results %s against target %s (want (T, ...) against (1, ...))"
                         % (tuple(r.shape), tuple(t.shape)))
    if t.dim() > 5:
        raise ValueError("surface distances: tensors of rank <= 5 (got %d)" % t.dim())
    nvox = t.numel()
    stride = nvox if stride is None else stride
    dims = torch.tensor(list(t.shape), dtype=torch.int32)            # host array: read by the launcher, not the kernels
    key = (r.device, T, nvox)
    if key not in _MANY_WS:
        _MANY_WS.clear()                                             # one workspace alive at a time
        _MANY_WS[key] = torch.empty(measures_many_workspace_floats(T, nvox), dtype=torch.float32, device=r.device)
    # counts[T][4] (uint64) and out[T][6] (fp64) in one 8-byte-element buffer: one read brings both to the host
    buf = torch.zeros(10 * T, dtype=torch.float64, device=r.device)
    L.call("sp_binary_measures_many", O.ptr(r), stride, T, O.ptr(t), float(binary_threshold), t.dim(), dims.data_ptr(),
           O.ptr(_MANY_WS[key]), O.ptr(buf), buf.data_ptr() + 32 * T, O.stream())
    host = buf.cpu().numpy()
    counts = host[:4 * T].view(numpy.int64).reshape(T, 4)
    sd = host[4 * T:].reshape(T, 6)
    out = []
    for k in range(T):
        tp, fp, fn, tn = (float(v) for v in counts[k])
        m = _measures_from_counts(tp, fp, fn, tn)
        if distances and tp + fp > 0 and tp + fn > 0:
            mx_rt, sm_rt, n_r, mx_tr, sm_tr, n_t = (float(v) for v in sd[k])
            m.hd, m.assd = float(numpy.sqrt(max(mx_rt, mx_tr))), 0.5 * (sm_rt / n_r + sm_tr / n_t)
        out.append(m)
    return out
