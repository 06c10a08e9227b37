"""Fused optimisers on flat buffers, drop-ins for the ``torch.optim`` classes of the same names.

``FusedAdam`` (``sp_adam_step_flat``) stands in for the ``torch.optim.Adam`` the reference scripts build
(train_unet_segmentation.py:32, train_shape_reconstruction.py:40): same constructor, ``param_groups`` / ``defaults``
(``adapt_betas`` edits ``param_group['betas']``, CaeReconstructionLearner.py:28-40), L2-coupled weight decay, bias correction,
no amsgrad.  ``FusedAdamW`` (decoupled weight decay) and ``FusedSGD`` (momentum, Nesterov) run the ``sp_optim_step_flat`` family
(csrc/sp_optim.hip), and so does ``FusedAdam`` once ``max_grad_norm`` is given: the global-norm gradient clipping of
``torch.nn.utils.clip_grad_norm_`` folded into the update -- one more launch (``sp_grad_sqnorm_partials``), no host read, so it
can be captured in a hipGraph.

When the parameters are the views of a ``FlatParamsMixin`` model the whole step is ONE kernel over the
flat parameter / gradient / moment buffers; otherwise it falls back to one launch per tensor.
``state_dict`` keeps the per-parameter layout of the torch class (step, exp_avg, exp_avg_sq / momentum_buffer).
"""
import torch
from torch.optim.optimizer import Optimizer

from stroke_prediction_amd.runtime import ops as O

MAX_PARTIALS = 256       # workgroups of the norm's first stage at most (sp_grad_sqnorm_partials)


class _FusedOptimizer(Optimizer):
    """What the fused optimisers share: the detection of flat groups, the device-resident hyper-parameter block and step count
    (``push_hyper`` / ``sync_step_from_device``), ``zero_grad``, the checkpoint layout and the ``sp_optim_step_flat`` route with
    its clipping.  A subclass names its per-parameter state tensors (``MOMENTS``: what the kernels call m and v), says whether it
    counts steps, and maps a parameter group to a kernel kind and to the hyper-parameter block."""
    MOMENTS = ("exp_avg", "exp_avg_sq")
    HAS_STEP = True

    def __init__(self, params, defaults, grad_scale=1.0, capturable=False, max_grad_norm=None):
        if max_grad_norm is not None:         # (a key only where it was asked for: param_groups otherwise stay torch's own)
            defaults = dict(defaults, max_grad_norm=float(max_grad_norm))
        super().__init__(params, defaults)
        self.grad_scale = grad_scale
        self.capturable = capturable      # step count in device memory: the step can be captured in a hipGraph
        self._flat = {}
        self._loose = {}                  # per group that is not flat: its hyper-parameter block and step count on the device
        self._clip = None                 # dict(partials, norm): created by the first clipped step
        self._clip_captured = None        # whether the captured step holds the norm's first stage

    # ------------------------------------------------------------------ what a subclass defines
    def _kind(self, group):
        raise NotImplementedError

    def _hyper(self, group):
        """{lr, beta1, beta2, eps, weight_decay, max_norm, momentum} as the kernels read them"""
        raise NotImplementedError

    @staticmethod
    def _max_norm(group):
        mn = group.get("max_grad_norm")
        return float(mn) if mn is not None and mn > 0 else 0.0

    # ------------------------------------------------------------------ flat detection
    def _flat_group(self, gi, group):
        """the group's flat buffers (p, g, m, v, step_dev, lr_dev) if its params and grads tile two contiguous buffers"""
        ps = group["params"]
        if not ps or any(p.grad is None or p.dtype != torch.float32 or not p.is_cuda for p in ps):
            return None
        p0, g0 = ps[0].data_ptr(), ps[0].grad.data_ptr()
        off = 0
        for p in ps:
            if p.data_ptr() != p0 + off or p.grad.data_ptr() != g0 + off or not p.is_contiguous():
                return None
            off += p.numel() * 4
        n = off // 4
        key = (gi, p0, g0, n)
        st = self._flat.get(gi)
        if st is None or st["key"] != key:
            dev = ps[0].device
            moments = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in self.MOMENTS]
            o = 0
            for p in ps:                      # keep (or adopt) per-parameter state as views of the flat moments
                s = self.state[p]
                k = p.numel()
                for name, flat in zip(self.MOMENTS, moments):
                    if s.get(name) is not None:
                        flat[o:o + k].copy_(s[name].reshape(-1))
                    s[name] = flat[o:o + k].view(p.shape)
                if self.HAS_STEP:
                    s.setdefault("step", 0)
                o += k
            # flat aliases of the parameter / gradient storage (torch owns the memory)
            pf = torch.as_strided(ps[0].data, (n,), (1,))
            gf = torch.as_strided(ps[0].grad, (n,), (1,))
            # step count: carried over from the flat group this one replaces (re-flatten after .cpu()/.cuda(): the
            # device counter is the truth in capturable mode), else from the per-parameter state
            step0 = int(self.state[ps[0]].get("step", 0))
            if st is not None and self.capturable:
                step0 = max(step0, int(st["step_dev"].item()))
            st = dict(key=key, p=pf, g=gf, m=moments[0], v=moments[1] if len(moments) > 1 else None,
                      step_dev=torch.full((1,), step0, dtype=torch.int32, device=dev),
                      lr_dev=torch.zeros(8, dtype=torch.float32, device=dev), hyper=None)
            self._flat[gi] = st
        return st

    def _loose_group(self, gi, group):
        """the device-resident hyper-parameter block and step count of a group whose tensors are not views of one buffer"""
        st = self._loose.get(gi)
        if st is None:
            ps = [p for p in group["params"] if p.grad is not None]
            dev = ps[0].device
            step0 = max([int(self.state[p].get("step", 0)) for p in ps if p in self.state] or [0])
            st = self._loose[gi] = dict(step_dev=torch.full((1,), step0, dtype=torch.int32, device=dev),
                                        lr_dev=torch.zeros(8, dtype=torch.float32, device=dev), hyper=None)
        return st

    # ------------------------------------------------------------------ the sp_optim_step_flat route
    def _step_family(self):
        """One update of every group through ``sp_optim_step_flat``.  With clipping: first the squared norm of EVERY gradient of
        the optimiser (one launch per flat group or loose tensor, accumulated into the same ``npartials`` doubles), then the
        updates, each of which forms the same coefficient from those doubles -- one global norm, as
        ``clip_grad_norm_(model.parameters(), ...)``."""
        from stroke_prediction_amd.runtime import lib as L
        capturing = torch.cuda.is_current_stream_capturing()
        work = []                                   # (group, block, [(p, g, m, v)])
        for gi, group in enumerate(self.param_groups):
            st = self._flat_group(gi, group)
            if st is not None:
                work.append((group, st, [(st["p"], st["g"], st["m"], st["v"])]))
                continue
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if any(not p.is_cuda or p.dtype != torch.float32 for p in ps):
                raise RuntimeError("%s runs on fp32 GPU tensors only" % type(self).__name__)
            tensors = []
            for p in ps:
                s = self.state[p]
                for name in self.MOMENTS:
                    if s.get(name) is None:
                        s[name] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if self.HAS_STEP:
                    s.setdefault("step", 0)
                tensors.append((p.data, p.grad.contiguous(), s[self.MOMENTS[0]], s[self.MOMENTS[1]] if len(self.MOMENTS) > 1 else None))
            work.append((group, self._loose_group(gi, group), tensors))
        clip = any(self._max_norm(group) > 0 for group, _, _ in work) or bool(self._clip_captured)
        if capturing:
            self._clip_captured = clip
        partials = norm = None
        npart = 0
        if clip and work:
            total = sum(t[0].numel() for _, _, ts in work for t in ts)
            npart = max(1, min(MAX_PARTIALS, -(-total // 1024)))
            if self._clip is None or self._clip["partials"].device != work[0][2][0][0].device:
                dev = work[0][2][0][0].device
                self._clip = dict(partials=torch.zeros(MAX_PARTIALS, dtype=torch.float64, device=dev),
                                  norm=torch.zeros(1, dtype=torch.float32, device=dev))
            partials, norm = self._clip["partials"], self._clip["norm"]
            first = True
            for _, _, ts in work:
                for _, g, _, _ in ts:
                    L.call("sp_grad_sqnorm_partials", O.ptr(g), g.numel(), O.ptr(partials), npart, 0 if first else 1, O.stream())
                    first = False
        for group, st, ts in work:
            # hyper-parameters live in device memory: while a hipGraph is being captured nothing is copied (a captured copy would
            # freeze today's values); ``push_hyper`` refreshes them before each replay
            if not capturing:
                self._push_hyper(st, group)
            if self.HAS_STEP:
                st["step_dev"].add_(1)
            kind = self._kind(group)
            for p, g, m, v in ts:
                L.call("sp_optim_step_flat", kind, O.ptr(p), O.ptr(g), O.ptr(m), O.ptr(v), p.numel(), O.ptr(st["lr_dev"]),
                       O.ptr(st["step_dev"]), self.grad_scale, O.ptr(partials), npart, O.ptr(norm), O.stream())
            if self.HAS_STEP and not self.capturable:      # (capturable: the device counter is the truth, read back on demand)
                for p in group["params"]:
                    if p.grad is not None:
                        self.state[p]["step"] = int(self.state[p].get("step", 0)) + 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        O.bump_param_epoch()          # packed weight fragments cached by the conv runners are stale after this
        self._step_family()
        return loss

    @property
    def last_grad_norm(self):
        """The gradient norm the last clipped step measured (``grad_scale`` included), as a one-element device tensor: turning it
        into a float is the caller's synchronisation.  ``None`` before the first clipped step."""
        return None if self._clip is None else self._clip["norm"]

    # ------------------------------------------------------------------ hyper-parameters on the device
    def _push_hyper(self, st, group):
        hyp = tuple(float(x) for x in self._hyper(group))
        if st["hyper"] != hyp:
            st["lr_dev"].copy_(torch.tensor(hyp + (0.0,) * (st["lr_dev"].numel() - len(hyp)), dtype=torch.float32), non_blocking=False)
            st["hyper"] = hyp

    def push_hyper(self):
        """capturable mode: copy lr / betas / eps / weight_decay / max_grad_norm / momentum of every group to the device if they
        changed (schedulers and ``adapt_betas`` edit ``param_groups`` on the host).  Call before replaying a captured step."""
        if self._clip_captured is False and any(self._max_norm(g) > 0 for g in self.param_groups):
            raise RuntimeError("max_grad_norm was switched on after the step was captured without the norm's launch: "
                               "construct the optimiser with max_grad_norm, or capture again")
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi) or self._loose.get(gi)
            if st is not None:
                self._push_hyper(st, group)

    def state_dict(self):
        """the torch class's layout; the step count of capturable mode lives on the device and is read back first."""
        if self.capturable:
            self.sync_step_from_device()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """The loaded state tensors / step replace the flat moments: drop the flat groups so that the next
        step re-adopts them from ``self.state`` (the cache key alone -- parameter addresses -- would not change)."""
        out = super().load_state_dict(state_dict)
        self._flat = {}
        self._loose = {}
        for group in self.param_groups:
            for p in group["params"]:
                s = self.state.get(p)
                if s is not None and "step" in s and torch.is_tensor(s["step"]):
                    s["step"] = int(s["step"].item())
        return out

    def sync_step_from_device(self):
        """capturable mode: copy the device step counters into the per-parameter state (before state_dict())."""
        if not self.HAS_STEP:
            return
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi) or self._loose.get(gi)
            if st is not None:
                step = int(st["step_dev"].item())
                for p in group["params"]:
                    if p in self.state or gi in self._flat:
                        self.state[p]["step"] = step

    def zero_grad(self, set_to_none=False):
        """Keeps ``p.grad`` attached (the flat gradient buffer is the kernels' accumulation target):
        one memset when the gradients are views of a flat buffer, per-tensor otherwise."""
        for gi, group in enumerate(self.param_groups):
            st = self._flat_group(gi, group)
            if st is not None:
                st["g"].zero_()
                continue
            for p in group["params"]:
                if p.grad is not None:
                    if p.grad.grad_fn is not None:
                        p.grad = p.grad.detach()
                    p.grad.zero_()


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` (L2-coupled weight decay).  Without ``max_grad_norm`` the step is ``sp_adam_step_flat`` /
    ``sp_adam_step_flat_hyp``; with it, kind ADAM of ``sp_optim_step_flat`` behind the norm's launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                 capturable=False, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults, grad_scale, capturable, max_grad_norm)

    def _kind(self, group):
        from stroke_prediction_amd.runtime import lib as L
        return L.CONSTS["SP_OPT_ADAM"]

    def _hyper(self, group):
        return (group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], self._max_norm(group), 0.0)

    @torch.no_grad()
    def step(self, closure=None):
        if self._clip_captured or any(g.get("max_grad_norm") is not None for g in self.param_groups):
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        O.bump_param_epoch()          # packed weight fragments cached by the conv runners are stale after this
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            st = self._flat_group(gi, group)
            if st is not None and self.capturable:
                from stroke_prediction_amd.runtime import lib as L
                # hyper-parameters live in device memory: while a hipGraph is being captured nothing is copied (a
                # captured copy would freeze today's values); ``push_hyper`` refreshes them before each replay
                if torch.cuda.is_current_stream_capturing():
                    self._clip_captured = False
                else:
                    self._push_hyper(st, group)
                st["step_dev"].add_(1)
                L.call("sp_adam_step_flat_hyp", O.ptr(st["p"]), O.ptr(st["g"]), O.ptr(st["m"]), O.ptr(st["v"]),
                       st["p"].numel(), O.ptr(st["lr_dev"]), O.ptr(st["step_dev"]), self.grad_scale, O.stream())
                continue
            if st is not None:
                step = int(self.state[group["params"][0]]["step"]) + 1
                O.adam_step_flat(st["p"], st["g"], st["m"], st["v"], group["lr"], b1, b2, group["eps"],
                                 group["weight_decay"], step, self.grad_scale)
                for p in group["params"]:
                    self.state[p]["step"] = step
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam runs on the GPU only")
                s = self.state[p]
                if "exp_avg" not in s:
                    s["step"] = 0
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                s["step"] = int(s["step"]) + 1
                O.adam_step_flat(p.data, p.grad.contiguous(), s["exp_avg"], s["exp_avg_sq"], group["lr"], b1, b2,
                                 group["eps"], group["weight_decay"], s["step"], self.grad_scale)
        return loss


class FusedAdamW(_FusedOptimizer):
    """``torch.optim.AdamW``: ``p *= 1 - lr * weight_decay``, then Adam without the L2 term (kind ADAMW); same state layout as Adam."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
                 capturable=False, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults, grad_scale, capturable, max_grad_norm)

    def _kind(self, group):
        from stroke_prediction_amd.runtime import lib as L
        return L.CONSTS["SP_OPT_ADAMW"]

    def _hyper(self, group):
        return (group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], self._max_norm(group), 0.0)


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` at dampening 0: ``g += wd * p; buf = momentum * buf + g; p -= lr * buf``, with ``nesterov``
    ``p -= lr * (g + momentum * buf)`` (kinds SGD / SGD_NESTEROV).  The buffer starts at zero, which is torch's first-step rule
    at dampening 0, and is kept as ``momentum_buffer`` per parameter.  ``nesterov`` picks the kernel, so a captured step keeps the
    one it was captured with; ``lr``, ``momentum``, ``weight_decay`` and ``max_grad_norm`` follow ``push_hyper``."""
    MOMENTS = ("momentum_buffer",)
    HAS_STEP = False

    def __init__(self, params, lr=1e-3, momentum=0, nesterov=False, weight_decay=0, dampening=0, grad_scale=1.0,
                 capturable=False, max_grad_norm=None):
        if dampening != 0:
            raise ValueError("FusedSGD has no dampening (got %r): the zero-initialised buffer equals torch's first step only at 0" % (dampening,))
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: negative lr, momentum or weight_decay")
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults, grad_scale, capturable, max_grad_norm)

    def _kind(self, group):
        from stroke_prediction_amd.runtime import lib as L
        return L.CONSTS["SP_OPT_SGD_NESTEROV" if group.get("nesterov") else "SP_OPT_SGD"]

    def _hyper(self, group):
        return (group["lr"], 0.0, 0.0, 0.0, group["weight_decay"], self._max_norm(group), group.get("momentum", 0.0))


def make_optimizer(args, params, hyper, graph=None, fusedadam=None):
    """The optimiser the command line asks for (common/util.py: ``--optimizer --lr --momentum --nesterov --weightdecay
    --clipnorm``).  ``hyper`` is the script's own Adam setting (lr, weight_decay, betas); ``graph`` / ``fusedadam`` default to the
    flags of those names and are passed by the scripts whose learner cannot replay a captured step or which never built a fused
    optimiser.  Without any of the new flags this builds what the scripts built before: ``torch.optim.Adam(params, **hyper)``,
    or ``FusedAdam(params, capturable=graph, **hyper)`` under ``--fusedadam`` / ``--graph``."""
    kind = getattr(args, "optimizer", "adam")
    graph = bool(getattr(args, "graph", False)) if graph is None else bool(graph)
    fused = bool(getattr(args, "fusedadam", False)) if fusedadam is None else bool(fusedadam)
    clip = getattr(args, "clipnorm", 0) or 0
    clip = float(clip) if clip > 0 else None
    hyper = dict(hyper)
    if getattr(args, "lr", None) is not None:
        hyper["lr"] = args.lr
    elif kind == "sgd":
        hyper["lr"] = 1e-2
    if getattr(args, "weightdecay", None) is not None:
        hyper["weight_decay"] = args.weightdecay
    if kind == "adam":
        if clip is not None:
            return FusedAdam(params, capturable=graph, max_grad_norm=clip, **hyper)
        if fused or graph:
            return FusedAdam(params, capturable=graph, **hyper)
        return torch.optim.Adam(params, **hyper)
    if kind == "adamw":
        return FusedAdamW(params, capturable=graph, max_grad_norm=clip, **hyper)
    if kind == "sgd":
        return FusedSGD(params, lr=hyper["lr"], momentum=getattr(args, "momentum", 0.99), nesterov=getattr(args, "nesterov", True),
                        weight_decay=hyper["weight_decay"], capturable=graph, max_grad_norm=clip)
    raise ValueError("unknown --optimizer %r" % (kind,))


def make_scheduler(args, optimizer):
    """``--lrschedule multistep``: ``MultiStepLR(--lrsteps)`` or none, as before; ``poly``: ``PolynomialLR`` over ``--epochs`` with
    ``--lrpower``.  Either is stepped by ``Learner.adapt_lr`` and reaches a captured step through ``push_hyper``."""
    if getattr(args, "lrschedule", "multistep") == "poly":
        return torch.optim.lr_scheduler.PolynomialLR(optimizer, total_iters=args.epochs, power=getattr(args, "lrpower", 0.9))
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, args.lrsteps) if args.lrsteps else None


def attach_flat_grads(model):
    """Point every ``p.grad`` of a FlatParamsMixin model at its slice of the flat gradient buffer (zeroed),
    so backward accumulates in place and the fused optimisers / the all-reduce see one contiguous operand."""
    model._ensure_flat()
    model._flat_grad.zero_()
    for (_, p), v in zip(model.named_parameters(), model._flat_views):
        p.grad = v
    return model._flat_grad
