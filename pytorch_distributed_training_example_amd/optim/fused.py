"""Fused multi-tensor optimizers: SGD, Adam/AdamW, Adadelta (csrc/kernels/optim.hip), and the layer-wise
adaptive LARS / LAMB (csrc/kernels/layerwise.hip; math contract above ``FusedLARS`` below).

Reference parity: the reference trains with ``torch.optim.Adadelta(lr=args.lr)`` + ``StepLR``
(/root/reference/train.py:99,101). These classes are drop-in ``torch.optim.Optimizer``s with the
same hyper-parameters, the same update math and the same per-parameter state keys
(``momentum_buffer``; ``step``/``exp_avg``/``exp_avg_sq``; ``step``/``square_avg``/``acc_delta``)
so torch optimizer checkpoints load into them and vice versa.

MI355X-first differences:
  * one kernel per (param dtype, grad dtype) group and ≤320 chunks of 32 Ki elements —
    param, grad and state are read once and written once;
  * ``master_weights=True``: bf16 parameters get an fp32 master copy in
    ``state['master_param']``; the kernel updates the master and writes the bf16 parameter
    in the same pass (no separate cast kernel, no autocast weight casts in forward);
  * lr (and Adam's step) live in device tensors, so a hipGraph-captured step replays with
    the current schedule value (``sync_lr()`` refreshes them outside the graph);
  * AMP: ``step(inv_scale=..., found_inf=...)`` unscales in-kernel and skips the update on
    device when an overflow was found — no host readback.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
from torch.optim import Optimizer

from ..ops._native import cuda_available, native, use_native


def _capturing() -> bool:
    return cuda_available() and torch.cuda.is_current_stream_capturing()


class _FusedOptimizer(Optimizer):
    _state_keys: Tuple[str, ...] = ()

    def __init__(self, params, defaults, master_weights: bool = True):
        super().__init__(params, defaults)
        self.master_weights = master_weights
        self._lr_dev: Dict[int, torch.Tensor] = {}
        self._lr_host: Dict[int, float] = {}

    # -- helpers -------------------------------------------------------------
    def _lr_tensor(self, gi: int, group: dict, device: torch.device) -> torch.Tensor:
        t = self._lr_dev.get(gi)
        lr = float(group["lr"])
        if t is None or t.device != device:
            t = torch.full((1,), lr, dtype=torch.float32, device=device)
            self._lr_dev[gi] = t
            self._lr_host[gi] = lr
        elif not _capturing() and self._lr_host.get(gi) != lr:
            t.fill_(lr)
            self._lr_host[gi] = lr
        return t

    def sync_lr(self) -> None:
        """Push host-side ``group['lr']`` into the device lr tensors (call outside graph replay)."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._lr_dev and self._lr_host.get(gi) != float(group["lr"]):
                self._lr_dev[gi].fill_(float(group["lr"]))
                self._lr_host[gi] = float(group["lr"])

    def _master(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        if not (self.master_weights and p.dtype in (torch.bfloat16, torch.float16)):
            return None
        st = self.state[p]
        m = st.get("master_param")
        if m is None:
            m = torch.empty_like(p, dtype=torch.float32)
            m.copy_(p.detach())
            st["master_param"] = m
        return m

    def _buckets(self, group) -> Dict[tuple, List[torch.Tensor]]:
        out: Dict[tuple, List[torch.Tensor]] = {}
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("fused optimizers do not support sparse gradients")
            m = self._master(p)
            key = ((m if m is not None else p).dtype, p.grad.dtype, m is not None, p.device)
            out.setdefault(key, []).append(p)
        return out

    @torch.no_grad()
    def step(self, closure=None, inv_scale: Optional[torch.Tensor] = None,
             found_inf: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            for key, ps in self._buckets(group).items():
                self._init_state(group, ps)
                masters = [self.state[p]["master_param"] for p in ps] if key[2] else []
                kparams = masters if key[2] else ps
                copies = ps if key[2] else []
                grads = [p.grad for p in ps]
                if use_native(*kparams):
                    self._native_step(gi, group, ps, kparams, grads, copies, inv_scale, found_inf)
                else:
                    if found_inf is not None and float(found_inf.item()) != 0.0:
                        continue
                    if inv_scale is not None:
                        grads = [g * inv_scale.to(g.dtype) for g in grads]
                    self._ref_step(group, ps, kparams, grads)
                    for p, m in zip(copies, masters):
                        p.copy_(m)
        return loss

    def _init_state(self, group, ps):
        raise NotImplementedError

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        raise NotImplementedError

    def _ref_step(self, group, ps, kparams, grads):
        raise NotImplementedError


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` semantics (momentum, dampening, nesterov, weight_decay, maximize)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, maximize: bool = False,
                 master_weights: bool = True):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov, maximize=maximize),
                         master_weights)

    def _init_state(self, group, ps):
        if group["momentum"] == 0:
            return
        for p in ps:
            st = self.state[p]
            if st.get("momentum_buffer") is None:
                ref = st.get("master_param", p)
                st["momentum_buffer"] = torch.zeros_like(ref, dtype=torch.float32)
                st["_first"] = True

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        bufs = [self.state[p]["momentum_buffer"] for p in ps] if group["momentum"] != 0 else []
        first = bool(bufs) and bool(self.state[ps[0]].get("_first", False))
        native().sgd(kparams, grads, bufs, copies, float(group["lr"]),
                     self._lr_tensor(gi, group, kparams[0].device), float(group["momentum"]),
                     float(group["dampening"]), float(group["weight_decay"]), bool(group["nesterov"]),
                     first, bool(group["maximize"]), inv_scale, found_inf)
        for p in ps:
            self.state[p]["_first"] = False

    def _ref_step(self, group, ps, kparams, grads):
        for p, kp, g in zip(ps, kparams, grads):
            g = g.float()
            if group["maximize"]:
                g = -g
            if group["weight_decay"]:
                g = g + group["weight_decay"] * kp.float()
            if group["momentum"]:
                st = self.state[p]
                b = st["momentum_buffer"]
                if st.get("_first", False):
                    b.copy_(g)
                    st["_first"] = False
                else:
                    b.mul_(group["momentum"]).add_(g, alpha=1 - group["dampening"])
                g = g + group["momentum"] * b if group["nesterov"] else b
            kp.add_(g.to(kp.dtype), alpha=-group["lr"])

    def state_dict(self):
        sd = super().state_dict()
        for st in sd["state"].values():
            st.pop("_first", None)
        return sd


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` / ``AdamW`` semantics (``adam_w_mode`` selects decoupled decay)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False, maximize: bool = False,
                 adam_w_mode: bool = False, master_weights: bool = True):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported by the fused kernel")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      maximize=maximize, adam_w_mode=adam_w_mode), master_weights)
        self._step_dev: Dict[int, torch.Tensor] = {}

    def _init_state(self, group, ps):
        shared = None
        for p in ps:
            st = self.state[p]
            if "exp_avg" not in st:
                ref = st.get("master_param", p)
                st["exp_avg"] = torch.zeros_like(ref, dtype=torch.float32)
                st["exp_avg_sq"] = torch.zeros_like(ref, dtype=torch.float32)
                if shared is None:
                    shared = torch.zeros((), dtype=torch.float32, device=p.device)
                st["step"] = shared

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        # every param of the group shares one device step counter (equal by construction)
        step_t = self.state[ps[0]]["step"]
        if step_t.device != kparams[0].device:
            step_t = step_t.to(kparams[0].device)
            self.state[ps[0]]["step"] = step_t
        if found_inf is None:
            step_t.add_(1)
        else:
            step_t.add_((found_inf.reshape(()) == 0).to(step_t.dtype))
        for p in ps[1:]:
            if self.state[p]["step"] is not step_t:  # e.g. after load_state_dict: alias once
                self.state[p]["step"] = step_t
        b1, b2 = group["betas"]
        native().adam(kparams, grads, [self.state[p]["exp_avg"] for p in ps],
                      [self.state[p]["exp_avg_sq"] for p in ps], copies, float(group["lr"]),
                      self._lr_tensor(gi, group, kparams[0].device), float(b1), float(b2), float(group["eps"]),
                      float(group["weight_decay"]), bool(group["adam_w_mode"]), step_t.reshape(1), 0.0,
                      bool(group["maximize"]), inv_scale, found_inf)

    def _ref_step(self, group, ps, kparams, grads):
        b1, b2 = group["betas"]
        bumped = set()
        for p, kp, g in zip(ps, kparams, grads):
            st = self.state[p]
            if id(st["step"]) not in bumped:  # step tensors may be shared across the group
                st["step"] += 1
                bumped.add(id(st["step"]))
            t = float(st["step"])
            g = g.float()
            if group["maximize"]:
                g = -g
            lr, wd = group["lr"], group["weight_decay"]
            if group["adam_w_mode"]:
                kp.mul_(1 - lr * wd)
            elif wd:
                g = g + wd * kp.float()
            st["exp_avg"].lerp_(g, 1 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            denom = (st["exp_avg_sq"].sqrt() / math.sqrt(bc2)).add_(group["eps"])
            kp.addcdiv_(st["exp_avg"], denom, value=-lr / bc1)


class FusedAdamW(FusedAdam):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, maximize: bool = False,
                 master_weights: bool = True):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize, adam_w_mode=True,
                         master_weights=master_weights)


class FusedAdadelta(_FusedOptimizer):
    """``torch.optim.Adadelta`` semantics — the reference's optimizer (train.py:99)."""

    def __init__(self, params, lr: float = 1.0, rho: float = 0.9, eps: float = 1e-6,
                 weight_decay: float = 0.0, maximize: bool = False, master_weights: bool = True):
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, maximize=maximize),
                         master_weights)

    def _init_state(self, group, ps):
        for p in ps:
            st = self.state[p]
            if "square_avg" not in st:
                ref = st.get("master_param", p)
                st["step"] = torch.zeros((), dtype=torch.float32)
                st["square_avg"] = torch.zeros_like(ref, dtype=torch.float32)
                st["acc_delta"] = torch.zeros_like(ref, dtype=torch.float32)

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        if not _capturing():
            for p in ps:
                self.state[p]["step"] += 1
        native().adadelta(kparams, grads, [self.state[p]["square_avg"] for p in ps],
                          [self.state[p]["acc_delta"] for p in ps], copies, float(group["lr"]),
                          self._lr_tensor(gi, group, kparams[0].device), float(group["rho"]), float(group["eps"]),
                          float(group["weight_decay"]), bool(group["maximize"]), inv_scale, found_inf)

    def _ref_step(self, group, ps, kparams, grads):
        rho, eps, lr, wd = group["rho"], group["eps"], group["lr"], group["weight_decay"]
        for p, kp, g in zip(ps, kparams, grads):
            st = self.state[p]
            st["step"] += 1
            g = g.float()
            if group["maximize"]:
                g = -g
            if wd:
                g = g + wd * kp.float()
            sa, ad = st["square_avg"], st["acc_delta"]
            sa.mul_(rho).addcmul_(g, g, value=1 - rho)
            std = sa.add(eps).sqrt_()
            delta = ad.add(eps).sqrt_().div_(std).mul_(g)
            ad.mul_(rho).addcmul_(delta, delta, value=1 - rho)
            kp.add_(delta, alpha=-lr)


# ----------------------------------------------------------------------------- LARS / LAMB
# Layer-wise adaptive optimizers (csrc/kernels/layerwise.hip). The contract below is what the kernels,
# the CPU path (_ref_step) and the tests compute.
#
# All arithmetic is fp32, on the fp32 master copy when there is one and on the parameter itself
# otherwise. g is the gradient after the optional AMP inv_scale and the maximize sign. ||.|| is the L2
# norm over ONE parameter tensor: fp32 squares summed in a fixed order, the last stage in double.
# `adapt` is a per-param-group flag (default True); with adapt=False the ratio r is 1.
#
#   FusedLARS    wn = ||w||, gn = ||g||
#                r  = trust_coefficient * wn / (gn + weight_decay * wn + eps)  if adapt and wn > 0 and gn > 0 else 1
#                d  = r * (g + weight_decay * w)
#                buf = d on the group's first step, else momentum * buf + (1 - dampening) * d   (momentum != 0)
#                w -= lr * (d + momentum * buf if nesterov else buf if momentum != 0 else d)
#              = torch.optim.SGD(weight_decay=0) applied to the pre-scaled gradient d (the LARC "scale" form).
#
#   FusedLAMB    m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  t = step after increment
#                u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay * w
#                r = ||w|| / ||u||  if adapt and ||w|| > 0 and ||u|| > 0 else 1
#                w -= lr * r * u
#
# Nothing is read on the host and nothing is allocated per step: the norm scratch (per-chunk partials,
# per-tensor sums and ratios) belongs to the optimizer and is allocated on the first step of each
# (group, dtype) bucket, before any graph capture. On a found-inf step weights, states and the step
# counter keep their bits. Zero-element parameters have nothing to update and are left out of the step.


def _sumsq(x: torch.Tensor) -> torch.Tensor:
    return x.detach().double().pow(2).sum()


class _LayerwiseScratch:
    """partials fp32 [2 * chunks], sums fp64 [n, 2], ratio fp32 [n]; slot t belongs to the bucket's t-th tensor."""

    def __init__(self, kparams: List[torch.Tensor]):
        dev = kparams[0].device
        self.sig = tuple(int(p.numel()) for p in kparams)
        self.partials = torch.empty(2 * int(native().layerwise_chunks(kparams)), dtype=torch.float32, device=dev)
        self.sums = torch.zeros(len(kparams), 2, dtype=torch.float64, device=dev)
        self.ratio = torch.ones(len(kparams), dtype=torch.float32, device=dev)


class _LayerwiseMixin:
    def _buckets(self, group):
        out = super()._buckets(group)
        # a zero-element tensor has no chunk, hence no trust-ratio slot in the kernels, and nothing to update
        return {k: [p for p in ps if p.numel() > 0] for k, ps in out.items() if any(p.numel() > 0 for p in ps)}

    def _scratch_for(self, gi: int, kparams, grads, copies) -> _LayerwiseScratch:
        key = (gi, kparams[0].dtype, grads[0].dtype, bool(copies), kparams[0].device)
        sig = tuple(int(p.numel()) for p in kparams)
        sc = self._scratch.get(key)
        if sc is None or sc.sig != sig:
            if _capturing():
                raise RuntimeError("layer-wise optimizer scratch must exist before graph capture: run one eager "
                                   "step with the same set of gradients first")
            sc = self._scratch[key] = _LayerwiseScratch(kparams)
        return sc

    def load_state_dict(self, state_dict):
        """torch casts every floating-point state tensor to its parameter's dtype, which would round the
        fp32 master copy and moments of a bf16 parameter to bf16: put those back from the saved values."""
        super().load_state_dict(state_dict)
        saved = [i for g in state_dict["param_groups"] for i in g["params"]]
        mine = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(saved, mine):
            for k, v in state_dict["state"].get(i, {}).items():
                if k != "step" and torch.is_tensor(v) and v.dtype == torch.float32 and p.dtype != torch.float32:
                    self.state[p][k] = v.detach().to(device=p.device, dtype=torch.float32, copy=True)

    def trust_ratios(self) -> Dict[torch.Tensor, torch.Tensor]:
        """{parameter: its last trust ratio (a 0-d view into the device scratch)} for the adapted groups
        that have stepped on the GPU."""
        out = {}
        for gi, group in enumerate(self.param_groups):
            if not group["adapt"]:
                continue
            for key, ps in self._buckets(group).items():
                sc = self._scratch.get((gi, key[0], key[1], key[2], key[3]))
                if sc is not None and len(ps) == len(sc.sig):
                    out.update({p: sc.ratio[i] for i, p in enumerate(ps)})
        return out


class FusedLARS(_LayerwiseMixin, FusedSGD):
    """LARS (You et al. 2017) in the LARC "scale" form: momentum SGD on the trust-ratio-scaled gradient.
    State is ``momentum_buffer`` as in ``FusedSGD``. Math contract: the comment block above."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.9, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, trust_coefficient: float = 0.001,
                 eps: float = 1e-8, adapt: bool = True, maximize: bool = False, master_weights: bool = True):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        _FusedOptimizer.__init__(self, params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                                    weight_decay=weight_decay, nesterov=nesterov,
                                                    trust_coefficient=trust_coefficient, eps=eps, adapt=adapt,
                                                    maximize=maximize), master_weights)
        self._scratch: Dict[tuple, _LayerwiseScratch] = {}

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        if not group["adapt"]:  # r = 1: d = g + wd * w, which is FusedSGD's step
            return FusedSGD._native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf)
        bufs = [self.state[p]["momentum_buffer"] for p in ps] if group["momentum"] != 0 else []
        first = bool(bufs) and bool(self.state[ps[0]].get("_first", False))
        sc = self._scratch_for(gi, kparams, grads, copies)
        native().lars(kparams, grads, bufs, copies, float(group["lr"]),
                      self._lr_tensor(gi, group, kparams[0].device), float(group["momentum"]),
                      float(group["dampening"]), float(group["weight_decay"]), bool(group["nesterov"]), first,
                      float(group["trust_coefficient"]), float(group["eps"]), bool(group["maximize"]), inv_scale,
                      found_inf, sc.partials, sc.sums, sc.ratio, False)
        for p in ps:
            self.state[p]["_first"] = False

    def _ref_step(self, group, ps, kparams, grads):
        wd, mom = group["weight_decay"], group["momentum"]
        for p, kp, g in zip(ps, kparams, grads):
            g = g.float()
            if group["maximize"]:
                g = -g
            w = kp.float()
            r = 1.0
            if group["adapt"]:
                wn, gn = _sumsq(w).sqrt(), _sumsq(g).sqrt()
                if wn > 0 and gn > 0:
                    r = float((group["trust_coefficient"] * wn / (gn + wd * wn + group["eps"])).float())
            d = (g + wd * w) * r
            if mom:
                st = self.state[p]
                b = st["momentum_buffer"]
                if st.get("_first", False):
                    b.copy_(d)
                    st["_first"] = False
                else:
                    b.mul_(mom).add_(d, alpha=1 - group["dampening"])
                d = d + mom * b if group["nesterov"] else b
            kp.add_(d.to(kp.dtype), alpha=-group["lr"])


class FusedLAMB(_LayerwiseMixin, FusedAdam):
    """LAMB (You et al. 2019). State is ``step`` / ``exp_avg`` / ``exp_avg_sq`` as in ``FusedAdam``; the
    group shares one device step counter and a found-inf step does not advance it. Math contract: the
    comment block above."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, adapt: bool = True, maximize: bool = False,
                 master_weights: bool = True):
        _FusedOptimizer.__init__(self, params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                                    adapt=adapt, maximize=maximize), master_weights)
        self._step_dev: Dict[int, torch.Tensor] = {}
        self._scratch: Dict[tuple, _LayerwiseScratch] = {}

    def _bump_step(self, ps, device, found_inf) -> torch.Tensor:
        # one device step counter per bucket, advanced on device (FusedAdam._native_step)
        step_t = self.state[ps[0]]["step"]
        if step_t.device != device:
            step_t = step_t.to(device)
            self.state[ps[0]]["step"] = step_t
        if found_inf is None:
            step_t.add_(1)
        else:
            step_t.add_((found_inf.reshape(()) == 0).to(step_t.dtype))
        for p in ps[1:]:
            if self.state[p]["step"] is not step_t:  # e.g. after load_state_dict: alias once
                self.state[p]["step"] = step_t
        return step_t

    def _native_step(self, gi, group, ps, kparams, grads, copies, inv_scale, found_inf):
        step_t = self._bump_step(ps, kparams[0].device, found_inf)
        sc = self._scratch_for(gi, kparams, grads, copies) if group["adapt"] else None
        b1, b2 = group["betas"]
        native().lamb(kparams, grads, [self.state[p]["exp_avg"] for p in ps],
                      [self.state[p]["exp_avg_sq"] for p in ps], copies, float(group["lr"]),
                      self._lr_tensor(gi, group, kparams[0].device), float(b1), float(b2), float(group["eps"]),
                      float(group["weight_decay"]), step_t.reshape(1), 0.0, bool(group["maximize"]), inv_scale,
                      found_inf, sc.partials if sc else None, sc.sums if sc else None, sc.ratio if sc else None,
                      False)

    def _ref_step(self, group, ps, kparams, grads):
        b1, b2 = group["betas"]
        lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
        bumped = set()
        for p, kp, g in zip(ps, kparams, grads):
            st = self.state[p]
            if id(st["step"]) not in bumped:  # step tensors may be shared across the group
                st["step"] += 1
                bumped.add(id(st["step"]))
            t = float(st["step"])
            g = g.float()
            if group["maximize"]:
                g = -g
            w = kp.float()
            st["exp_avg"].lerp_(g, 1 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (st["exp_avg"] / (1 - b1 ** t)) / ((st["exp_avg_sq"] / (1 - b2 ** t)).sqrt_().add_(eps))
            if wd:
                u = u + wd * w
            r = 1.0
            if group["adapt"]:
                wn, un = _sumsq(w).sqrt(), _sumsq(u).sqrt()
                if wn > 0 and un > 0:
                    r = float((wn / un).float())
            kp.add_(u.to(kp.dtype), alpha=-lr * r)


def layerwise_param_groups(module_or_named_params, weight_decay: float, skip_1d: bool = True) -> List[dict]:
    """The usual two groups for LARS / LAMB from a module or an iterable of ``(name, parameter)``:
    parameters with ``ndim >= 2`` get ``weight_decay`` and ``adapt=True``; parameters with ``ndim <= 1``
    (BatchNorm and LayerNorm scales, all biases) get ``weight_decay=0`` and ``adapt=False``.
    ``skip_1d=False`` puts every parameter in the first group. Frozen parameters are left out."""
    named = (module_or_named_params.named_parameters() if hasattr(module_or_named_params, "named_parameters")
             else module_or_named_params)
    adapted, plain = [], []
    for _, p in named:
        if not p.requires_grad:
            continue
        (plain if skip_1d and p.ndim <= 1 else adapted).append(p)
    groups = [dict(params=adapted, weight_decay=weight_decay, adapt=True)]
    if plain:
        groups.append(dict(params=plain, weight_decay=0.0, adapt=False))
    return groups


def build_optimizer(name: str, params, lr: float, **kw) -> Optimizer:
    name = name.lower()
    if name == "lars":
        return FusedLARS(params, lr=lr, **kw)
    if name == "lamb":
        return FusedLAMB(params, lr=lr, **kw)
    if name == "sgd":
        return FusedSGD(params, lr=lr, **kw)
    if name == "adamw":
        return FusedAdamW(params, lr=lr, **kw)
    if name == "adam":
        return FusedAdam(params, lr=lr, **kw)
    if name == "adadelta":
        return FusedAdadelta(params, lr=lr, **kw)
    raise ValueError(f"unknown optimizer {name}")
