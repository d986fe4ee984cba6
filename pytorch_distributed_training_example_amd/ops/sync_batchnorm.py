"""SyncBatchNorm: BatchNorm whose batch statistics span every rank of a process group, on the NHWC bf16
BatchNorm kernels (csrc/kernels/batchnorm.hip, the "SyncBatchNorm" section).

The local train forward / backward (ops/batchnorm.py) is split where the ranks' statistics meet:

    forward   reduce my rows -> (mean_r, M2_r, n_r)  | exchange |  merge (Chan, double, rank order)
              -> mean / invstd / (a, b) / running stats          |  apply y = relu?(a x + b + residual?)
    backward  reduce my rows -> (sum dz, sum dz (x - mean))      | exchange |  merge -> A, B, D (all ranks),
              dgamma / dbeta (my rows only: the data-parallel reducer averages them)  |  apply dx

**Exchange**: each rank writes its row into a zero-filled ``[W, .]`` fp32 buffer and the group all-reduces
(SUM) it. Adding zeros is exact, so every rank receives every rank's row bit for bit whatever order the
backend reduces in, and it needs nothing but all-reduce (gloo on GPU tensors, RCCL and the ``pdt_p2p``
backend all have it). One collective per direction per BatchNorm: ``(2C + 1) W`` floats forward,
``2C W`` backward. The merge sums in rank order, so mean, invstd, the running statistics and every
coefficient are identical bits on every rank. Per-rank batch sizes may differ (``n_r`` travels along).

Inputs the kernels do not take (CPU, fp32, NCHW) run a plain-PyTorch fp32 path with the same exchange and
the same formulas. In eval mode, with one rank, or without an initialised process group this is exactly
``batch_norm_act`` and no collective is issued.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist
from torch import nn

from ._native import native, use_native
from .batchnorm import batch_norm_act

CAPTURE_MSG = ("SyncBatchNorm under hipGraph capture with more than one rank is not supported yet: the "
               "statistics exchange is a collective inside the captured region")


def _exchange(buf: torch.Tensor, world: int, group) -> torch.Tensor:
    """``buf`` [W, K] fp32: zero but for this rank's row; returns it with every rank's row filled in."""
    if world > 1:
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf


def _dims(x: torch.Tensor):
    return tuple(d for d in range(x.dim()) if d != 1), (1, -1) + (1,) * (x.dim() - 2)


def merge_forward_reference(g: torch.Tensor, eps: float):
    """The forward merge in PyTorch ops (what bn_sync_merge_fwd_kernel computes): gathered ``g`` [W, 2C + 1]
    -> (mean fp64, biased var fp64, N fp64 scalar). Chan's formula in double, ranks in index order."""
    C = (g.shape[1] - 1) // 2
    gd = g.double()
    n, mr, m2r = gd[:, 2 * C], gd[:, :C], gd[:, C:2 * C]
    N = n.sum()
    mean = (n[:, None] * mr).sum(0) / N
    m2 = m2r.sum(0) + (n[:, None] * (mr - mean) ** 2).sum(0)
    return mean, m2 / N, N


class _SyncBNRefFn(torch.autograd.Function):
    """fp32 PyTorch path (CPU / fp32 / NCHW inputs): the same exchange and formulas as the kernels."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, momentum, eps, relu, group, world, rank):
        dims, sh = _dims(x)
        C = x.shape[1]
        n = x.numel() // C
        xd = x.double()
        mean_r = xd.mean(dims)
        m2_r = ((xd - mean_r.view(sh)) ** 2).sum(dims)
        buf = torch.zeros(world, 2 * C + 1, dtype=torch.float32, device=x.device)
        buf[rank, :C] = mean_r.float()
        buf[rank, C:2 * C] = m2_r.float()
        buf[rank, 2 * C] = float(n)
        g = _exchange(buf, world, group)
        if bool((g[:, 2 * C] < 1).any()):
            raise RuntimeError("SyncBatchNorm: a rank has zero rows in this batch (every rank must contribute "
                               "at least one sample)")
        mean_d, var_d, N = merge_forward_reference(g, eps)
        mean = mean_d.float()
        invstd = (1.0 / torch.sqrt(var_d + eps)).float()
        if running_mean is not None:
            running_mean.mul_(1.0 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
        if running_var is not None:
            unb = var_d * (N / (N - 1)) if float(N) > 1 else var_d
            running_var.mul_(1.0 - momentum).add_(unb.float().to(running_var.dtype), alpha=momentum)
        xf = x.float()
        gm = weight.float() if weight is not None else torch.ones_like(mean)
        a = gm * invstd
        b = (bias.float() if bias is not None else torch.zeros_like(mean)) - mean * a
        y = xf * a.view(sh) + b.view(sh)
        if residual is not None:
            y = y + residual.float()
        pos = None
        if relu:
            pos = y > 0
            y = y.clamp_min(0)
        ctx.relu, ctx.has_res, ctx.has_weight = relu, residual is not None, weight is not None
        ctx.group, ctx.world, ctx.rank, ctx.N = group, world, rank, float(N)
        ctx.save_for_backward(x, pos, weight, mean, invstd)
        ctx.mark_non_differentiable(mean, invstd)
        return y.to(x.dtype), mean, invstd

    @staticmethod
    def backward(ctx, dy, _dmean, _dinvstd):
        x, pos, weight, mean, invstd = ctx.saved_tensors
        dims, sh = _dims(x)
        C = x.shape[1]
        dz = dy.float()
        if ctx.relu:
            dz = dz * pos
        xc = x.float() - mean.view(sh)
        buf = torch.zeros(ctx.world, 2 * C, dtype=torch.float32, device=x.device)
        buf[ctx.rank, :C] = dz.sum(dims, dtype=torch.float64).float()
        buf[ctx.rank, C:] = (dz.double() * xc.double()).sum(dims).float()
        g = _exchange(buf, ctx.world, ctx.group)
        tot = g.double().sum(0).float()  # rank order
        S1, S2 = tot[:C], tot[C:]
        gm = weight.float() if weight is not None else torch.ones_like(mean)
        A = gm * invstd
        B = -gm * invstd * invstd * (S2 * invstd) / ctx.N
        D = -gm * invstd * S1 / ctx.N
        dx = (A.view(sh) * dz + B.view(sh) * xc + D.view(sh)).to(x.dtype)
        need_w = ctx.has_weight and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        dg = (g[ctx.rank, C:] * invstd).to(weight.dtype) if need_w else None
        db = g[ctx.rank, :C].to(weight.dtype) if need_w else None
        dres = dz.to(dy.dtype) if ctx.has_res else None
        return (dx, dres, dg, db) + (None,) * 8


class _SyncBNFn(torch.autograd.Function):
    """Native path: NHWC bf16 on the GPU, C % 64 == 0."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, momentum, eps, relu, group, world, rank):
        C_ = native()
        C = x.shape[1]
        buf = torch.zeros(world, 2 * C + 1, dtype=torch.float32, device=x.device)
        C_.bn_sync_fwd_stats(x, buf[rank])  # (mean_r, M2_r, n_r) straight into this rank's row
        g = _exchange(buf, world, group)
        mean, invstd, ab, ntot = C_.bn_sync_fwd_merge(g, weight, bias, running_mean, running_var, momentum, eps)
        y, mask = C_.bn_apply_coef(x, residual, ab, relu)
        ctx.relu, ctx.has_res, ctx.has_weight = relu, residual is not None, weight is not None
        ctx.group, ctx.world, ctx.rank = group, world, rank
        # backward needs the BN input and a 1-bit ReLU mask, never the output y
        ctx.save_for_backward(x, mask if relu else None, weight, mean, invstd, ntot)
        ctx.mark_non_differentiable(mean, invstd)
        return y, mean, invstd

    @staticmethod
    def backward(ctx, dy, _dmean, _dinvstd):
        C_ = native()
        x, mask, weight, mean, invstd, ntot = ctx.saved_tensors
        C = x.shape[1]
        fmt = torch.channels_last if x.dim() == 4 else torch.contiguous_format
        dy = dy.contiguous(memory_format=fmt)
        buf = torch.zeros(ctx.world, 2 * C, dtype=torch.float32, device=x.device)
        C_.bn_sync_bwd_sums(dy, x, mask, mean, ctx.relu, buf[ctx.rank])
        g = _exchange(buf, ctx.world, ctx.group)
        need_w = ctx.has_weight and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        coef, dg, db = C_.bn_sync_bwd_merge(g, ctx.rank, weight, invstd, ntot, need_w)
        dx, dres = C_.bn_bwd_apply_coef(dy, x, mask, mean, coef, ctx.relu, ctx.has_res)
        return (dx, dres if ctx.has_res else None, dg if need_w else None, db if need_w else None) + (None,) * 8


def _group_world(group) -> int:
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def sync_batch_norm_act(x, residual, weight, bias, running_mean, running_var, training, momentum, eps, relu,
                        group=None, _force_sync: bool = False, _return_stats: bool = False):
    """Functional ``relu?(batchnorm(x) + residual?)`` with the batch statistics taken over every rank of
    ``group`` (None: the default group). Eval mode, one rank or no process group: ``batch_norm_act``,
    no collective. ``_force_sync`` (private: single-process kernel tests and timing) runs the full
    split path with W = 1; ``_return_stats`` (private) also returns the merged (mean, invstd)."""
    world = _group_world(group) if training else 1
    if not training or (world == 1 and not _force_sync):
        assert not _return_stats, "merged statistics exist on the sync path only"
        return batch_norm_act(x, residual, weight, bias, running_mean, running_var, training, momentum, eps, relu)
    rank = dist.get_rank(group) if world > 1 else 0
    if x.numel() == 0:
        raise RuntimeError("SyncBatchNorm: this rank has zero rows in this batch (every rank must contribute "
                           "at least one sample)")
    nhwc = (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)) or (x.dim() == 2 and x.is_contiguous())
    native_ok = (use_native(x) and x.dtype == torch.bfloat16 and nhwc and x.shape[1] % 64 == 0
                 and (residual is None or (residual.shape == x.shape and residual.dtype == x.dtype)))
    if native_ok:
        if world > 1 and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(CAPTURE_MSG)
        if residual is not None:
            residual = residual.contiguous(memory_format=torch.channels_last if x.dim() == 4
                                           else torch.contiguous_format)
        fn = _SyncBNFn
    else:
        fn = _SyncBNRefFn
    y, mean, invstd = fn.apply(x, residual, weight, bias, running_mean, running_var, float(momentum), float(eps),
                               bool(relu), group, world, rank)
    return (y, mean, invstd) if _return_stats else y


class SyncBatchNorm(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` whose training statistics span ``process_group`` (same parameters, buffers and
    state_dict keys), with the fused ReLU / residual of ``ops.batchnorm.BatchNorm2d``:
    ``forward(x, residual=None, relu=None)``. Deliberately NOT a subclass of our ``BatchNorm2d``: the ResNet
    blocks' linked / deferred paths test for that class and so take their plain path for this module."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True,
                 fused_relu: bool = False, process_group=None, device=None, dtype=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device, dtype)
        self.fused_relu = fused_relu
        self.process_group = process_group
        self._nbt = 0  # host-side num_batches_tracked (synced into the buffer on save)

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                relu: Optional[bool] = None) -> torch.Tensor:
        relu = self.fused_relu if relu is None else relu
        training = self.training or not self.track_running_stats
        momentum = self.momentum
        if self.training and self.track_running_stats:
            self._nbt += 1
            if momentum is None:  # cumulative moving average
                momentum = 1.0 / float(self._nbt + int(self.num_batches_tracked.item()))
        rm = self.running_mean if (not self.training or self.track_running_stats) else None
        rv = self.running_var if (not self.training or self.track_running_stats) else None
        w = self.weight if self.affine else None
        b = self.bias if self.affine else None
        return sync_batch_norm_act(x, residual, w, b, rm, rv, training, momentum if momentum is not None else 0.0,
                                   self.eps, relu, self.process_group)

    def sync_num_batches_tracked(self) -> None:
        if self.track_running_stats and self._nbt:
            self.num_batches_tracked.add_(self._nbt)
            self._nbt = 0

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.sync_num_batches_tracked()
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kwargs):
        self._nbt = 0
        super()._load_from_state_dict(*args, **kwargs)


def convert_sync_batchnorm(module: nn.Module, process_group=None) -> nn.Module:
    """Replace every ``nn.BatchNorm2d`` (ours and torch's) under ``module`` by a ``SyncBatchNorm`` holding the
    SAME ``Parameter`` objects and buffers (an existing optimizer or DDP wrapper still sees them), and the same
    ``fused_relu``, ``eps``, ``momentum``, ``affine``, ``track_running_stats`` and training flag. Returns the
    converted module (a new object only when ``module`` itself is a BatchNorm)."""
    if isinstance(module, SyncBatchNorm):
        return module
    if isinstance(module, nn.BatchNorm2d):
        new = SyncBatchNorm(module.num_features, module.eps, module.momentum, module.affine,
                            module.track_running_stats, fused_relu=getattr(module, "fused_relu", False),
                            process_group=process_group, device="meta")
        for name in ("weight", "bias"):
            new._parameters[name] = module._parameters[name]
        for name in ("running_mean", "running_var", "num_batches_tracked"):
            new._buffers[name] = module._buffers[name]
        new.training = module.training
        new._nbt = getattr(module, "_nbt", 0)  # batches counted on the host, not yet in the buffer
        return new
    for name, child in module.named_children():
        new = convert_sync_batchnorm(child, process_group)
        if new is not child:
            setattr(module, name, new)
    return module
