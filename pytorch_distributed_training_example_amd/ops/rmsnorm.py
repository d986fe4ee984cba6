"""RMSNorm backed by the wave-per-row HIP kernel (csrc/kernels/rmsnorm.hip).

``y = x * rsqrt(mean(x^2) + eps) * weight``: no mean, no bias. ``RMSNorm`` subclasses
``torch.nn.RMSNorm`` (same state_dict: one key, ``weight``). The weight is kept in fp32 while
activations may be bf16; the kernel reads bf16 rows, normalises in fp32 and writes bf16.
CPU tensors, unsupported widths and ``PDT_DISABLE_NATIVE=1`` take the same math in plain PyTorch.
"""
from __future__ import annotations

import torch
from torch import nn

from ._native import native, use_native

_SUPPORTED_K = {1, 2, 3, 4, 5, 6, 8}


def rms_norm_reference(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """fp32 math, one rounding to ``x``'s dtype: what the kernel computes."""
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd * weight.float()).to(x.dtype)


def _rms_native_ok(x, weight) -> bool:
    D = x.shape[-1]
    return (use_native(x) and weight is not None and weight.dim() == 1 and weight.shape[0] == D
            and D % 256 == 0 and D // 256 in _SUPPORTED_K and x.dtype in (torch.float32, torch.bfloat16)
            and weight.dtype == torch.float32)


class _RMSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        y, rstd, _ = native().rms_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dx, dw = native().rms_bwd(dy.contiguous(), x, weight, rstd)
        return dx, dw, None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if _rms_native_ok(x, weight):
        return _RMSFn.apply(x.contiguous(), weight, float(eps))
    return rms_norm_reference(x, weight, eps)


class _AddRMSFn(torch.autograd.Function):
    """(s, y) = (x + h, RMSNorm(x + h)) in one kernel; backward dx = dh = RMS'(dy) + ds."""

    @staticmethod
    def forward(ctx, x, h, weight, eps):
        y, rstd, s = native().rms_fwd(x, weight, eps, h)
        ctx.save_for_backward(s, weight, rstd)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, weight, rstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        dres = ds.contiguous() if ds is not None else None
        dx, dw = native().rms_bwd(dy.contiguous(), s, weight, rstd, dres)
        return dx, dx, dw, None


def add_rms_norm(x: torch.Tensor, h: torch.Tensor, norm: "RMSNorm"):
    """Pre-norm residual step: returns ``(s, norm(s))`` with ``s = x + h``. On the native path the add,
    the RMSNorm and (in backward) the two gradients of ``s`` are one kernel each way, as
    ``add_layer_norm`` does for LayerNorm."""
    if _rms_native_ok(x, norm.weight) and h.shape == x.shape and h.dtype == x.dtype:
        return _AddRMSFn.apply(x.contiguous(), h.contiguous(), norm.weight, float(norm.eps))
    s = x + h
    return s, norm(s)


_Base = getattr(nn, "RMSNorm", None)

if _Base is not None:
    class RMSNorm(_Base):
        """``torch.nn.RMSNorm`` (same ``weight`` key, so checkpoints interchange) on :func:`rms_norm`."""

        def __init__(self, normalized_shape, eps: float = 1e-5, device=None, dtype=None):
            super().__init__(normalized_shape, eps=eps, elementwise_affine=True, device=device, dtype=dtype)
            assert len(self.normalized_shape) == 1, "RMSNorm: one normalised dimension"

        def forward(self, x):
            return rms_norm(x, self.weight, self.eps)
else:  # pragma: no cover - torch without nn.RMSNorm
    class RMSNorm(nn.Module):
        def __init__(self, normalized_shape, eps: float = 1e-5, device=None, dtype=None):
            super().__init__()
            if isinstance(normalized_shape, int):
                normalized_shape = (normalized_shape,)
            self.normalized_shape = tuple(normalized_shape)
            assert len(self.normalized_shape) == 1, "RMSNorm: one normalised dimension"
            self.eps = eps
            self.weight = nn.Parameter(torch.ones(self.normalized_shape, device=device, dtype=dtype))

        def forward(self, x):
            return rms_norm(x, self.weight, self.eps)
