"""SwiGLU on the packed gate/up GEMM output (csrc/kernels/swiglu.hip).

``swiglu(gu)`` for ``gu`` [..., 2F] returns ``silu(gu[..., :F]) * gu[..., F:]`` [..., F]: the gate and the
up projection come from ONE GEMM with a packed [2F, D] weight, and the [tokens, 2F] activation is read
once. The backward writes the packed gradient [dg | du] in one pass, recomputing the sigmoid from
``gu`` (nothing else is saved). CPU tensors, ``F % 8 != 0`` and ``PDT_DISABLE_NATIVE=1`` take the same
math in plain PyTorch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._native import native, use_native


def swiglu_reference(gu: torch.Tensor) -> torch.Tensor:
    g, u = gu.chunk(2, dim=-1)
    return F.silu(g) * u


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return native().swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        return native().swiglu_bwd(dy.contiguous(), gu)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    if (use_native(gu) and gu.dtype in (torch.float32, torch.bfloat16) and gu.shape[-1] % 16 == 0
            and gu.shape[-1] > 0):
        gu = gu.contiguous()  # a strided view is copied, never misread
        if gu.data_ptr() % 16 == 0:
            return _SwiGLUFn.apply(gu)
    return swiglu_reference(gu)
