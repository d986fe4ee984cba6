"""LayerNorm backed by the wave-per-row HIP kernel (csrc/kernels/layernorm.hip).

``LayerNorm`` subclasses ``torch.nn.LayerNorm`` (same state_dict). Parameters are kept in
fp32 while activations may be bf16; the kernel reads bf16 rows, normalises in fp32 and
writes bf16. Falls back to ``F.layer_norm`` for CPU tensors or unsupported widths.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ._native import native, use_native

_SUPPORTED_K = {1, 2, 3, 4, 5, 6, 8}


class _LNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd, _ = native().ln_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = native().ln_bwd(dy.contiguous(), x, weight, mean, rstd)
        return dx, dw, db, None


def layer_norm(x, normalized_shape, weight, bias, eps=1e-5):
    if _ln_native_ok(x, weight, bias, normalized_shape):
        return _LNFn.apply(x.contiguous(), weight, bias, float(eps))
    if weight is not None and x.dtype != weight.dtype:
        return F.layer_norm(x.float(), normalized_shape, weight.float(),
                            bias.float() if bias is not None else None, eps).to(x.dtype)
    return F.layer_norm(x, normalized_shape, weight, bias, eps)


class _AddLNFn(torch.autograd.Function):
    """(s, y) = (x + h, LayerNorm(x + h)) in one kernel; backward dx = dh = LN'(dy) + ds."""

    @staticmethod
    def forward(ctx, x, h, weight, bias, eps):
        y, mean, rstd, s = native().ln_fwd(x, weight, bias, eps, h)
        ctx.save_for_backward(s, weight, mean, rstd)
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, weight, mean, rstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        dres = ds.contiguous() if ds is not None else None
        dx, dw, db = native().ln_bwd(dy.contiguous(), s, weight, mean, rstd, dres)
        return dx, dx, dw, db, None


def _ln_native_ok(x, weight, bias, normalized_shape) -> bool:
    D = x.shape[-1]
    return (use_native(x) and weight is not None and bias is not None and len(normalized_shape) == 1
            and D % 256 == 0 and D // 256 in _SUPPORTED_K and x.dtype in (torch.float32, torch.bfloat16)
            and weight.dtype == torch.float32 and bias.dtype == torch.float32)


class _DropAddLNFn(torch.autograd.Function):
    """(s, y) = (x + dropout(h), LayerNorm(s)) in one kernel; backward dx = LN'(dy) + ds and
    dh = dropout'(dx) from one kernel too. The mask is regenerated from (ticket, stream) both ways
    (csrc/philox.h); bit for bit ``_AddLNFn`` on the separately dropped ``h``."""

    @staticmethod
    def forward(ctx, x, h, weight, bias, eps, ticket, stream, thr):
        y, mean, rstd, s = native().ln_fwd_drop(x, weight, bias, eps, h, ticket, stream, thr)
        ctx.save_for_backward(s, weight, mean, rstd, ticket)
        ctx.stream, ctx.thr = stream, thr
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, weight, mean, rstd, ticket = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        dres = ds.contiguous() if ds is not None else None
        dx, dh, dw, db = native().ln_bwd_drop(dy.contiguous(), s, weight, mean, rstd, dres, ticket, ctx.stream,
                                              ctx.thr)
        return dx, dh, dw, db, None, None, None, None


def add_layer_norm(x: torch.Tensor, h: torch.Tensor, ln: nn.LayerNorm, p: float = 0.0, ticket=None,
                   stream: int | None = None):
    """Pre-norm residual step: returns ``(s, ln(s))`` with ``s = x + h``. On the native path the
    add, the LayerNorm and (in backward) the two gradients of ``s`` are one kernel each way,
    instead of an add kernel + LayerNorm forward and LayerNorm backward + an add kernel.

    ``p > 0`` with a ``ticket`` (ops/dropout.py): ``s = x + dropout(h)`` — residual dropout inside
    the same kernels where the native path applies (no extra pass forward, one extra write of
    ``dh`` backward), else the elementwise dropout op followed by the ``p == 0`` path."""
    if p != 0.0 and ticket is not None:
        from .dropout import dropout, threshold
        thr = threshold(p)
        if ticket.tensor is not None and thr > 0:
            if stream is None:
                stream = ticket.next_stream()
            if (_ln_native_ok(x, ln.weight, ln.bias, ln.normalized_shape) and h.shape == x.shape
                    and h.dtype == x.dtype):
                return _DropAddLNFn.apply(x.contiguous(), h.contiguous(), ln.weight, ln.bias, float(ln.eps),
                                          ticket.tensor, int(stream), thr)
        h = dropout(h, p, ticket, stream)
    if (_ln_native_ok(x, ln.weight, ln.bias, ln.normalized_shape) and h.shape == x.shape
            and h.dtype == x.dtype):
        return _AddLNFn.apply(x.contiguous(), h.contiguous(), ln.weight, ln.bias, float(ln.eps))
    s = x + h
    return s, ln(s)


class LayerNorm(nn.LayerNorm):
    def forward(self, x):
        return layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
