"""Scaled-dot-product attention backed by the flash-attention HIP kernels (csrc/kernels/attention.hip).

``attention_qkv(qkv, heads, causal)`` takes the packed QKV projection output [B, T, 3·H·Dh]
(bf16, the c_attn GEMM result) and returns [B, T, H·Dh] ready for the output projection:
the kernels read Q/K/V through strided views of the packed tensor and write O token-major,
and the backward writes dQ/dK/dV straight into one packed [B, T, 3·H·Dh] gradient — no
permute/contiguous/cat copies around attention (PyTorch SDPA needs three of them).

Head dim 64 (ViT-B/16, GPT-2-medium) runs on the HIP kernels; anything else falls back to
``F.scaled_dot_product_attention``. CPU tensors use the math reference.

Grouped-query attention: ``attention_qkv(qkv, heads, causal, kv_heads=Hkv)`` takes the packed tensor
[B, T, (H + 2·Hkv)·Dh] (H query heads, then Hkv key heads, then Hkv value heads: the row order of
``torch.cat([q_proj, k_proj, v_proj]).weight``); query head h reads K/V head h // (H / Hkv), HF's
``repeat_kv`` order. The GQA kernels read the Hkv heads in place (no expanded copy) and the dK/dV
kernel sums a group's query heads in fp32 registers in a fixed order: no atomics, one rounding.
``kv_heads`` of ``None`` or ``heads`` is multi-head attention, the code path above unchanged. There is
no dropout on the grouped-query path.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ._native import native, use_native

KERNEL_HEAD_DIMS = (64,)


def _views(qkv: torch.Tensor, heads: int):
    B, T, C3 = qkv.shape
    dh = C3 // (3 * heads)
    v5 = qkv.view(B, T, 3, heads, dh)
    return [v5[:, :, i].permute(0, 2, 1, 3) for i in range(3)], dh  # each [B, H, T, Dh] strided


class _FlashQKVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, causal, scale):
        B, T, _ = qkv.shape
        (q, k, v), dh = _views(qkv, heads)
        out = torch.empty(B, T, heads, dh, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, heads, T, device=qkv.device, dtype=torch.float32)
        native().attn_fwd_out(q, k, v, out.permute(0, 2, 1, 3), lse, causal, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads, ctx.causal, ctx.scale = heads, causal, scale
        return out.view(B, T, heads * dh)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, _ = qkv.shape
        heads = ctx.heads
        (q, k, v), dh = _views(qkv, heads)
        dout = dout.contiguous().view(B, T, heads, dh).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        (dq, dk, dv), _ = _views(dqkv, heads)
        native().attn_bwd_out(dout, q, k, v, out.permute(0, 2, 1, 3), lse, dq, dk, dv, ctx.causal, ctx.scale)
        return dqkv, None, None, None


def _views_gqa(qkv: torch.Tensor, heads: int, kv_heads: int):
    """q [B, H, T, Dh], k and v [B, Hkv, T, Dh]: strided views of the packed [B, T, (H + 2·Hkv)·Dh]."""
    B, T, C = qkv.shape
    dh = C // (heads + 2 * kv_heads)
    v4 = qkv.view(B, T, heads + 2 * kv_heads, dh).permute(0, 2, 1, 3)
    return (v4[:, :heads], v4[:, heads:heads + kv_heads], v4[:, heads + kv_heads:]), dh


class _FlashGQAFn(torch.autograd.Function):
    """_FlashQKVFn for kv_heads < heads: the GQA instantiations of the flash kernels on views of the
    packed tensor; the backward fills one packed dqkv of the forward's layout."""

    @staticmethod
    def forward(ctx, qkv, heads, kv_heads, causal, scale):
        B, T, _ = qkv.shape
        (q, k, v), dh = _views_gqa(qkv, heads, kv_heads)
        out = torch.empty(B, T, heads, dh, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, heads, T, device=qkv.device, dtype=torch.float32)
        native().attn_fwd_gqa_out(q, k, v, out.permute(0, 2, 1, 3), lse, causal, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads, ctx.kv_heads, ctx.causal, ctx.scale = heads, kv_heads, causal, scale
        return out.view(B, T, heads * dh)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, _ = qkv.shape
        heads, kv_heads = ctx.heads, ctx.kv_heads
        (q, k, v), dh = _views_gqa(qkv, heads, kv_heads)
        dout = dout.contiguous().view(B, T, heads, dh).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        (dq, dk, dv), _ = _views_gqa(dqkv, heads, kv_heads)
        native().attn_bwd_gqa_out(dout, q, k, v, out.permute(0, 2, 1, 3), lse, dq, dk, dv, ctx.causal, ctx.scale)
        return dqkv, None, None, None, None


def _attention_gqa(qkv, heads, kv_heads, causal, scale):
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"attention_qkv: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    B, T, C = qkv.shape
    if C % (heads + 2 * kv_heads) != 0:
        raise ValueError(f"attention_qkv: last dim {C} is not (heads + 2·kv_heads)·Dh with heads = {heads}, "
                         f"kv_heads = {kv_heads}")
    dh = C // (heads + 2 * kv_heads)
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    flash = (use_native(qkv) and qkv.dtype == torch.bfloat16 and dh in KERNEL_HEAD_DIMS and qkv.stride(-1) == 1)
    if flash:  # a build without the GQA launchers is an error here, not a fall-back
        return _FlashGQAFn.apply(qkv.contiguous(), heads, kv_heads, causal, scale)
    (q, k, v), _ = _views_gqa(qkv, heads, kv_heads)
    G = heads // kv_heads  # expanded K/V; autograd sums each group's gradient
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    if qkv.is_cuda:
        y = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)
    else:
        y = attention_reference(q, k, v, causal, scale).to(qkv.dtype)
    return y.transpose(1, 2).reshape(B, T, heads * dh)


class _FlashQKVDropFn(torch.autograd.Function):
    """_FlashQKVFn with dropout on the attention probabilities: the DROP kernels regenerate the mask
    from (ticket, stream) in the forward, dQ and dK/dV kernels (csrc/philox.h); nothing else is saved."""

    @staticmethod
    def forward(ctx, qkv, heads, causal, scale, ticket, stream, thr):
        B, T, _ = qkv.shape
        (q, k, v), dh = _views(qkv, heads)
        out = torch.empty(B, T, heads, dh, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, heads, T, device=qkv.device, dtype=torch.float32)
        native().attn_fwd_drop_out(q, k, v, out.permute(0, 2, 1, 3), lse, causal, scale, ticket, stream, thr)
        ctx.save_for_backward(qkv, out, lse, ticket)
        ctx.heads, ctx.causal, ctx.scale, ctx.stream, ctx.thr = heads, causal, scale, stream, thr
        return out.view(B, T, heads * dh)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, ticket = ctx.saved_tensors
        B, T, _ = qkv.shape
        heads = ctx.heads
        (q, k, v), dh = _views(qkv, heads)
        dout = dout.contiguous().view(B, T, heads, dh).permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        (dq, dk, dv), _ = _views(dqkv, heads)
        native().attn_bwd_drop_out(dout, q, k, v, out.permute(0, 2, 1, 3), lse, dq, dk, dv, ctx.causal, ctx.scale,
                                   ticket, ctx.stream, ctx.thr)
        return dqkv, None, None, None, None, None, None


def attention_qkv(qkv: torch.Tensor, heads: int, causal: bool = False, dropout_p: float = 0.0,
                  scale: float | None = None, ticket=None, stream: int | None = None,
                  kv_heads: int | None = None) -> torch.Tensor:
    """Packed-QKV attention: [B, T, 3·H·Dh] -> [B, T, H·Dh]; with ``kv_heads`` (grouped-query attention)
    [B, T, (H + 2·Hkv)·Dh] -> [B, T, H·Dh]. ``kv_heads`` of ``None`` or ``heads`` is multi-head attention.

    ``dropout_p > 0`` with a ``ticket`` (ops/dropout.py) drops attention probabilities with the
    counter-generated mask and stays on the flash kernels (GPU) / the masked math reference (CPU).
    Without a ticket (or under PDT_DROPOUT_FUSED=0) ``dropout_p > 0`` is aten's: SDPA on the GPU.
    Grouped-query attention has no dropout form: ``kv_heads != heads`` with ``dropout_p > 0`` raises."""
    if kv_heads is not None and kv_heads != heads:
        if dropout_p != 0.0:
            raise ValueError("attention_qkv: dropout is not supported with grouped-query attention "
                             f"(kv_heads = {kv_heads}, heads = {heads})")
        return _attention_gqa(qkv, heads, kv_heads, causal, scale)
    B, T, C3 = qkv.shape
    dh = C3 // (3 * heads)
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    thr = 0
    if dropout_p != 0.0 and ticket is not None and ticket.tensor is not None:
        from .dropout import threshold
        thr = threshold(dropout_p)
        if stream is None:
            stream = ticket.next_stream()
        if thr == 0:
            dropout_p = 0.0
    flash = (use_native(qkv) and qkv.dtype == torch.bfloat16 and dh in KERNEL_HEAD_DIMS
             and qkv.stride(-1) == 1 and hasattr(native(), "attn_fwd_out"))
    if flash and thr > 0:
        return _FlashQKVDropFn.apply(qkv.contiguous(), heads, causal, scale, ticket.tensor, int(stream), thr)
    if flash and dropout_p == 0.0:
        return _FlashQKVFn.apply(qkv.contiguous(), heads, causal, scale)
    (q, k, v), _ = _views(qkv, heads)
    if thr > 0:  # our mask off the flash kernels (CPU, other head dims / dtypes): masked math reference
        from .dropout import dropout_mask
        m = dropout_mask(ticket.tensor, stream, (B, heads, T, T), dropout_p, "attn")
        y = attention_reference(q, k, v, causal, scale, keep=m, keep_scale=256.0 / (256 - thr)).to(qkv.dtype)
    elif qkv.is_cuda:
        y = F.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, is_causal=causal, scale=scale)
    else:
        y = attention_reference(q, k, v, causal, scale, aten_dropout_p=dropout_p).to(qkv.dtype)
    return y.transpose(1, 2).reshape(B, T, heads * dh)


# ----------------------------------------------------------------------------- decoding on a KV cache
DECODE_STATS = {"native_calls": 0, "geo": None}  # launches of the decode kernel and the last (S, C) it ran with


def attention_decode_geo(batch: int, kv_heads: int, capacity: int, splits: int | None = None, group: int = 1):
    """(S, C) of the split-KV decode kernel for a cache: S splits of C keys each (C % 64 == 0, S =
    ceil(capacity / C)). A function of the cache's shape, never of ``lens``. ``splits``: ask for that many
    instead of the default rule; ``group`` = heads / kv_heads."""
    S, C = native().attn_decode_geo(batch, kv_heads, capacity, int(splits or 0), group)
    return int(S), int(C)


def _decode_reference(qkv, k_cache, v_cache, lens, heads, kv_heads, scale):
    B, _, _ = qkv.shape
    cap, dh = k_cache.shape[2], k_cache.shape[3]
    G = heads // kv_heads
    q = qkv[:, 0, :heads * dh].reshape(B, heads, dh).float()
    valid = torch.arange(cap, device=qkv.device)[None, :] <= lens[:, None]  # [B, cap]: keys 0 .. lens[b]
    k = k_cache.float().repeat_interleave(G, dim=1)
    # rows past lens[b] may hold anything, NaN included: they are taken out, not multiplied by zero
    v = torch.where(valid[:, None, :, None], v_cache.float(), torch.zeros((), device=qkv.device))
    s = torch.einsum("bhd,bhkd->bhk", q, k) * scale
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhk,bhkd->bhd", p, v.repeat_interleave(G, dim=1))
    return o.to(qkv.dtype).reshape(B, 1, heads * dh), lse


def attention_decode(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor,
                     heads: int, kv_heads: int | None = None, scale: float | None = None,
                     splits: int | None = None, cache=None, return_lse: bool = False):
    """Attention of one new token per sequence on a KV cache: ``qkv`` [B, 1, (H + 2·Hkv)·64] with Q rotated
    (``rope_append_`` has already written the token's K and V at position ``lens[b]``), ``k_cache`` /
    ``v_cache`` [B, Hkv, capacity, 64], ``lens`` int32 [B] on qkv's device, read there. Returns [B, 1, H·64]
    (and the LSE [B, H] with ``return_lse``). Inference only: raises when a gradient is required.

    bf16 GPU tensors run the split-KV kernel (csrc/kernels/attn_decode.hip); ``splits`` overrides its number
    of splits and ``cache`` (a ``KVCache``) lends the scratch of the partials, so that no step allocates it.
    CPU, fp32 and ``PDT_DISABLE_NATIVE=1`` take the PyTorch reference."""
    kv_heads = heads if kv_heads is None else kv_heads
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"attention_decode: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, k_cache, v_cache)):
        raise RuntimeError("attention_decode: inference only (run it under torch.no_grad())")
    if qkv.dim() != 3 or qkv.shape[1] != 1 or qkv.shape[2] % (heads + 2 * kv_heads) != 0:
        raise ValueError(f"attention_decode: qkv {tuple(qkv.shape)} is not [B, 1, (heads + 2·kv_heads)·Dh]")
    dh = qkv.shape[2] // (heads + 2 * kv_heads)
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if use_native(qkv) and qkv.dtype == torch.bfloat16:  # head dim 64 and the layouts: the binding's checks
        B, cap = qkv.shape[0], k_cache.shape[2] if k_cache.dim() == 4 else 0
        out = torch.empty(B, 1, heads * dh, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, heads, device=qkv.device, dtype=torch.float32) if return_lse else None
        o_part = ml_part = None
        if cap > 0 and k_cache.dim() == 4 and dh == 64:
            S, _ = attention_decode_geo(B, kv_heads, cap, splits, heads // kv_heads)
            if S > 1:
                if cache is not None:
                    o_part, ml_part = cache.scratch(heads, S)
                else:
                    o_part = torch.empty(B, heads, S, 64, device=qkv.device, dtype=torch.float32)
                    ml_part = torch.empty(B, heads, S, 2, device=qkv.device, dtype=torch.float32)
        geo = native().attn_decode(qkv, k_cache, v_cache, lens, heads, kv_heads, scale, int(splits or 0), out,
                                   o_part, ml_part, lse)
        DECODE_STATS["native_calls"] += 1
        DECODE_STATS["geo"] = (int(geo[0]), int(geo[1]))
        return (out, lse) if return_lse else out
    out, lse = _decode_reference(qkv, k_cache, v_cache, lens, heads, kv_heads, scale)
    return (out, lse) if return_lse else out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False,
              dropout_p: float = 0.0, scale: float | None = None) -> torch.Tensor:
    """Unpacked [B, H, T, Dh] interface (SDPA-compatible)."""
    return F.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, is_causal=causal, scale=scale)


def attention_reference(q, k, v, causal=False, scale=None, keep=None, keep_scale=1.0, aten_dropout_p=0.0):
    """fp32 math reference (tests, CPU). ``keep`` [B, H, T, T] bool: dropout of the probabilities
    (softmax(S) * keep * keep_scale); ``aten_dropout_p``: ``F.dropout`` on them instead."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    if causal:
        T, S = s.shape[-2], s.shape[-1]
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(S - T)
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.to(p.dtype) * keep_scale
    elif aten_dropout_p:
        p = F.dropout(p, aten_dropout_p, training=True)
    return p @ v.float()
