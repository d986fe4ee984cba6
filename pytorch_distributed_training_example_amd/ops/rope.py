"""Rotary position embedding on the packed QKV tensor (csrc/kernels/rope.hip).

``rope_qkv_(qkv, cos, sin, heads)`` rotates the Q and K thirds of the ``c_attn`` output
[B, T, 3·H·Dh] in place and returns it; V is not touched. With ``kv_heads=Hkv`` (grouped-query
attention) the tensor is [B, T, (H + 2·Hkv)·Dh]: the H query heads and the Hkv key heads, columns
[0, (H + Hkv)·Dh), are rotated and the Hkv value heads behind them are neither read nor written. Half-split convention (HF's
``rotate_half``): for every head, position t and j < Dh/2

    x'[j]        = x[j]·cos[t, j] − x[j + Dh/2]·sin[t, j]
    x'[j + Dh/2] = x[j + Dh/2]·cos[t, j] + x[j]·sin[t, j]

The rotation is orthogonal, so the backward is the same kernel with the sine negated, run in place
on the packed gradient attention's backward returns: one read and one write of the rotated heads
each way, no copy of V, nothing saved but the table. bf16 GPU tensors at head dim 64 take the
HIP kernel; anything else (CPU, fp32, ``PDT_DISABLE_NATIVE=1``) the same math in plain PyTorch.
"""
from __future__ import annotations

import torch
from torch import nn

from ._native import native, use_native

KERNEL_HEAD_DIM = 64


def rope_table(T_max: int, base: float = 10000.0, dim: int = 64):
    """``(cos, sin)``, fp32 [T_max, dim/2]: the angle of position t and pair j is t · base^(−2j/dim),
    formed in float64 and rounded once."""
    assert dim % 2 == 0
    j = torch.arange(dim // 2, dtype=torch.float64)
    inv_freq = torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * j / dim)
    ang = torch.arange(T_max, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return torch.cos(ang).float(), torch.sin(ang).float()


class RotaryTable(nn.Module):
    """The table as non-persistent buffers ``cos`` / ``sin`` (not in the state_dict; rebuilt from
    ``base``). A module of its own so that the precision policies can leave it in fp32
    (models/precision.py), which is what the kernel reads."""

    def __init__(self, T_max: int, base: float = 10000.0, dim: int = 64):
        super().__init__()
        cos, sin = rope_table(T_max, base, dim)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)


def _native_ok(qkv, cos, sin, heads, kv_heads) -> bool:
    return (use_native(qkv) and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.is_contiguous()
            and qkv.shape[-1] == (heads + 2 * kv_heads) * KERNEL_HEAD_DIM and cos.dtype == torch.float32
            and cos.shape[-1] == KERNEL_HEAD_DIM // 2 and qkv.data_ptr() % 16 == 0)


def _rotate_reference_(qkv, cos, sin, heads, kv_heads, conj):
    B, T, C = qkv.shape
    dh = C // (heads + 2 * kv_heads)
    half = dh // 2
    qk = qkv.view(B, T, heads + 2 * kv_heads, dh)[:, :, :heads + kv_heads]  # the Q heads, then the K heads
    lo, hi = qk[..., :half].float(), qk[..., half:].float()
    c = cos[:T].float().view(1, T, 1, half)
    s = sin[:T].float().view(1, T, 1, half)
    if conj:
        s = -s
    new_lo, new_hi = lo * c - hi * s, hi * c + lo * s  # both before either write: lo / hi alias qkv in fp32
    qk[..., :half] = new_lo.to(qkv.dtype)
    qk[..., half:] = new_hi.to(qkv.dtype)
    return qkv


def _rotate_(qkv, cos, sin, heads, kv_heads, conj):
    B, T, C = qkv.shape
    if T > cos.shape[0]:
        raise ValueError(f"rope: sequence length {T} exceeds the table's {cos.shape[0]} positions")
    if _native_ok(qkv, cos, sin, heads, kv_heads):
        if kv_heads == heads:
            native().rope_qkv(qkv, cos, sin, heads, conj)
        else:
            native().rope_qkv_gqa(qkv, cos, sin, heads, kv_heads, conj)
        return qkv
    return _rotate_reference_(qkv, cos, sin, heads, kv_heads, conj)


class _RopeQKVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, heads, kv_heads):
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(cos, sin)
        ctx.heads, ctx.kv_heads = heads, kv_heads
        return _rotate_(qkv, cos, sin, heads, kv_heads, False)

    @staticmethod
    def backward(ctx, dqkv):
        cos, sin = ctx.saved_tensors
        # in place on the gradient attention's backward just wrote (contiguous() is then a no-op)
        return _rotate_(dqkv.contiguous(), cos, sin, ctx.heads, ctx.kv_heads, True), None, None, None, None


def rope_qkv_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int,
              kv_heads: int | None = None) -> torch.Tensor:
    """Rotate Q and K of the packed ``qkv`` [B, T, (heads + 2·kv_heads)·Dh] in place; returns ``qkv``.
    ``kv_heads`` of ``None`` is ``heads``: the multi-head layout [B, T, 3·heads·Dh]."""
    kv_heads = heads if kv_heads is None else kv_heads
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"rope_qkv_: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    if qkv.dim() != 3 or qkv.shape[-1] % (heads + 2 * kv_heads) != 0:
        raise ValueError(f"rope_qkv_: qkv {tuple(qkv.shape)} is not [B, T, (heads + 2·kv_heads)·Dh] with "
                         f"heads = {heads}, kv_heads = {kv_heads}")
    if not qkv.is_contiguous():
        raise ValueError("rope_qkv_: qkv must be contiguous (it is rotated in place)")
    if torch.is_grad_enabled() and qkv.requires_grad:
        return _RopeQKVFn.apply(qkv, cos, sin, heads, kv_heads)
    return _rotate_(qkv, cos, sin, heads, kv_heads, False)


# ----------------------------------------------------------------------------- decoding: rotate at an offset + cache write
APPEND_STATS = {"native_calls": 0}  # launches of the append kernel


def _append_reference_(qkv, cos, sin, heads, kv_heads, k_cache, v_cache, lens):
    """The kernel's contract in tensor ops, without a host read of ``lens``: row (b, t) sits at position
    p = lens[b] + t; a row whose p is outside the cache or the table changes nothing."""
    B, Tn, C = qkv.shape
    dh = C // (heads + 2 * kv_heads)
    half = dh // 2
    cap = k_cache.shape[2]
    limit = min(cap, cos.shape[0])
    pos = lens.long()[:, None] + torch.arange(Tn, device=qkv.device)[None, :]  # [B, Tn]
    ok = (pos >= 0) & (pos < limit)
    pc = pos.clamp(0, limit - 1)
    x = qkv.view(B, Tn, heads + 2 * kv_heads, dh)
    qk = x[:, :, :heads + kv_heads]
    lo, hi = qk[..., :half].float(), qk[..., half:].float()
    c, s = cos.float()[pc][:, :, None, :], sin.float()[pc][:, :, None, :]
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], -1).to(qkv.dtype)  # [B, Tn, H + Hkv, dh]
    x[:, :, :heads + kv_heads] = torch.where(ok[:, :, None, None], rot, x[:, :, :heads + kv_heads])
    # cache position j of sequence b takes new row t = j - lens[b] when 0 <= t < Tn (a gather: no write races)
    t = torch.arange(cap, device=qkv.device)[None, :] - lens.long()[:, None]  # [B, cap]
    take = (t >= 0) & (t < Tn) & (torch.arange(cap, device=qkv.device)[None, :] < limit)
    idx = t.clamp(0, Tn - 1)[:, None, :, None].expand(B, kv_heads, cap, dh)
    for cache_t, new in ((k_cache, rot[:, :, heads:]), (v_cache, x[:, :, heads + kv_heads:])):
        rows = new.permute(0, 2, 1, 3).gather(2, idx)  # [B, Hkv, cap, dh]
        cache_t.copy_(torch.where(take[:, None, :, None], rows.to(cache_t.dtype), cache_t))
    return qkv


def rope_append_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, kv_heads: int | None,
                 k_cache: torch.Tensor, v_cache: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """The rotary embedding at a per-sequence offset, fused with the KV-cache write. ``qkv`` [B, Tn,
    (heads + 2·kv_heads)·Dh] holds ``c_attn``'s output for Tn new tokens; row (b, t) sits at position
    p = lens[b] + t (``lens`` int32 [B] on qkv's device, read there). The query and key heads are rotated in
    place with cos/sin[p], as ``rope_qkv_`` rotates row p of a full sequence; the rotated key heads and the
    untouched value heads also go to ``k_cache[b, :, p]`` / ``v_cache[b, :, p]`` ([B, kv_heads, capacity, Dh],
    contiguous).
    A row whose p falls outside the cache or the table writes nothing. Returns ``qkv``; ``lens`` is not
    advanced. Inference only: raises when a gradient is required."""
    kv_heads = heads if kv_heads is None else kv_heads
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"rope_append_: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, k_cache, v_cache)):
        raise RuntimeError("rope_append_: inference only (run it under torch.no_grad())")
    if qkv.dim() != 3 or qkv.shape[-1] % (heads + 2 * kv_heads) != 0 or not qkv.is_contiguous():
        raise ValueError(f"rope_append_: qkv {tuple(qkv.shape)} is not a contiguous [B, Tn, (heads + 2·kv_heads)·Dh] "
                         f"with heads = {heads}, kv_heads = {kv_heads}")
    if use_native(qkv) and qkv.dtype == torch.bfloat16:  # head dim 64, layouts, lens: the binding's checks
        native().rope_kv_append(qkv, cos, sin, heads, kv_heads, k_cache, v_cache, lens)
        APPEND_STATS["native_calls"] += 1
        return qkv
    dh = qkv.shape[-1] // (heads + 2 * kv_heads)
    if k_cache.shape != v_cache.shape or k_cache.dim() != 4 or k_cache.shape[0] != qkv.shape[0] \
            or k_cache.shape[1] != kv_heads or k_cache.shape[3] != dh:
        raise ValueError(f"rope_append_: caches {tuple(k_cache.shape)}, {tuple(v_cache.shape)} are not "
                         f"[{qkv.shape[0]}, {kv_heads}, capacity, {dh}]")
    return _append_reference_(qkv, cos, sin, heads, kv_heads, k_cache, v_cache, lens)
