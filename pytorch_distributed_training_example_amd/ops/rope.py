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
from .kv_cache import PAGE

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


# ----------------------------------------------------------------------------- the same on a paged cache
APPEND_PAGED_STATS = {"native_calls": 0}  # launches of the paged append kernel


def gather_pages(pool: torch.Tensor, block_table: torch.Tensor) -> torch.Tensor:
    """A slot's pages as a contiguous cache [B, Hkv, 64·max_pages, Dh], for the reference paths: ``pool``
    [n_pages, Hkv, 64, Dh] read through ``block_table`` [B, max_pages]; an entry outside the pool gives zero
    rows, as the kernel's resource of zero records does."""
    B, mp = block_table.shape
    tbl = block_table.long()
    ok = (tbl >= 0) & (tbl < pool.shape[0])
    pages = torch.where(ok[:, :, None, None, None], pool[torch.where(ok, tbl, torch.zeros_like(tbl))],
                        torch.zeros((), dtype=pool.dtype, device=pool.device))
    return pages.permute(0, 2, 1, 3, 4).reshape(B, pool.shape[1], mp * PAGE, pool.shape[3])


def rope_append_paged_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, kv_heads: int | None,
                       k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                       lens: torch.Tensor) -> torch.Tensor:
    """``rope_append_`` on a paged cache: ``k_pool`` / ``v_pool`` [n_pages, kv_heads, 64, Dh] hold pages of 64
    positions and ``block_table`` (int32 [B, max_pages], on qkv's device) names the page of positions
    [64 j, 64 j + 64) of slot b, or -1. Row (b, t) at p = lens[b] + t is rotated in place as ``rope_append_``
    rotates it and stored at row p & 63 of page ``block_table[b, p >> 6]``; a row whose p is outside the table or
    the rotary table does nothing, one whose page id is outside the pool is rotated and not stored. Returns
    ``qkv``; ``lens`` is not advanced. Inference only."""
    kv_heads = heads if kv_heads is None else kv_heads
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"rope_append_paged_: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, k_pool, v_pool)):
        raise RuntimeError("rope_append_paged_: inference only (run it under torch.no_grad())")
    if qkv.dim() != 3 or qkv.shape[-1] % (heads + 2 * kv_heads) != 0 or not qkv.is_contiguous():
        raise ValueError(f"rope_append_paged_: qkv {tuple(qkv.shape)} is not a contiguous [B, Tn, (heads + "
                         f"2·kv_heads)·Dh] with heads = {heads}, kv_heads = {kv_heads}")
    if use_native(qkv) and qkv.dtype == torch.bfloat16:  # head dim 64, layouts, table, lens: the binding's checks
        native().rope_kv_append_paged(qkv, cos, sin, heads, kv_heads, k_pool, v_pool, block_table, lens)
        APPEND_PAGED_STATS["native_calls"] += 1
        return qkv
    dh = qkv.shape[-1] // (heads + 2 * kv_heads)
    if k_pool.shape != v_pool.shape or k_pool.dim() != 4 or tuple(k_pool.shape[1:]) != (kv_heads, PAGE, dh) \
            or block_table.dim() != 2 or block_table.shape[0] != qkv.shape[0]:
        raise ValueError(f"rope_append_paged_: pools {tuple(k_pool.shape)}, {tuple(v_pool.shape)} are not [n_pages, "
                         f"{kv_heads}, {PAGE}, {dh}] or the table {tuple(block_table.shape)} is not [{qkv.shape[0]}, "
                         "max_pages]")
    # the contiguous reference on the gathered pages, then the named pages written back
    B, mp = block_table.shape
    kc, vc = gather_pages(k_pool, block_table), gather_pages(v_pool, block_table)
    _append_reference_(qkv, cos, sin, heads, kv_heads, kc, vc, lens)
    tbl = block_table.long()
    ok = (tbl >= 0) & (tbl < k_pool.shape[0])
    for pool, c in ((k_pool, kc), (v_pool, vc)):
        pool[tbl[ok]] = c.view(B, kv_heads, mp, PAGE, dh).permute(0, 2, 1, 3, 4)[ok]
    return qkv


# ----------------------------------------------------------------------------- the same on an e4m3 paged cache
APPEND_PAGED_FP8_STATS = {"native_calls": 0}  # launches of the quantising paged append kernel


def rope_append_paged_fp8_(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, heads: int, kv_heads: int | None,
                           k_pool: torch.Tensor, v_pool: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                           block_table: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """``rope_append_paged_`` with a quantising store (csrc/kernels/attn_paged_fp8.hip): ``k_pool`` / ``v_pool``
    [n_pages, kv_heads, 64, 64] float8_e4m3fn and ``k_scale`` / ``v_scale`` [n_pages, kv_heads, 64] fp32. ``qkv`` is
    rotated in place exactly as ``rope_append_paged_`` rotates it; the row that call would store (K: the rotated
    row after its rounding to qkv's dtype) goes to the pools as ``quantize_rows_e4m3`` of it, bytes and scale. Rows
    out of range behave as there. Returns ``qkv``; ``lens`` is not advanced. Inference only.

    bf16 GPU tensors run the kernel; CPU, fp32 and ``PDT_DISABLE_NATIVE=1`` pass the bf16 reference's rows through
    the torch form of ``quantize_rows_e4m3``."""
    kv_heads = heads if kv_heads is None else kv_heads
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"rope_append_paged_fp8_: heads = {heads} is not a positive multiple of kv_heads = {kv_heads}")
    if torch.is_grad_enabled() and qkv.requires_grad:
        raise RuntimeError("rope_append_paged_fp8_: inference only (run it under torch.no_grad())")
    if qkv.dim() != 3 or qkv.shape[-1] % (heads + 2 * kv_heads) != 0 or not qkv.is_contiguous():
        raise ValueError(f"rope_append_paged_fp8_: qkv {tuple(qkv.shape)} is not a contiguous [B, Tn, (heads + "
                         f"2·kv_heads)·Dh] with heads = {heads}, kv_heads = {kv_heads}")
    if use_native(qkv) and qkv.dtype == torch.bfloat16:  # dtypes, layouts, table, lens: the binding's checks
        native().rope_kv_append_paged_fp8(qkv, cos, sin, heads, kv_heads, k_pool, v_pool, k_scale, v_scale,
                                          block_table, lens)
        APPEND_PAGED_FP8_STATS["native_calls"] += 1
        return qkv
    from .linear import quantize_rows_e4m3_reference
    dh = qkv.shape[-1] // (heads + 2 * kv_heads)
    if k_pool.dtype != torch.float8_e4m3fn or k_pool.shape != v_pool.shape or k_pool.dim() != 4 \
            or tuple(k_pool.shape[1:]) != (kv_heads, PAGE, dh) or k_scale.shape != k_pool.shape[:3] \
            or v_scale.shape != k_pool.shape[:3] or block_table.dim() != 2 or block_table.shape[0] != qkv.shape[0]:
        raise ValueError(f"rope_append_paged_fp8_: pools {tuple(k_pool.shape)}, {tuple(v_pool.shape)} are not e4m3 "
                         f"[n_pages, {kv_heads}, {PAGE}, {dh}] with scale pools [n_pages, {kv_heads}, {PAGE}], or the "
                         f"table {tuple(block_table.shape)} is not [{qkv.shape[0]}, max_pages]")
    # the contiguous reference into an empty cache of qkv's dtype, then the written rows quantised into their pages
    B, Tn = qkv.shape[0], qkv.shape[1]
    cap = block_table.shape[1] * PAGE
    kc = torch.zeros(B, kv_heads, cap, dh, dtype=qkv.dtype, device=qkv.device)
    vc = torch.zeros_like(kc)
    _append_reference_(qkv, cos, sin, heads, kv_heads, kc, vc, lens)
    pos = torch.arange(cap, device=qkv.device)[None, :].expand(B, cap)
    t = pos - lens.long()[:, None]
    page = block_table.long().gather(1, pos >> 6)
    take = (t >= 0) & (t < Tn) & (pos < min(cap, cos.shape[0])) & (page >= 0) & (page < k_pool.shape[0])
    bi, ji = take.nonzero(as_tuple=True)
    pg, row = page[bi, ji], ji & (PAGE - 1)
    for pool, scale, c in ((k_pool, k_scale, kc), (v_pool, v_scale, vc)):
        q, s = quantize_rows_e4m3_reference(c[bi, :, ji].reshape(-1, dh))
        pool.view(torch.uint8)[pg, :, row] = q.view(torch.uint8).view(-1, kv_heads, dh)
        scale[pg, :, row] = s.view(-1, kv_heads)
    return qkv
