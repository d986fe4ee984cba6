"""Dropout whose mask is a pure function of a counter (csrc/philox.h), never a stored tensor.

One mask definition serves every site: the elementwise kernel (csrc/kernels/dropout.hip), the
residual dropout inside add+LayerNorm (layernorm.hip), the attention-probability dropout inside the
flash kernels (attention.hip) and the CPU reference below, which CPU tensors take — so CPU and GPU
draw identical masks and the backward regenerates what the forward used from ``(ticket, stream)``.

Contract (philox.h has the full statement):
  * Philox4x32-10, counter ``(block_lo, block_hi, stream, step)``, key ``(key_lo, key_hi)``;
  * keep iff the element's byte ``>= thr``, ``thr = round(256 p)`` clamped to 0..255; every kernel
    scales by ``1 / (1 - p_eff)`` with ``p_eff = thr / 256`` (``effective_p``);
  * ``key = (seed + rank * 0x9E3779B97F4A7C15) mod 2^64``: ranks sharing a seed draw different masks;
  * ``DropoutState.begin_forward`` writes the *ticket* ``(key, step)`` on the device and advances the
    device step counter in one tiny kernel (captured by a hipGraph: each replay draws fresh masks);
    the ticket hands out consecutive ``stream`` ids to the dropout sites of that forward.

``PDT_DROPOUT_FUSED=0`` (config.py) replaces all of this by ``F.dropout`` / SDPA's dropout (A/B and
escape hatch): ``begin_forward`` then returns a ticket without a tensor and launches nothing.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from ..config import SW
from ._native import native, use_native

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_RANK_STRIDE = 0x9E3779B97F4A7C15
_MASK64 = (1 << 64) - 1


def threshold(p: float) -> int:
    """Keep iff byte >= threshold(p): round(256 p) clamped to 0..255."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return max(0, min(255, int(math.floor(p * 256.0 + 0.5))))


def effective_p(p: float) -> float:
    """The probability the kernels realise (and scale by): threshold(p) / 256."""
    return threshold(p) / 256.0


def scale_of(thr: int) -> float:
    """1 / (1 - thr/256) as the fp32 value the kernels multiply by."""
    return float(np.float32(256.0) / np.float32(256 - thr))


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy uint32 arrays: ``counter`` 4 arrays (broadcastable), ``key`` 2 ints.
    Returns the 4 output words. (0,0,0,0) / (0,0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0.astype(np.uint64)
        p1 = _M1 * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _block_bytes(blocks: np.ndarray, key: int, step: int, stream: int) -> np.ndarray:
    """[len(blocks), 16] uint8: the 16 mask bytes of each Philox block (byte e = word e>>2, bits 8(e&3)..)."""
    key &= _MASK64
    blocks = blocks.astype(np.uint64)
    words = philox4x32_10(((blocks & np.uint64(0xFFFFFFFF)).astype(np.uint32), (blocks >> np.uint64(32)).astype(np.uint32),
                           np.uint32(stream & 0xFFFFFFFF), np.uint32(step & 0xFFFFFFFF)),
                          (key & 0xFFFFFFFF, key >> 32))
    w = np.stack(words, axis=-1).astype("<u4")  # [n, 4] little-endian words
    return w.view(np.uint8).reshape(len(blocks), 16)


def reference_mask(seed: int, step: int, stream: int, shape: Sequence[int], p: float, kind: str = "flat",
                   heads: Optional[int] = None) -> torch.Tensor:
    """The bool keep mask on the CPU. ``seed`` is the 64-bit key the kernels see (``DropoutState.key``:
    the seed itself on rank 0). ``kind="flat"``: element order of ``shape``; ``kind="attn"``:
    ``shape = (B, H, T, T)`` in 4 x 4 (query x key) patches (philox.h)."""
    thr = threshold(p)
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if shape else 1
    if kind == "flat":
        nblk = (n + 15) // 16
        by = _block_bytes(np.arange(nblk, dtype=np.uint64), seed, step, stream).reshape(-1)[:n]
        return torch.from_numpy((by >= thr).reshape(shape))
    if kind != "attn":
        raise ValueError(f"unknown mask kind {kind!r}")
    if len(shape) != 4 or shape[2] != shape[3] or (heads is not None and heads != shape[1]):
        raise ValueError(f"attn mask wants shape (B, H, T, T) with H == heads, got {shape}, heads={heads}")
    B, H, T, _ = shape
    TP = (T + 3) // 4
    by = _block_bytes(np.arange(B * H * TP * TP, dtype=np.uint64), seed, step, stream)
    # [BH, qp, kp, qi, ki] -> [BH, qp, qi, kp, ki] -> [B, H, 4TP, 4TP] cut to T
    by = by.reshape(B * H, TP, TP, 4, 4).transpose(0, 1, 3, 2, 4).reshape(B, H, 4 * TP, 4 * TP)[:, :, :T, :T]
    return torch.from_numpy(np.ascontiguousarray(by >= thr))


def _signed(v: int) -> int:
    v &= _MASK64
    return v - (1 << 64) if v >= (1 << 63) else v


class Ticket:
    """One forward's ``(key, step)`` device tensor plus the host counter of its dropout sites."""
    __slots__ = ("tensor", "_next")

    def __init__(self, tensor: Optional[torch.Tensor]):
        self.tensor = tensor  # int64 [2], or None under PDT_DROPOUT_FUSED=0 (aten draws its own masks)
        self._next = 0

    def next_stream(self) -> int:
        s = self._next
        self._next += 1
        return s


class DropoutState:
    """Host seed + device ``(key, step)`` counter. No host read on the step path."""

    def __init__(self, seed: int = 0, rank: int = 0):
        self.seed, self.rank = int(seed), int(rank)
        self._host_step = 0
        self._dev: Optional[torch.Tensor] = None  # int64 [2] = (key, step), created on first use

    @property
    def key(self) -> int:
        return (self.seed + self.rank * _RANK_STRIDE) & _MASK64

    def _device_state(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None or self._dev.device != device:
            if self._dev is not None:
                self._host_step = int(self._dev[1].item())
            self._dev = torch.tensor([_signed(self.key), self._host_step], dtype=torch.int64, device=device)
        return self._dev

    def begin_forward(self, device="cpu") -> Ticket:
        if not SW.dropout_fused:
            return Ticket(None)
        st = self._device_state(device)
        if st.is_cuda:
            return Ticket(native().dropout_begin(st))
        t = st.clone()
        st[1] += 1
        return Ticket(t)

    def get_state(self) -> dict:
        """``{"seed", "step"}`` as plain ints (synchronises)."""
        step = int(self._dev[1].item()) if self._dev is not None else self._host_step
        return {"seed": self.seed, "step": step}

    def set_state(self, seed: int, step: int) -> None:
        """In place on the device tensor, so a captured ``begin_forward`` sees it on the next replay."""
        self.seed, self._host_step = int(seed), int(step)
        if self._dev is not None:
            self._dev.copy_(torch.tensor([_signed(self.key), self._host_step], dtype=torch.int64))


_STATE = DropoutState()


def default_state() -> DropoutState:
    """The process-wide state the models draw from (cli.py seeds it from --seed and the rank)."""
    return _STATE


def manual_seed(seed: int, rank: int = 0, step: int = 0) -> DropoutState:
    _STATE.rank = int(rank)
    _STATE.set_state(seed, step)
    return _STATE


def begin_forward(device="cpu") -> Ticket:
    return _STATE.begin_forward(device)


def get_state() -> dict:
    return _STATE.get_state()


def set_state(seed: int, step: int) -> None:
    _STATE.set_state(seed, step)


def ticket_values(ticket: torch.Tensor):
    """(key, step) of a ticket as Python ints (CPU reference paths and tests; synchronises on the GPU)."""
    k, s = ticket.tolist()
    return k & _MASK64, s


def dropout_mask(ticket, stream: int, shape: Sequence[int], p: float, kind: str = "flat") -> torch.Tensor:
    """The bool keep mask of one site: on the GPU from the device functions the kernels inline, on the
    CPU from ``reference_mask``."""
    t = ticket.tensor if isinstance(ticket, Ticket) else ticket
    if t.is_cuda:
        return native().dropout_mask(t, int(stream), [int(s) for s in shape], threshold(p), kind)
    key, step = ticket_values(t)
    return reference_mask(key, step, stream, shape, p, kind)


class _DropFn(torch.autograd.Function):
    """y = round_T(x * m * scale); saves the ticket and the stream id, nothing else."""

    @staticmethod
    def _apply_mask(x, ticket, stream, thr):
        if x.is_cuda:
            return native().dropout_fwd(x.contiguous(), ticket, stream, thr)
        key, step = ticket_values(ticket)
        m = reference_mask(key, step, stream, x.shape, thr / 256.0)
        y = (x.float() * scale_of(thr)).to(x.dtype)
        return torch.where(m, y, torch.zeros((), dtype=x.dtype))

    @staticmethod
    def forward(ctx, x, ticket, stream, thr):
        ctx.save_for_backward(ticket)
        ctx.stream, ctx.thr = stream, thr
        return _DropFn._apply_mask(x, ticket, stream, thr)

    @staticmethod
    def backward(ctx, dy):
        (ticket,) = ctx.saved_tensors
        return _DropFn._apply_mask(dy, ticket, ctx.stream, ctx.thr), None, None, None


def dropout(x: torch.Tensor, p: float, ticket: Optional[Ticket], stream: Optional[int] = None) -> torch.Tensor:
    """Training-mode dropout of ``x`` with the mask of ``(ticket, stream)``; ``stream`` defaults to the
    ticket's next id. ``p == 0`` or no ticket: ``x`` itself, no launch. GPU tensors always take the HIP
    kernel, CPU tensors the reference."""
    if ticket is None or p == 0.0:
        return x
    if ticket.tensor is None:  # PDT_DROPOUT_FUSED=0
        return F.dropout(x, p, training=True)
    if stream is None:
        stream = ticket.next_stream()
    thr = threshold(p)
    if thr == 0:
        return x
    if x.is_cuda:
        use_native(x)  # raises when the extension is missing: no eager fallback on the GPU
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dropout: fp32 / bf16 only on the GPU, got {x.dtype}")
    return _DropFn.apply(x, ticket.tensor, int(stream), thr)
