"""The key/value cache of incremental decoding (csrc/kernels/attn_decode.hip reads and writes it).

``KVCache(n_layer, batch, kv_heads, capacity, device)`` holds, per layer, ``k[l]`` and ``v[l]``:
[B, Hkv, capacity, 64], contiguous, so one key row is one 128-byte line; K is stored after the rotary
embedding. ``lens`` (int32 [B], on the device) counts the valid positions of every sequence: the
kernels read it there, and nothing on the decode path reads it on the host, which is what lets a
captured decode step replay at a new position.

What the host does know is an upper bound of ``lens``, kept by the three mutators ``reset()``,
``advance(n)`` (a device add) and ``set_lens(...)`` without a device read; ``require(n, table_len)``
refuses ``bound + n > capacity`` and ``bound + n > table_len`` before any launch. (The kernels clamp
positions to the cache as well: a wrong ``lens`` costs a wrong answer, never an out-of-bounds store.)

The fp32 scratch of the split-KV partials belongs to the cache too: ``scratch(heads, S)`` allocates once
per (heads, S) and hands the same tensors back on every later step. The batch is fixed for the life of
a cache.
"""
from __future__ import annotations

import torch

HEAD_DIM = 64


class KVCache:
    def __init__(self, n_layer: int, batch: int, kv_heads: int, capacity: int, device, dtype=torch.bfloat16):
        if min(n_layer, batch, kv_heads, capacity) <= 0:
            raise ValueError(f"KVCache: n_layer, batch, kv_heads and capacity must be positive, got "
                             f"{(n_layer, batch, kv_heads, capacity)}")
        self.n_layer, self.batch, self.kv_heads, self.capacity = n_layer, batch, kv_heads, capacity
        self.device, self.dtype = torch.device(device), dtype
        shape = (batch, kv_heads, capacity, HEAD_DIM)
        self.k = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.v = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.lens = torch.zeros(batch, device=self.device, dtype=torch.int32)
        self._bound = 0  # host-side upper bound of lens
        self._scratch: dict = {}

    @property
    def bound(self) -> int:
        """An upper bound of ``lens``, known without reading the device."""
        return self._bound

    def reset(self) -> None:
        self.lens.zero_()
        self._bound = 0

    def advance(self, n: int = 1) -> None:
        """``lens += n`` on the device; the bound follows."""
        self.lens.add_(n)
        self._bound += n

    def set_lens(self, lens, bound: int | None = None) -> None:
        """``lens[:] = lens``. A sequence or a CPU tensor gives the bound itself (its maximum); a device
        tensor is not read: pass ``bound`` (an upper bound of its entries, which the caller vouches for), or
        the present bound is kept, which the new values must not exceed."""
        if not isinstance(lens, torch.Tensor):
            lens = torch.as_tensor(lens, dtype=torch.int32)
        if lens.shape != (self.batch,):
            raise ValueError(f"KVCache.set_lens: expected {self.batch} lengths, got shape {tuple(lens.shape)}")
        if lens.device.type == "cpu":
            lo, hi = int(lens.min()), int(lens.max())
            if lo < 0 or hi > self.capacity or (bound is not None and hi > bound):
                raise ValueError(f"KVCache.set_lens: lengths in [{lo}, {hi}] do not fit capacity {self.capacity}"
                                 + (f" / the stated bound {bound}" if bound is not None else ""))
            bound = hi if bound is None else bound
        if bound is not None:
            if not 0 <= bound <= self.capacity:
                raise ValueError(f"KVCache.set_lens: bound {bound} outside [0, {self.capacity}]")
            self._bound = bound
        self.lens.copy_(lens.to(torch.int32))

    def require(self, n: int, table_len: int | None = None) -> None:
        """Refuse ``n`` more positions that might not fit the cache or the rotary table."""
        if self._bound + n > self.capacity:
            raise ValueError(f"KVCache: {n} more positions on top of up to {self._bound} exceed the capacity "
                             f"{self.capacity}")
        if table_len is not None and self._bound + n > table_len:
            raise ValueError(f"KVCache: {n} more positions on top of up to {self._bound} exceed the rotary "
                             f"table's {table_len} positions")

    def scratch(self, heads: int, S: int):
        """(o_part [B, heads, S, 64], ml_part [B, heads, S, 2]) fp32: allocated on the first request."""
        key = (heads, S)
        if key not in self._scratch:
            self._scratch[key] = (
                torch.empty(self.batch, heads, S, HEAD_DIM, device=self.device, dtype=torch.float32),
                torch.empty(self.batch, heads, S, 2, device=self.device, dtype=torch.float32))
        return self._scratch[key]
