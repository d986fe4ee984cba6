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

The fp32 scratch of the split-KV partials belongs to the cache too: ``scratch(heads, S, tokens)`` allocates once
per (heads, S, tokens) and hands the same tensors back on every later step. The batch is fixed for the life of
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
        if dtype == torch.float8_e4m3fn:
            raise NotImplementedError("KVCache: an fp8 contiguous cache is out of scope; the e4m3 cache is the paged one "
                                      "(PagedKVCache(..., dtype=torch.float8_e4m3fn))")
        self.n_layer, self.batch, self.kv_heads, self.capacity = n_layer, batch, kv_heads, capacity
        self.device, self.dtype = torch.device(device), dtype
        shape = (batch, kv_heads, capacity, HEAD_DIM)
        self.k = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.v = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.lens = torch.zeros(batch, device=self.device, dtype=torch.int32)
        self._bound = 0  # host-side upper bound of lens
        self._scratch: dict = {}
        self.extending = False  # set by Llama.extend around its forward: Tn > 1 then runs the append kernel

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

    def scratch(self, heads: int, S: int, tokens: int = 1):
        """(o_part [B, heads, S, 64], ml_part [B, heads, S, 2]) fp32: allocated on the first request. With
        ``tokens`` > 1 (a multi-token append) the shapes are [B, tokens, heads, S, 64] and [B, tokens, heads, S, 2]."""
        key = (heads, S) if tokens == 1 else (heads, S, tokens)
        if key not in self._scratch:
            lead = (self.batch,) if tokens == 1 else (self.batch, tokens)
            self._scratch[key] = (
                torch.empty(*lead, heads, S, HEAD_DIM, device=self.device, dtype=torch.float32),
                torch.empty(*lead, heads, S, 2, device=self.device, dtype=torch.float32))
        return self._scratch[key]


PAGE = 64


class PagedKVCache:
    """A KV cache in pages of 64 positions (csrc/kernels/attn_paged.hip reads and writes it).

    Per layer ``k[l]`` and ``v[l]`` are pools [n_pages, Hkv, 64, 64] shared by ``slots`` sequence slots;
    ``block_table`` (int32 [slots, max_pages_per_seq], on the device, one for all layers) names the page of
    positions [64 j, 64 j + 64) of a slot, or -1. ``lens`` and ``active`` are int32 [slots] on the device. A slot
    holds only the pages its sequence has reached, a finished sequence gives them back (``free``) and a new one
    joins (``admit``, then ``Llama.prefill(..., slots=[s])``) while the others decode.

    The allocator lives on the host: a mirror of the table, a free list and, per slot, an upper bound of
    ``lens`` kept without a device read, as ``KVCache.bound`` is. ``reserve(n)`` gives every active slot the
    pages ``bound + n`` positions need, before the step that writes them, and uploads the table only when an
    entry changed (in steady decoding once per 64 steps and slot); it raises before it changes or launches
    anything when the pool, ``max_pages_per_seq`` or the rotary table (``table_len``) cannot cover the step.
    Nothing on the step path reads the device, so a captured decode step replays with ``reserve`` called
    between the replays. Freed pages are not cleared: the kernels never read a row at or past ``lens``.

    With ``dtype=torch.float8_e4m3fn`` (csrc/kernels/attn_paged_fp8.hip) the pools hold one byte per element, a key
    row is one 64-byte line, and ``k_scale[l]`` / ``v_scale[l]`` (fp32 [n_pages, Hkv, 64]) hold one scale per stored
    (position, K/V head) row: the row is ``quantize_rows_e4m3``'s of the row the bf16 cache would store, and the
    attention runs on ``float(k) * k_scale[row]``, ``float(v) * v_scale[row]``. Table, ``lens``, ``active``, the
    allocator and the scratch mean what they mean above; freed pages and their scales are not cleared either."""

    def __init__(self, n_layer: int, slots: int, kv_heads: int, n_pages: int, max_pages_per_seq: int, device,
                 dtype=torch.bfloat16):
        if min(n_layer, slots, kv_heads, n_pages, max_pages_per_seq) <= 0:
            raise ValueError("PagedKVCache: n_layer, slots, kv_heads, n_pages and max_pages_per_seq must be positive, "
                             f"got {(n_layer, slots, kv_heads, n_pages, max_pages_per_seq)}")
        self.n_layer, self.slots, self.kv_heads = n_layer, slots, kv_heads
        self.n_pages, self.max_pages = n_pages, max_pages_per_seq
        self.device, self.dtype = torch.device(device), dtype
        shape = (n_pages, kv_heads, PAGE, HEAD_DIM)
        self.k = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.v = [torch.zeros(shape, device=self.device, dtype=dtype) for _ in range(n_layer)]
        self.k_scale = self.v_scale = None
        if self.fp8:
            self.k_scale = [torch.zeros(shape[:3], device=self.device, dtype=torch.float32) for _ in range(n_layer)]
            self.v_scale = [torch.zeros(shape[:3], device=self.device, dtype=torch.float32) for _ in range(n_layer)]
        self.block_table = torch.full((slots, max_pages_per_seq), -1, device=self.device, dtype=torch.int32)
        self.lens = torch.zeros(slots, device=self.device, dtype=torch.int32)
        self.active = torch.zeros(slots, device=self.device, dtype=torch.int32)
        self.table_len: int | None = None  # positions of the rotary table, when the owner has one
        self._table = torch.full((slots, max_pages_per_seq), -1, dtype=torch.int32)  # host mirror
        self._free = list(range(n_pages - 1, -1, -1))  # popped from the end: page 0 first
        self._held = [0] * slots  # pages a slot holds: the first _held[s] entries of its table row
        self._bound = [0] * slots
        self._active = [False] * slots
        self._scratch: dict = {}
        self._view = None  # (block_table rows, lens) of the slots a prefill or an extend runs on
        self.extending = False  # set by Llama.extend around its forward: Tn > 1 then runs the paged append kernel

    # ------------------------------------------------------------------ what the contiguous cache also answers
    @property
    def fp8(self) -> bool:
        """An e4m3 cache: byte pools with ``k_scale`` / ``v_scale`` beside them."""
        return self.dtype == torch.float8_e4m3fn

    @property
    def batch(self) -> int:
        return self.slots

    @property
    def capacity(self) -> int:
        return self.max_pages * PAGE

    @property
    def bound(self) -> int:
        """An upper bound of every entry of ``lens``, known without reading the device."""
        return max(self._bound)

    @property
    def bounds(self) -> list:
        return list(self._bound)

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages_of(self, slot: int) -> list:
        return self._table[slot, :self._held[slot]].tolist()

    def is_active(self, slot: int) -> bool:
        return self._active[slot]

    # ------------------------------------------------------------------ slots
    def _slot(self, slot: int) -> int:
        if not 0 <= int(slot) < self.slots:
            raise ValueError(f"PagedKVCache: slot {slot} outside [0, {self.slots})")
        return int(slot)

    def admit(self, slot: int) -> None:
        """Open ``slot`` for a new sequence: active, empty, no pages yet (``reserve`` hands them out)."""
        slot = self._slot(slot)
        if self._active[slot]:
            raise ValueError(f"PagedKVCache.admit: slot {slot} is in use (free it first)")
        self._active[slot] = True
        self._bound[slot] = 0
        self.active[slot] = 1
        self.lens[slot] = 0

    def free(self, slot: int) -> None:
        """Return the slot's pages to the free list (uncleared), its table row to -1, its lens and active to 0."""
        slot = self._slot(slot)
        held = self._held[slot]
        self._free.extend(reversed(self._table[slot, :held].tolist()))
        self._table[slot] = -1
        self._held[slot], self._bound[slot], self._active[slot] = 0, 0, False
        self.active[slot] = 0
        self.lens[slot] = 0
        if held:
            self.block_table.copy_(self._table)

    def _named(self, slots) -> list:
        if slots is None:
            return [s for s in range(self.slots) if self._active[s]]
        named = [self._slot(s) for s in slots]
        if len(set(named)) != len(named) or not all(self._active[s] for s in named):
            raise ValueError(f"PagedKVCache: slots {list(slots)} must be distinct admitted slots")
        return named

    def reserve(self, n: int = 1, slots=None) -> None:
        """Before a step of ``n`` tokens: every named slot (default: every active one) gets the pages that
        ``ceil((bound + n) / 64)`` needs. Raises, with nothing changed, when the free list, ``max_pages_per_seq``
        or the rotary table cannot cover it."""
        named = self._named(slots)
        need = {}
        for s in named:
            end = self._bound[s] + n
            if self.table_len is not None and end > self.table_len:
                raise ValueError(f"PagedKVCache: {n} more positions on top of up to {self._bound[s]} in slot {s} exceed "
                                 f"the rotary table's {self.table_len} positions")
            pages = -(-end // PAGE)
            if pages > self.max_pages:
                raise ValueError(f"PagedKVCache: {n} more positions on top of up to {self._bound[s]} in slot {s} need "
                                 f"{pages} pages, more than max_pages_per_seq = {self.max_pages}")
            need[s] = max(pages - self._held[s], 0)
        total = sum(need.values())
        if total > len(self._free):
            raise ValueError(f"PagedKVCache: the step needs {total} more pages and the pool has {len(self._free)} free "
                             f"of {self.n_pages}")
        if total == 0:
            return
        for s, k in need.items():
            for _ in range(k):
                self._table[s, self._held[s]] = self._free.pop()
                self._held[s] += 1
        self.block_table.copy_(self._table)

    def require(self, n: int, table_len: int | None = None, slots=None) -> None:
        """Refuse ``n`` more positions that the named slots' pages (``reserve`` was not called) or the rotary
        table might not hold."""
        for s in self._named(slots):
            end = self._bound[s] + n
            if end > self._held[s] * PAGE:
                raise ValueError(f"PagedKVCache: {n} more positions on top of up to {self._bound[s]} in slot {s} exceed "
                                 f"its {self._held[s]} pages: call reserve({n}) before the step")
            if table_len is not None and end > table_len:
                raise ValueError(f"PagedKVCache: {n} more positions on top of up to {self._bound[s]} in slot {s} exceed "
                                 f"the rotary table's {table_len} positions")

    # ------------------------------------------------------------------ lens
    def advance(self, n: int = 1, slots=None) -> None:
        """``lens += n * active`` on the device; the bounds of the active slots follow. With ``slots`` (distinct
        admitted slots) only those move."""
        if slots is None:
            self.lens.add_(self.active, alpha=n)
            named = [s for s in range(self.slots) if self._active[s]]
        else:
            named = self._named(slots)
            self.lens.index_add_(0, torch.as_tensor(named, device=self.device),
                                 torch.full((len(named),), n, device=self.device, dtype=torch.int32))
        for s in named:
            self._bound[s] += n

    def set_lens(self, lens, bound=None, slots=None) -> None:
        """``lens[slots] = lens`` (default: all slots). ``KVCache.set_lens``'s contract per slot: a sequence or a
        CPU tensor gives the bounds itself; a device tensor is not read: pass ``bound`` (an int for every named
        slot, or one per slot, which the caller vouches for), or the present bounds are kept, which the new
        values must not exceed."""
        named = list(range(self.slots)) if slots is None else [self._slot(s) for s in slots]
        if not isinstance(lens, torch.Tensor):
            lens = torch.as_tensor(lens, dtype=torch.int32)
        if lens.shape != (len(named),):
            raise ValueError(f"PagedKVCache.set_lens: expected {len(named)} lengths, got shape {tuple(lens.shape)}")
        if bound is not None and not isinstance(bound, (list, tuple)):
            bound = [int(bound)] * len(named)
        if lens.device.type == "cpu":
            vals = [int(x) for x in lens.tolist()]
            if bound is None:
                bound = vals
            if min(vals) < 0 or any(v > b for v, b in zip(vals, bound)):
                raise ValueError(f"PagedKVCache.set_lens: lengths {vals} are negative or exceed the stated bounds {bound}")
        if bound is not None:
            if len(bound) != len(named) or any(not 0 <= b <= self._held[s] * PAGE for s, b in zip(named, bound)):
                raise ValueError(f"PagedKVCache.set_lens: bounds {list(bound)} do not fit the pages the slots hold "
                                 f"({[self._held[s] for s in named]})")
            for s, b in zip(named, bound):
                self._bound[s] = int(b)
        lens = lens.to(device=self.device, dtype=torch.int32)
        if slots is None:
            self.lens.copy_(lens)
        else:
            self.lens.index_copy_(0, torch.as_tensor(named, device=self.device), lens)

    # ------------------------------------------------------------------ what a forward runs on
    def select(self, slots) -> None:
        """The slots the next forward's rows are (a prefill of newly admitted slots), or None for all of them."""
        if slots is None:
            self._view = None
        else:
            idx = torch.as_tensor(self._named(slots), device=self.device)
            self._view = (self.block_table.index_select(0, idx).contiguous(), self.lens.index_select(0, idx), list(slots))

    def view(self):
        """(block_table rows, lens, slots or None) of the slots the forward runs on."""
        return self._view if self._view is not None else (self.block_table, self.lens, None)

    def scratch(self, heads: int, S: int, tokens: int = 1):
        """(o_part [slots, heads, S, 64], ml_part [slots, heads, S, 2]) fp32: allocated on the first request. With
        ``tokens`` > 1 (a multi-token append) the shapes are [slots, tokens, heads, S, 64] and [slots, tokens, heads,
        S, 2], as ``KVCache.scratch``'s; a call on fewer rows than ``slots`` uses the leading rows."""
        key = (heads, S) if tokens == 1 else (heads, S, tokens)
        if key not in self._scratch:
            lead = (self.slots,) if tokens == 1 else (self.slots, tokens)
            self._scratch[key] = (
                torch.empty(*lead, heads, S, HEAD_DIM, device=self.device, dtype=torch.float32),
                torch.empty(*lead, heads, S, 2, device=self.device, dtype=torch.float32))
        return self._scratch[key]
