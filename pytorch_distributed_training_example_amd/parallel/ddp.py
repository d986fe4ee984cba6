"""Bucketed, backward-overlapped data parallelism (``DistributedDataParallel``).

Reference: /root/reference/train.py:34-39 (``average_gradients``) averages gradients with one
blocking ``dist.all_reduce`` per parameter after ``loss.backward()`` returns, i.e. no
bucketing and no overlap (the comment at train.py:24 names DDP but it is never used).

This module is a from-scratch reducer with the ``torch.nn.parallel.DistributedDataParallel``
API surface (ctor kwargs, ``no_sync``, ``register_comm_hook``, ``module.``-prefixed
state_dict, rank-0 parameter/buffer broadcast) built for MI355X:

  * gradients live in flat per-bucket buffers (``gradient_as_bucket_view``) so a bucket is
    reduced with ONE RCCL call and the fused optimizers read it in place;
  * a post-accumulate-grad hook marks parameters ready; a bucket launches as soon as its
    last gradient exists, in bucket order on every rank (collective order must match
    across ranks), as an async RCCL all-reduce. c10d runs it on its own RCCL HIP stream,
    ordered after the producing kernels by an event, so it overlaps the rest of backward;
  * the 1/world averaging is done inside the collective (``ReduceOp.AVG``) on RCCL — no
    per-parameter ``div_`` kernels (the reference launches 10 per step, train.py:39);
  * at the end of backward (autograd engine callback) the compute stream waits on the
    outstanding collectives — the host never blocks, so the whole step can be captured in
    a hipGraph (engine/graph.py);
  * after the first iteration buckets are rebuilt in the order gradients actually
    became ready (rank 0's order is broadcast so all ranks agree);
  * optional ``reduce_dtype`` (e.g. reduce bf16 gradients in fp32) and comm hooks
    (bf16/fp16 compression, per-rank debugging);
  * ``join()``: ranks may run different numbers of iterations; a rank that ran out of data shadows the
    collectives of the ranks still training (torch's uneven-inputs semantics).
"""
from __future__ import annotations

import contextlib
import logging
import os
import warnings
from typing import Any, Callable, Dict, List, Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn as nn

from ..ops._native import cuda_available
from ..ops import multi_tensor
from ..ops.sync_batchnorm import SyncBatchNorm
from .debug import ReducerDebug
from .buckets import (AUTO_TAIL_BYTES, DEFAULT_BUCKET_CAP_MB, DEFAULT_FIRST_BUCKET_BYTES, BucketSpec,
                      compute_bucket_assignment, plan_auto)

log = logging.getLogger(__name__)


class GradBucket:
    """What a comm hook sees (mirrors ``torch.distributed.GradBucket``)."""

    def __init__(self, index: int, buffer: torch.Tensor, params: List[nn.Parameter],
                 views: List[torch.Tensor], is_last: bool):
        self._index = index
        self._buffer = buffer
        self._params = params
        self._views = views
        self._is_last = is_last

    def index(self) -> int:
        return self._index

    def buffer(self) -> torch.Tensor:
        return self._buffer

    def set_buffer(self, t: torch.Tensor) -> None:
        self._buffer.copy_(t)

    def gradients(self) -> List[torch.Tensor]:
        return self._views

    def parameters(self) -> List[nn.Parameter]:
        return self._params

    def is_last(self) -> bool:
        return self._is_last


def is_dense(t: torch.Tensor) -> bool:
    """True if ``t`` covers exactly ``numel`` consecutive elements (any dim order)."""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _strided_view(buffer: torch.Tensor, p: torch.Tensor, offset: int) -> torch.Tensor:
    if p.is_contiguous() or not is_dense(p):
        return buffer[offset:offset + p.numel()].view(p.shape)
    return torch.as_strided(buffer, p.shape, p.stride(), offset)


class _Bucket:
    def __init__(self, index: int, spec: BucketSpec, params: List[nn.Parameter],
                 reduce_dtype: Optional[torch.dtype]):
        self.index = index
        self.spec = spec
        self.params = params
        self.buffer = torch.zeros(spec.total, dtype=spec.dtype, device=spec.device)
        # Views keep the parameter's strides (e.g. channels_last conv weights), so autograd
        # accumulates into them without a layout-changing copy.
        self.views = [_strided_view(self.buffer, p, o) for p, o in zip(params, spec.offsets)]
        self.comm_buffer = self.buffer
        if reduce_dtype is not None and reduce_dtype != spec.dtype:
            self.comm_buffer = torch.zeros(spec.total, dtype=reduce_dtype, device=spec.device)
        self.pending = len(params)
        self.arrived = [False] * len(params)
        self.launched = False
        self.work: Any = None
        self.future: Any = None
        self.zero_slots: List[int] = []
        self.copy_src: List[torch.Tensor] = []
        self.copy_dst: List[torch.Tensor] = []
        self.copy_params: List[nn.Parameter] = []

    def reset(self) -> None:
        self.pending = len(self.params)
        self.arrived = [False] * len(self.params)
        self.launched = False
        self.work = None
        self.future = None


class _JoinState:
    """What one ``join()`` context carries (``DistributedDataParallel._join``)."""

    def __init__(self, divide_by_initial_world_size: bool, throw_on_early_termination: bool):
        self.divide_by_initial_world_size = divide_by_initial_world_size
        self.throw = throw_on_early_termination
        self.last: Optional[torch.Tensor] = None        # the last non-zero notify result (device)
        # divide_by_initial_world_size=False: device scalars from the notify result, applied to every
        # reduced bucket with the multi-tensor scale (never read on the host)
        self.rescale: Optional[torch.Tensor] = None     # world / active: after an average over world
        self.inv_active: Optional[torch.Tensor] = None  # 1 / active: after a plain SUM


def _default_avg_op(pg) -> tuple[Any, bool]:
    """(op, needs_divide). RCCL averages in-collective; gloo has no AVG.

    With ONE rank the average is the identity: SUM without a divide. RCCL runs an in-place
    single-rank SUM as a no-op, but AVG as a pre-multiply pass over every bucket (oneRankReduce:
    1.8 ms/step for GPT-2-medium's 710 MB of gradients) — torch DDP's pre-divided SUM also skips it.
    """
    if dist.get_world_size(pg) == 1:
        return dist.ReduceOp.SUM, False
    backend = dist.get_backend(pg)
    # pdt_p2p takes AVG for every tensor: P2P kernels, RCCL inner group, or SUM + divide when its
    # inner group is gloo (parallel/p2p.py P2PProcessGroup.allreduce)
    if backend in ("nccl", "pdt_p2p"):
        return dist.ReduceOp.AVG, False
    return dist.ReduceOp.SUM, True


class DistributedDataParallel(nn.Module):
    """Drop-in for ``torch.nn.parallel.DistributedDataParallel`` (single device per rank)."""

    def __init__(
        self,
        module: nn.Module,
        device_ids: Optional[Sequence[int]] = None,
        output_device: Optional[int] = None,
        dim: int = 0,
        broadcast_buffers: bool = True,
        init_sync: bool = True,
        process_group=None,
        bucket_cap_mb: Optional[float | str] = None,
        find_unused_parameters: bool = False,
        check_reduction: bool = False,
        gradient_as_bucket_view: bool = True,
        static_graph: bool = False,
        first_bucket_mb: Optional[float] = None,
        reduce_dtype: Optional[torch.dtype] = None,
        rebuild_buckets: bool = True,
        reduce_single_rank: bool = False,
        debug: Optional[bool] = None,
    ):
        super().__init__()
        self.module = module
        self.device_ids = list(device_ids) if device_ids is not None else None
        self.output_device = output_device
        self.dim = dim
        self.process_group = process_group if process_group is not None else (
            dist.group.WORLD if dist.is_initialized() else None)
        self.world_size = dist.get_world_size(self.process_group) if dist.is_initialized() else 1
        self.broadcast_buffers = broadcast_buffers
        self.find_unused_parameters = find_unused_parameters
        self.gradient_as_bucket_view = gradient_as_bucket_view
        self.static_graph = static_graph
        self.reduce_dtype = reduce_dtype
        # "auto": the comm-model plan (buckets.plan_auto) — the bucket that fills last is capped at
        # PDT_TAIL_BUCKET_MB (2 MiB) so the collective left after backward is short, earlier ones grow
        self._auto_plan = isinstance(bucket_cap_mb, str) and bucket_cap_mb.lower() == "auto"
        if isinstance(bucket_cap_mb, str) and not self._auto_plan:
            bucket_cap_mb = float(bucket_cap_mb)
        self._tail_bytes = int(float(os.environ.get("PDT_TAIL_BUCKET_MB", AUTO_TAIL_BYTES / 2 ** 20)) * 2 ** 20)
        self.bucket_bytes_cap = int((bucket_cap_mb if bucket_cap_mb is not None and not self._auto_plan
                                     else DEFAULT_BUCKET_CAP_MB) * 1024 * 1024)
        self.first_bucket_bytes = int(first_bucket_mb * 1024 * 1024) if first_bucket_mb is not None \
            else min(DEFAULT_FIRST_BUCKET_BYTES, self.bucket_bytes_cap)
        self.require_backward_grad_sync = True
        self._comm_hook: Optional[Callable] = None
        self._comm_hook_state: Any = None
        self._rebuild_enabled = rebuild_buckets and not static_graph
        # torch DDP packs buckets and issues the all-reduce even with ONE rank; ours skips that work
        # at world 1 unless asked (bench.py asks, so its N=1 point carries the same per-step
        # reducer work — pack copies, RCCL launch, stream joins — as N>1, and a captured step
        # holds a real collective)
        self.reduce_single_rank = bool(reduce_single_rank) and self.process_group is not None
        self._ready_order: List[int] = []
        self._rebuilt = False
        self._rebuild_pending = False
        self._callback_queued = False
        self._next_bucket = 0
        self._num_iterations = 0
        self._join: Optional[_JoinState] = None  # set inside a join() context only
        # exposed-communication timing (enable_comm_timing): per backward, events on the compute
        # stream at the start of _finalize_backward and after the last bucket's wait
        self._comm_timing = False
        self._comm_events: List[tuple] = []
        # per backward: (bucket index, event on the compute stream when the bucket launched)
        self._launch_events: List[tuple] = []
        self._lead_samples: List[List[tuple]] = []
        # debug mode (parallel/debug.py ReducerDebug): collective log + stream-safety assert + per-bucket
        # checksum across ranks after every backward; ``PDT_DDP_DEBUG=1`` turns it on without code changes
        if debug is None:
            debug = os.environ.get("PDT_DDP_DEBUG", "0") not in ("", "0")
        self._debug = ReducerDebug(self.process_group) if debug else None

        ignore = getattr(module, "_ddp_params_and_buffers_to_ignore", set())
        seen = set()
        self._params: List[nn.Parameter] = []
        self._param_names: List[str] = []
        for name, p in module.named_parameters():
            if not p.requires_grad or name in ignore or id(p) in seen:
                continue
            seen.add(id(p))
            self._params.append(p)
            self._param_names.append(name)
        self._buffers_to_sync = [b for n, b in module.named_buffers() if n not in ignore]
        if self.process_group is not None and (self.world_size > 1 or self.reduce_single_rank):
            self._avg_op, self._needs_div = _default_avg_op(self.process_group)
        else:
            self._avg_op, self._needs_div = None, False

        if init_sync and self.world_size > 1:
            self._sync_module_states()
        self._build_buckets(order=None)
        self._hook_handles = [p.register_post_accumulate_grad_hook(self._make_hook(i))
                              for i, p in enumerate(self._params)]

    # ------------------------------------------------------------------ setup
    def _sync_module_states(self, src: int = 0) -> None:
        """Broadcast rank ``src``'s (default: rank 0's) parameters and buffers (coalesced by dtype).

        The reference relies on every rank using the same seed (train.py:80-81) and never
        broadcasts; a broadcast makes replicas identical regardless of init RNG.
        """
        tensors = [p.data for p in self.module.parameters()] + list(self._buffers_to_sync)
        self._broadcast_coalesced(tensors, src=src)

    def _broadcast_coalesced(self, tensors: List[torch.Tensor], bucket_bytes: int = 256 << 20, src: int = 0) -> None:
        """``src``: the sending rank within the process group (rank 0 unless a join() context names another)."""
        by_key: Dict[Any, List[torch.Tensor]] = {}
        for t in tensors:
            if t.numel() == 0:
                continue
            by_key.setdefault((t.dtype, t.device), []).append(t)
        for _, ts in by_key.items():
            chunk: List[torch.Tensor] = []
            size = 0
            for t in ts + [None]:  # type: ignore[list-item]
                if t is not None:
                    chunk.append(t)
                    size += t.numel() * t.element_size()
                if chunk and (t is None or size >= bucket_bytes):
                    flat = torch.cat([c.reshape(-1) for c in chunk])
                    dist.broadcast(flat, src=dist.get_global_rank(self.process_group, src)
                                   if self.process_group not in (None, dist.group.WORLD) else src,
                                   group=self.process_group)
                    off = 0
                    for c in chunk:
                        c.copy_(flat[off:off + c.numel()].view_as(c))
                        off += c.numel()
                    chunk, size = [], 0

    def _build_buckets(self, order: Optional[List[int]]) -> None:
        if self._auto_plan:
            specs = plan_auto(self._params, self.bucket_bytes_cap, self._tail_bytes, order=order)
        else:
            specs = compute_bucket_assignment(self._params, self.bucket_bytes_cap,
                                              self.first_bucket_bytes, order=order)
        old_grads = {i: p.grad for i, p in enumerate(self._params)}
        self._buckets: List[_Bucket] = []
        self._param_loc: Dict[int, tuple[int, int]] = {}
        for b, spec in enumerate(specs):
            params = [self._params[i] for i in spec.indices]
            bucket = _Bucket(b, spec, params, self.reduce_dtype)
            for j, i in enumerate(spec.indices):
                self._param_loc[i] = (b, j)
            self._buckets.append(bucket)
        if self.gradient_as_bucket_view:
            for i, p in enumerate(self._params):
                b, j = self._param_loc[i]
                view = self._buckets[b].views[j]
                g = old_grads[i]
                if g is not None:
                    view.copy_(g)
                    p.grad = view

    def bucket_specs(self) -> List[BucketSpec]:
        return [b.spec for b in self._buckets]

    # ------------------------------------------------------------------ hooks
    def _make_hook(self, index: int) -> Callable:
        def hook(param: torch.Tensor) -> None:
            self._on_grad_ready(index, param)
        return hook

    def _active(self) -> bool:
        """Buckets/collectives are only needed with >1 rank, a comm hook, or ``reduce_single_rank``."""
        return self.world_size > 1 or self._comm_hook is not None or self.reduce_single_rank

    def _on_grad_ready(self, index: int, param: torch.Tensor) -> None:
        if not self.require_backward_grad_sync or not self._active():
            return
        if not self._callback_queued:
            self._callback_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._finalize_backward)
        if self._rebuild_enabled and not self._rebuilt:
            self._ready_order.append(index)
        b, j = self._param_loc[index]
        bucket = self._buckets[b]
        if bucket.arrived[j]:
            return
        g = param.grad
        view = bucket.views[j]
        if g is None:
            bucket.zero_slots.append(j)
        elif g.data_ptr() != view.data_ptr():
            # autograd stole a fresh gradient tensor: pack it into the bucket together with the
            # bucket's other stolen grads in ONE multi-tensor copy at launch time
            bucket.copy_src.append(g)
            bucket.copy_dst.append(view)
            bucket.copy_params.append(param)
        bucket.arrived[j] = True
        bucket.pending -= 1
        self._launch_ready_buckets()

    def _launch_ready_buckets(self) -> None:
        while self._next_bucket < len(self._buckets) and self._buckets[self._next_bucket].pending == 0:
            self._launch(self._buckets[self._next_bucket])
            self._next_bucket += 1

    def _pack(self, bucket: _Bucket) -> None:
        for j in bucket.zero_slots:
            bucket.views[j].zero_()
            if self.gradient_as_bucket_view:
                bucket.params[j].grad = bucket.views[j]
        if bucket.copy_src:
            multi_tensor.copy_(bucket.copy_src, bucket.copy_dst)
            if self.gradient_as_bucket_view:
                for p, v in zip(bucket.copy_params, bucket.copy_dst):
                    p.grad = v
        bucket.zero_slots, bucket.copy_src, bucket.copy_dst, bucket.copy_params = [], [], [], []

    def _launch(self, bucket: _Bucket) -> None:
        bucket.launched = True
        self._pack(bucket)
        if self._comm_timing and cuda_available() and not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()  # the compute stream's position when this bucket's gradients are complete
            self._launch_events.append((bucket.index, ev))
        if bucket.comm_buffer is not bucket.buffer:
            multi_tensor.copy_([bucket.buffer], [bucket.comm_buffer])
        if self._debug is not None:
            self._debug.on_launch(bucket.index, bucket.comm_buffer,
                                  "comm_hook" if self._comm_hook is not None else "all_reduce")
        if self._comm_hook is not None:
            gb = GradBucket(bucket.index, bucket.comm_buffer, bucket.params, bucket.views,
                            bucket.index == len(self._buckets) - 1)
            bucket.future = self._comm_hook(self._comm_hook_state, gb)
            return
        bucket.work = dist.all_reduce(bucket.comm_buffer, op=self._avg_op,
                                      group=self.process_group, async_op=True)

    def _finalize_backward(self) -> None:
        timing = self._comm_timing and cuda_available() and not torch.cuda.is_current_stream_capturing()
        if timing:  # backward's compute is all queued: from here the compute stream waits on comm
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        # Parameters that did not take part in this backward (unused / frozen branch)
        # contribute zeros so every rank launches the same collectives in the same order.
        for bucket in self._buckets:
            if bucket.pending > 0:
                for j, arrived in enumerate(bucket.arrived):
                    if not arrived:
                        bucket.zero_slots.append(j)
                        bucket.arrived[j] = True
                bucket.pending = 0
        self._launch_ready_buckets()
        works = [(b.index, b.future if b.future is not None else b.work) for b in self._buckets] \
            if self._debug is not None else None
        # join(divide_by_initial_world_size=False): divide by the ranks still active instead of the world
        rescale = self._join.rescale if self._join is not None else None
        for bucket in self._buckets:
            if bucket.future is not None:
                out = bucket.future.wait()
                if isinstance(out, (list, tuple)):
                    out = out[0]
                if out is not None and out.data_ptr() != bucket.buffer.data_ptr():
                    bucket.buffer.copy_(out.view(-1)[: bucket.buffer.numel()])
                if rescale is not None:  # the hook averaged over the world
                    multi_tensor.scale_([bucket.buffer], rescale)
            elif bucket.work is not None:
                bucket.work.wait()  # stream-ordered: compute stream waits on the RCCL stream
                if self._needs_div:
                    if rescale is not None:
                        multi_tensor.scale_([bucket.comm_buffer], self._join.inv_active)
                    else:
                        bucket.comm_buffer.div_(self.world_size)
                elif rescale is not None:  # ReduceOp.AVG divided by the world
                    multi_tensor.scale_([bucket.comm_buffer], rescale)
                if bucket.comm_buffer is not bucket.buffer:
                    multi_tensor.copy_([bucket.comm_buffer], [bucket.buffer])
            if not self.gradient_as_bucket_view:
                for p, v in zip(bucket.params, bucket.views):
                    if p.grad is None:
                        p.grad = v.clone()
                    elif p.grad.data_ptr() != v.data_ptr():
                        p.grad.copy_(v)
            bucket.reset()
        if works is not None:  # every bucket reduced and unpacked: the optimizer reads them next
            self._debug.after_backward(works, [b.buffer for b in self._buckets],
                                       [[self._param_names[i] for i in b.spec.indices] for b in self._buckets])
        if timing:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self._comm_events.append((e0, e1))
            self._lead_samples.append([(i, ev, e0) for i, ev in self._launch_events])
        self._launch_events = []
        self._next_bucket = 0
        self._callback_queued = False
        self._num_iterations += 1
        if self._rebuild_enabled and not self._rebuilt:
            self._rebuild_pending = True

    def _maybe_rebuild(self) -> None:
        if not self._rebuild_pending:
            return
        self._rebuild_pending = False
        self._rebuilt = True
        order = list(dict.fromkeys(self._ready_order))
        order += [i for i in range(len(self._params)) if i not in set(order)]
        if self.world_size > 1:
            obj = [order]
            dist.broadcast_object_list(obj, src=0, group=self.process_group)
            order = obj[0]
        self._build_buckets(order=order)

    # ------------------------------------------------------------------ API
    def forward(self, *inputs, **kwargs):
        src = 0 if self._join is None else self._join_pre_forward()
        if torch.is_grad_enabled() and self.require_backward_grad_sync:
            self._maybe_rebuild()
        if self.broadcast_buffers and self.world_size > 1 and self._buffers_to_sync:
            self._broadcast_coalesced(list(self._buffers_to_sync), src=src)
        return self.module(*inputs, **kwargs)

    # ------------------------------------------------------------------ uneven inputs (join)
    def _join_notify(self, active: bool, sync: bool) -> torch.Tensor:
        """All-reduce (SUM) the notify tensor: ``world + 1`` fp32 elements, element r = 1 if rank r is active,
        the last = 1 if this iteration's backward synchronises gradients. A joined rank sends zeros. Adding
        zeros is exact (the one-row-per-rank exchange of ops/sync_batchnorm.py), so from the one result every
        rank knows the active count, the highest active rank and whether anyone syncs."""
        js, w = self._join, self.world_size
        row = [0.0] * (w + 1)
        if active:
            row[dist.get_rank(self.process_group)] = 1.0
            row[w] = 1.0 if sync else 0.0
        dev = self._buckets[0].buffer.device if self._buckets else torch.device("cpu")
        t = torch.tensor(row, dtype=torch.float32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.process_group)
        if active and not js.divide_by_initial_world_size:
            n = t[:w].sum().reshape(1)  # >= 1: this rank is in it
            js.inv_active = torch.reciprocal(n)
            js.rescale = float(w) / n
        return t

    def _join_pre_forward(self) -> int:
        """An active rank's forward inside join(): notify; returns the rank whose buffers are broadcast (the
        highest active rank: a joined rank 0's running statistics are stale). The result is read on the host
        only where a value from it is needed here."""
        js, w = self._join, self.world_size
        t = self._join_notify(True, torch.is_grad_enabled() and self.require_backward_grad_sync)
        js.last = t
        need_src = self.broadcast_buffers and bool(self._buffers_to_sync)
        if not (js.throw or need_src):
            return 0
        v = t.tolist()
        if js.throw and sum(x > 0 for x in v[:w]) < w:
            raise RuntimeError("Detected at least one rank that exhausted inputs. Throwing across all ranks.")
        return max(r for r in range(w) if v[r] > 0)

    def _join_shadow(self) -> None:
        """A joined rank: until no rank is active, issue the collectives of one active iteration (same order,
        sizes and dtypes) through the real code paths, contributing zero gradients."""
        js, w = self._join, self.world_size
        while True:
            t = self._join_notify(False, False)
            v = t.tolist()
            active = sum(x > 0 for x in v[:w])
            if active == 0:
                return
            if js.throw:
                raise RuntimeError(f"Rank {dist.get_rank(self.process_group)} exhausted all inputs.")
            js.last = t
            if not js.divide_by_initial_world_size:  # the same scaling as the active ranks (debug checksums)
                n = t[:w].sum().reshape(1)
                js.inv_active = torch.reciprocal(n)
                js.rescale = float(w) / n
            sync = v[w] > 0
            if sync:
                self._maybe_rebuild()
            if self.broadcast_buffers and self._buffers_to_sync:
                self._broadcast_coalesced(list(self._buffers_to_sync), src=max(r for r in range(w) if v[r] > 0))
            if sync:
                for b in self._buckets:
                    b.buffer.zero_()
                    b.arrived = [True] * len(b.params)
                    b.pending = 0
                    b.zero_slots, b.copy_src, b.copy_dst, b.copy_params = [], [], [], []
                self._launch_ready_buckets()
                self._finalize_backward()

    def _join_final_sync(self) -> None:
        """Every rank has seen the last non-zero notify vector; the highest rank in it took every step:
        broadcast its parameters and buffers."""
        js, w = self._join, self.world_size
        if js.last is None:  # no rank ran a step
            return
        v = js.last.tolist()
        self._sync_module_states(src=max(r for r in range(w) if v[r] > 0))

    @contextlib.contextmanager
    def join(self, divide_by_initial_world_size: bool = True, enable: bool = True,
             throw_on_early_termination: bool = False):
        """Train through uneven inputs (``torch.nn.parallel.DistributedDataParallel.join``): inside the
        context each rank may run a different number of iterations, zero included.

        Every forward of an active rank first all-reduces a ``world + 1`` element notify tensor. A rank that
        leaves the body normally shadows the others: per remaining iteration it joins the notify, the bucket
        rebuild broadcast, the buffer broadcast (from the highest active rank) and, with zero gradients,
        every bucket's reduction (comm hooks, ``reduce_dtype`` and debug mode included), until no rank is
        active. Then the last joiner's parameters and buffers are broadcast, so every replica ends with the
        model that took every step. Optimizer state on ranks that joined early stays one or more steps
        behind, as in torch; synchronise it yourself if training continues on those ranks.

        ``divide_by_initial_world_size``: True averages over the initial world size (a joined rank counts
        as a zero gradient); False divides by the number of ranks still active.
        ``throw_on_early_termination``: raise ``RuntimeError`` on every rank as soon as one rank has joined.
        ``enable=False``, one rank or no process group: a no-op without any collective.

        Refused (``RuntimeError`` at entry): a module containing ``SyncBatchNorm`` (its forward collectives
        cannot be shadowed) and entering during a stream capture. A rank that leaves the body through an
        exception does not shadow; the exception propagates."""
        if not enable or self.process_group is None or self.world_size == 1:
            yield
            return
        if self._join is not None:
            raise RuntimeError("join() is already active on this DistributedDataParallel")
        if any(isinstance(m, SyncBatchNorm) for m in self.module.modules()):
            raise RuntimeError("join() does not support a module containing SyncBatchNorm: its forward "
                               "statistics exchange is a collective a joined rank cannot shadow")
        if cuda_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("join() cannot be entered while a stream capture is in progress: a joined rank "
                               "shadows collectives from the host")
        self._join = _JoinState(bool(divide_by_initial_world_size), bool(throw_on_early_termination))
        try:
            yield
            self._join_shadow()
            self._join_final_sync()
        finally:
            self._join = None

    @contextlib.contextmanager
    def no_sync(self):
        """Accumulate gradients locally (into the bucket buffers) without communicating."""
        old = self.require_backward_grad_sync
        self.require_backward_grad_sync = False
        try:
            yield
        finally:
            self.require_backward_grad_sync = old

    def enable_comm_timing(self, on: bool = True) -> None:
        """Time the EXPOSED communication of each backward: GPU time between the end of backward's
        compute (the start of the finalize callback, where the last buckets launch) and the moment
        the compute stream may proceed past every bucket's all-reduce (the waits + unpack copies).
        Communication hidden under backward does not count; a reducer with no overlap shows its
        whole all-reduce time here. Events only, no host sync until ``comm_exposed_ms``."""
        self._comm_timing = bool(on)
        self._comm_events = []
        self._launch_events = []
        self._lead_samples = []

    def comm_exposed_ms(self, reset: bool = True) -> Optional[float]:
        """Mean exposed-communication ms per timed backward (synchronises); None if none timed."""
        ev = self._comm_events
        if reset:
            self._comm_events = []
        if not ev:
            return None
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def bucket_ready_lead_ms(self, reset: bool = True) -> Optional[List[float]]:
        """Per bucket (launch order): mean GPU time between the point in the compute stream where the
        bucket's collective could start (all of its gradients produced and packed) and the end of
        backward's compute. > 0 means the all-reduce had that long to run under backward; the bucket
        that fills last has ~0. Meaningful at N=1 too (the collective itself is not timed), so it
        shows whether the bucket ORDER lets communication overlap. Synchronises."""
        samples = self._lead_samples
        if reset:
            self._lead_samples = []
        if not samples:
            return None
        torch.cuda.synchronize()
        acc: Dict[int, List[float]] = {}
        for per_bwd in samples:
            for i, ev, e0 in per_bwd:
                acc.setdefault(i, []).append(ev.elapsed_time(e0))
        return [sum(v) / len(v) for _, v in sorted(acc.items())]

    def bucket_bytes(self) -> List[int]:
        """Bytes of each gradient bucket, in launch order."""
        return [b.comm_buffer.numel() * b.comm_buffer.element_size() for b in self._buckets]

    def register_comm_hook(self, state: Any, hook: Callable) -> None:
        if self._comm_hook is not None:
            raise RuntimeError("register_comm_hook can only be called once")
        self._comm_hook_state = state
        self._comm_hook = hook

    def zero_grad(self, set_to_none: bool = True) -> None:
        """set_to_none (default): autograd then steals fresh gradients and the reducer packs
        them with one multi-tensor copy per bucket — cheaper than zeroing + accumulating."""
        if set_to_none:
            for p in self._params:
                p.grad = None
        else:
            self.zero_grad_buckets()

    def zero_grad_buckets(self) -> None:
        """Zero all flat gradient buckets with one memset each (keeps grads as views)."""
        for b in self._buckets:
            b.buffer.zero_()
        if self.gradient_as_bucket_view:
            for b in self._buckets:
                for p, v in zip(b.params, b.views):
                    p.grad = v

    def grad_buffers(self) -> List[torch.Tensor]:
        return [b.buffer for b in self._buckets]

    def parameters_and_views(self):
        for b in self._buckets:
            yield from zip(b.params, b.views)

    def __getattr__(self, name: str):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.module, name)

    def __del__(self):
        for h in getattr(self, "_hook_handles", []):
            try:
                h.remove()
            except Exception:
                pass


def unwrap(model: nn.Module) -> nn.Module:
    """Strip a DDP wrapper (ours or torch's)."""
    return model.module if hasattr(model, "module") and isinstance(
        model, (DistributedDataParallel, torch.nn.parallel.DistributedDataParallel)) else model
