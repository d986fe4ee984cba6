"""Linear layer with the bias gradient on the column-strip HIP kernel (csrc/kernels/gelu.hip).

Forward is one hipBLASLt GEMM with the bias fused in its epilogue (``F.linear``). Backward is the
two library GEMMs (dX = dY·W, dW = dYᵀ·X) plus ``colsum`` for dbias — aten would reduce dY with a
generic ``sum(0)`` reduction kernel, which streams a [tokens, D] bf16 gradient at a fraction of
HBM rate (profiles/r1_steady_gpt2_medium_ours.md: 73 ``reduce_kernel`` calls, 1.6 ms/step).

Forward GEMMs on our MFMA kernel (csrc/kernels/gemm.hip: bias epilogue, and the MLP's fc1 + bias + GELU in
one pass, ``linear_gelu``) are chosen PER SHAPE by measurement, as the 1x1 convs are (ops/conv.py _pick):
``PDT_LINEAR_EPILOGUE=auto`` (default) looks the (kind, M, N, K) up in ``tuning/linear_gfx950.json`` (decided by
whole-step A/B); a shape not in the table runs the library. ``=time`` times an unlisted shape once (eager steps
only) against hipBLASLt (+ our bias+GELU kernel for the fused kind) and caches the winner — isolated timings
mispredict the step (GPT-2-medium lost 3 % on them), hence not the default. Our kernel wins on
some shapes only (vit_qkv 1.08x, vit_fc2 1.03x, gpt2_proj + bias 1.05x; 0.61-0.94x on the others:
profiles/r5/gemm_bn128.txt, profiles/r3/gemm_vs_hipblaslt.md), so all-or-nothing would lose. ``=1``: ours
on every shape it serves, ``=0``: never. ``PDT_LINEAR_DUMP=path`` writes the decisions at exit.

Inference on at most 64 rows (a decode step, a short extend) has a kernel of its own, ``linear_skinny``
(csrc/kernels/gemm_skinny.hip): the weights stream once from memory to the matrix cores' registers, optionally
with SwiGLU applied to ``c_fc``'s packed gate/up output in the same launch. The Llama decoder uses it under
``PDT_DECODE_GEMM=1`` (default 0). ``quantize_rows_e4m3`` + ``linear_skinny_w8`` are the same Linears on weights
stored as e4m3 bytes with one fp32 scale per output feature (csrc/kernels/gemm_skinny_w8.hip): half the bytes to
stream; ``Llama.quantize_decode_weights()`` opts a model in. ``quantize_groups_int4`` + ``linear_skinny_w4`` store
symmetric int4 with one fp32 scale per 128 inputs in a layout packed for the kernel
(csrc/kernels/gemm_skinny_w4.hip; ``pack_int4`` defines it): a quarter of the bytes plus the scales;
``Llama.quantize_decode_weights("int4")``. ``linear_w4`` serves the same int4 operands at any row count: above 64
rows a tiled, compute-bound kernel of its own (csrc/kernels/gemm_w4.hip);
``Llama.quantize_decode_weights("int4", all_rows=True)``.
"""
from __future__ import annotations

import atexit
import json
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from ..config import SW
from ._native import native, use_native

# weight gradient dW = dY^T X sums over all tokens (K = 6K-25K): one hipBLASLt GEMM leaves most of
# the chip idle on the ViT/GPT-2 shapes (27-36 output tiles of 256x256); split-K batched GEMMs
# over token slices + an fp32-accumulated sum measured 0.5-0.9x of its time
# (tools/linear_wgrad_bench.py). The slice count is timed once per shape (eager steps; a shape
# first seen under hipGraph capture keeps the single GEMM). PDT_LINEAR_SPLITK=0: single GEMM.
_WG_CHOICE: Dict[Tuple, int] = {}


def _wgrad(dy2: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    from .conv import _wgrad_splitk
    T = dy2.shape[0]
    if not SW.linear_splitk or not dy2.is_cuda:
        return dy2.t() @ x2
    key = (T, dy2.shape[1], x2.shape[1], dy2.dtype)
    sk = _WG_CHOICE.get(key)
    if sk is None:
        if torch.cuda.is_current_stream_capturing():
            return dy2.t() @ x2
        cands = {1: lambda: dy2.t() @ x2}
        for s in (2, 4, 8, 16):
            if T % s == 0 and T // s >= 256:
                cands[s] = (lambda s=s: _wgrad_splitk(dy2, x2, s))
        from .conv import _time
        times = {s: _time(fn) for s, fn in cands.items()}
        sk = _WG_CHOICE[key] = min(times, key=times.get)
    return dy2.t() @ x2 if sk == 1 else _wgrad_splitk(dy2, x2, sk)


def gemm_nt_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    """Shapes our GEMM kernel serves: bf16, out features % 128, in features % 64."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.dim() == 2
            and w.shape[0] % 128 == 0 and w.shape[1] % 64 == 0 and x.shape[-1] == w.shape[1] and x.numel() > 0)


_LIN_CHOICE: Dict[str, str] = {}
_LIN_TABLE = [False]
TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tuning",
                     "linear_gfx950.json")


def _lin_table() -> None:
    if _LIN_TABLE[0]:
        return
    _LIN_TABLE[0] = True
    try:
        with open(TABLE) as f:
            d = json.load(f)
        if d.get("arch") in (None, _arch()):
            _LIN_CHOICE.update({k: v for k, v in d.get("choices", {}).items() if v in ("ours", "lib")})
    except (OSError, ValueError):
        pass
    out = os.environ.get("PDT_LINEAR_DUMP")
    if out:
        atexit.register(lambda: json.dump({"arch": _arch(), "choices": dict(sorted(_LIN_CHOICE.items()))},
                                          open(out, "w"), indent=1))


def _arch() -> str:
    try:
        return torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    except Exception:  # pragma: no cover - no GPU
        return "cpu"


def _ours(x: torch.Tensor, w: torch.Tensor, kind: str = "bias", b: Optional[torch.Tensor] = None,
          tanh_form: bool = False) -> bool:
    """Run this forward GEMM (``kind``: "bias" | "nobias" | "gelu") on our kernel? See the module docstring."""
    mode = SW.linear_epilogue
    if mode == "0" or not gemm_nt_ok(x, w):
        return False
    if mode == "1":
        return True
    M, K, N = x.numel() // x.shape[-1], x.shape[-1], w.shape[0]
    key = f"{kind},{M},{N},{K}"
    c = _LIN_CHOICE.get(key)
    if c is None:
        _lin_table()
        c = _LIN_CHOICE.get(key)
    if c is None and mode != "time":
        # a shape the table does not list runs the library: isolated forward timings picked ours for GPT-2-medium's
        # qkv / fc1 / fused GELU and the whole step lost 3 % (tuning/linear_gfx950.json _note); "time" re-enables it
        c = _LIN_CHOICE[key] = "lib"
    if c is None:
        if torch.cuda.is_current_stream_capturing():
            return False
        from .conv import _time
        x2, wc = x.reshape(-1, K).contiguous(), w.contiguous()
        if kind == "gelu":
            bf = b.float() if b is not None else None
            ours = lambda: native().gemm_nt(x2, wc, bf, 2, tanh_form)  # noqa: E731
            from .gelu import bias_gelu
            lib = lambda: bias_gelu(F.linear(x2, wc), bf, "tanh" if tanh_form else "none")  # noqa: E731
        else:
            bb = b if kind == "bias" else None
            ours = lambda: native().gemm_nt(x2, wc, bb, 1 if bb is not None else 0, False)  # noqa: E731
            lib = lambda: F.linear(x2, wc, bb)  # noqa: E731
        with torch.no_grad():
            c = "ours" if _time(ours) < _time(lib) else "lib"
        _LIN_CHOICE[key] = c
    return c == "ours"


def linear_choices() -> Dict[str, str]:
    """Decisions taken so far: {"kind,M,N,K": "ours" | "lib"}."""
    return dict(_LIN_CHOICE)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        if _ours(x, w, "bias" if b is not None else "nobias", b):
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            y = native().gemm_nt(x2, w.contiguous(), b, 1 if b is not None else 0, False)[0]
            # (not .view: autograd refuses an in-place op, ops/rope.py, on a view made inside a Function;
            # y is this call's own tensor, which is what _unsafe_view is for, as F.linear itself does)
            return torch.ops.aten._unsafe_view(y, [*x.shape[:-1], w.shape[0]])
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        d = dy.shape[-1]
        dy2 = dy.reshape(-1, d)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ w).reshape(*dy.shape[:-1], w.shape[1])
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dy2, x.reshape(-1, x.shape[-1]))
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = native().colsum(dy2, w.dtype)
        return dx, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        # autocast does not reach into an autograd.Function: cast the operands the way autocast casts
        # F.linear's, then run (and later backpropagate) the Function with autocast off, so its saved
        # tensors and the incoming gradient share one dtype (amp_bf16: our bf16 path; amp_fp16: aten)
        dt = torch.get_autocast_dtype("cuda")
        with torch.autocast("cuda", enabled=False):
            return linear(x.to(dt), weight.to(dt), bias.to(dt) if bias is not None else None)
    if (use_native(x) and x.dtype in (torch.float32, torch.bfloat16) and weight.dtype == x.dtype
            and (bias is None or bias.dtype == x.dtype) and weight.shape[0] % 8 == 0):
        return _LinearFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)


class Linear(torch.nn.Linear):
    """``nn.Linear`` (same parameters and state-dict keys) on :func:`linear`: dbias on the ``colsum``
    kernel. Besides speed this keeps the step hipGraph-safe: aten's ``sum(0)`` over a [1024, 1000]
    gradient takes its multi-block path, whose staging workspace does not survive a captured
    backward — a replay after any later allocation returns a wrong bias gradient (the ResNet head at
    1024/GPU trained to NaN; tools/diag_graph_colsum_bwd.py, profiles/r6/graph_colsum_bwd.txt)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return linear(x, self.weight, self.bias)


class _LinearGeluFn(torch.autograd.Function):
    """g = gelu(x·Wᵀ + b) with the GEMM, bias and GELU in one kernel (EPI_GELU); h = x·Wᵀ is kept for
    the backward, which is the column-strip GELU-backward + bias-gradient kernel and two GEMMs."""

    @staticmethod
    def forward(ctx, x, w, b, tanh_form):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        bf = b.float() if b is not None else None
        h, g = native().gemm_nt(x2, w.contiguous(), bf, 2, tanh_form)
        ctx.save_for_backward(x2, w, h, bf)
        ctx.tanh_form, ctx.xshape, ctx.has_b, ctx.bdtype = tanh_form, x.shape, b is not None, (
            b.dtype if b is not None else None)
        return g.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dg):
        x2, w, h, bf = ctx.saved_tensors
        dh, db = native().bias_gelu_bwd(dg.reshape(h.shape).contiguous(), h, bf, ctx.tanh_form)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = (dh @ w).view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dh, x2)
        dbias = db.to(ctx.bdtype) if ctx.has_b and ctx.needs_input_grad[2] else None
        return dx, dw, dbias, None


def linear_gelu(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], approximate: str) -> Optional[torch.Tensor]:
    """gelu(linear(x, weight, bias)) on the fused-epilogue kernel, or None when it does not apply
    (switch off, unsupported shape/dtype): the caller then runs linear + bias_gelu."""
    if (bias is not None and bias.dtype not in (torch.bfloat16, torch.float32)) or not use_native(x) \
            or not _ours(x, weight, "gelu", bias, approximate == "tanh"):
        return None
    return _LinearGeluFn.apply(x, weight, bias, approximate == "tanh")


# ---------------------------------------------------------------------------- decode-time Linears (M <= 64)
# launches of the bf16 skinny GEMM, the last (S, FT, NT) any of the kernels ran with, launches of the e4m3-weight
# one and of the int4-weight one, launches of the any-row int4 GEMM (gemm_w4.hip)
SKINNY_STATS = {"native_calls": 0, "geo": None, "w8_calls": 0, "w4_calls": 0, "w4_tall_calls": 0}
SKINNY_MAX_ROWS = 64


def skinny_ok(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False) -> bool:
    """Inside gemm_skinny.hip's contract: GPU bf16, 1..64 rows, out features % 16 (% 32 with ``swiglu``: F % 16),
    in features % 64, a contiguous 16-byte aligned weight below 2^31 bytes."""
    if not (x.is_cuda and w.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.dim() == 2
            and x.dim() >= 1 and x.shape[-1] == w.shape[1]):
        return False
    N, K = w.shape
    rows = x.numel() // K if K else 0
    return (1 <= rows <= SKINNY_MAX_ROWS and N % (32 if swiglu else 16) == 0 and N > 0 and K % 64 == 0 and K > 0
            and w.is_contiguous() and w.data_ptr() % 16 == 0 and N * K * 2 < 2 ** 31)


def linear_skinny(x: torch.Tensor, w: torch.Tensor, swiglu: bool = False, splits: Optional[int] = None) -> torch.Tensor:
    """``x @ w.T`` (``swiglu``: SwiGLU of it, ``w`` the packed [gate; up] rows) for inference on at most 64 rows, on
    the weight-streaming kernel. GPU bf16 inside the contract with no gradient to record; anything else (CPU,
    fp32, ``PDT_DISABLE_NATIVE=1``, a shape outside the contract, autograd) is ``F.linear`` (then
    ``ops.swiglu.swiglu``). ``splits``: grid split-K override (None: the kernel's rule)."""
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
    if use_native(x) and not needs_grad and skinny_ok(x, w, swiglu):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if x2.data_ptr() % 16 == 0:
            mode, sp = (1 if swiglu else 0), int(splits or 0)
            y = native().gemm_skinny(x2, w, mode, sp)
            SKINNY_STATS["native_calls"] += 1
            SKINNY_STATS["geo"] = tuple(int(v) for v in native().gemm_skinny_geo(x2.shape[0], w.shape[0], w.shape[1],
                                                                                 mode, sp))
            return y.view(*x.shape[:-1], y.shape[-1])
    y = F.linear(x, w)
    if swiglu:
        from .swiglu import swiglu as _swiglu
        y = _swiglu(y)
    return y


# ---------------------------------------------------------------------------- the same on e4m3 weights (W8A16)
E4M3_MAX = 448.0


def quantize_rows_e4m3(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w`` [N, K] bf16 -> (``wq`` [N, K] float8_e4m3fn, ``scale`` [N] fp32), one scale per output feature, in
    fp32: amax = max_k |w|, scale = amax * (1 / 448) (1 for a zero row), wq = e4m3(clamp(w * (448 / amax), +-448)),
    round to nearest even. The kernel on the GPU, the same formula in torch elsewhere (CPU,
    ``PDT_DISABLE_NATIVE=1``, K % 8 != 0): equal bytes and scales. A NaN or Inf in ``w`` is refused."""
    if w.dim() != 2 or w.dtype != torch.bfloat16:
        raise ValueError(f"quantize_rows_e4m3: a bf16 [N, K] weight, got {w.dtype} {tuple(w.shape)}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_rows_e4m3: the weight holds NaN or Inf")
    if use_native(w) and w.shape[1] % 8 == 0 and w.numel() > 0:
        wc = w.contiguous()
        if wc.data_ptr() % 16 == 0:
            wq, scale = native().quantize_rows_e4m3(wc)
            return wq, scale
    return quantize_rows_e4m3_reference(w)


def quantize_rows_e4m3_reference(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``quantize_rows_e4m3``'s formula in torch on ``w`` [N, K] (any float dtype, taken to fp32), without its checks
    and without a host read: what the reference paths of the e4m3 KV cache apply to the rows they store."""
    wf = w.float()
    amax = wf.abs().amax(1)
    zero = amax == 0
    scale = torch.where(zero, torch.ones_like(amax), amax * torch.tensor(1.0 / E4M3_MAX, dtype=torch.float32))
    # (a division of tensors: ``448 / amax`` would be ``amax.reciprocal() * 448``, two roundings and other bytes)
    inv = torch.where(zero, torch.zeros_like(amax), torch.full_like(amax, E4M3_MAX) / amax)
    return (wf * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn), scale


def skinny_w8_ok(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, swiglu: bool = False) -> bool:
    """Inside gemm_skinny_w8.hip's contract: GPU, bf16 rows (1..64), e4m3 weights with an fp32 scale per output
    feature, out features % 16 (% 32 with ``swiglu``), in features % 128 and below 2^24, contiguous 16-byte
    aligned weights and scales, the weight below 2^31 bytes."""
    if not (x.is_cuda and wq.is_cuda and scale.is_cuda and x.dtype == torch.bfloat16
            and wq.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and wq.dim() == 2 and x.dim() >= 1
            and x.shape[-1] == wq.shape[1] and scale.shape == (wq.shape[0],)):
        return False
    N, K = wq.shape
    rows = x.numel() // K if K else 0
    return (1 <= rows <= SKINNY_MAX_ROWS and N % (32 if swiglu else 16) == 0 and N > 0 and K % 128 == 0
            and 0 < K < 2 ** 24 and wq.is_contiguous() and wq.data_ptr() % 16 == 0 and scale.is_contiguous()
            and scale.data_ptr() % 16 == 0 and N * K < 2 ** 31)


def linear_skinny_w8(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                     splits: Optional[int] = None) -> torch.Tensor:
    """``x @ (wq.float() * scale[:, None]).T`` (``swiglu``: SwiGLU of it, ``wq`` the packed [gate; up] rows) for
    inference on at most 64 rows, on the W8A16 weight-streaming kernel: the scale multiplies the fp32 sum once.
    GPU bf16 rows inside the contract with no gradient to record; anything else (CPU, fp32,
    ``PDT_DISABLE_NATIVE=1``, a shape outside the contract, autograd on ``x``) is ``F.linear`` on the dequantised
    weight (then ``ops.swiglu.swiglu``). ``splits``: grid split-K override (None: the kernel's rule)."""
    needs_grad = torch.is_grad_enabled() and x.requires_grad
    if use_native(x) and not needs_grad and skinny_w8_ok(x, wq, scale, swiglu):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if x2.data_ptr() % 16 == 0:
            mode, sp = (1 if swiglu else 0), int(splits or 0)
            y = native().gemm_skinny_w8(x2, wq, scale, mode, sp)
            SKINNY_STATS["w8_calls"] += 1
            SKINNY_STATS["geo"] = tuple(int(v) for v in native().gemm_skinny_w8_geo(x2.shape[0], wq.shape[0],
                                                                                    wq.shape[1], mode, sp))
            return y.view(*x.shape[:-1], y.shape[-1])
    y = F.linear(x, (wq.float() * scale[:, None]).to(x.dtype))
    if swiglu:
        from .swiglu import swiglu as _swiglu
        y = _swiglu(y)
    return y


# ---------------------------------------------------------------------------- the same on group-wise int4 (W4A16)
INT4_GROUP = 128   # k per scale
INT4_LINE = 256    # k per 128-byte line of a packed row: the kernel's K step
INT4_MAX = 7.0
# Byte b of a packed word holds value j = _NIB_LO[b] in its low nibble and j = _NIB_HI[b] in its high one: the word
# has j = 2 t in nibble t and j = 2 t + 1 in nibble t + 4.
_NIB_LO, _NIB_HI = (0, 4, 1, 5), (2, 6, 3, 7)


def pack_int4(q: torch.Tensor) -> torch.Tensor:
    """``q`` int8 [N, K] with values in [-8, 7], K % 256 == 0 -> uint8 [N, K / 2], the layout gemm_skinny_w4.hip
    reads (this function and ``unpack_int4`` are its definition). A row's 128-byte line ``s`` holds k in
    [256 s, 256 s + 256); its bytes [32 g, 32 g + 32), g = 0..3, are eight little-endian 32-bit words, and word i
    holds the eight values k = 256 s + 32 i + 8 g + j as two's-complement nibbles, j = 2 t in nibble t and
    j = 2 t + 1 in nibble t + 4."""
    if q.dim() != 2 or q.dtype != torch.int8 or q.shape[1] % INT4_LINE != 0:
        raise ValueError(f"pack_int4: an int8 [N, K] with K % {INT4_LINE} == 0, got {q.dtype} {tuple(q.shape)}")
    N, K = q.shape
    u = (q & 15).to(torch.uint8).view(N, K // INT4_LINE, 8, 4, 8)          # [n, s, i, g, j]
    b = u[..., list(_NIB_LO)] | (u[..., list(_NIB_HI)] << 4)               # [n, s, i, g, byte of the word]
    return b.permute(0, 1, 3, 2, 4).reshape(N, K // 2)                     # [n, s, g, i, byte]


def unpack_int4(wq: torch.Tensor) -> torch.Tensor:
    """``pack_int4``'s inverse: uint8 [N, K / 2] -> int8 [N, K] in [-8, 7]."""
    if wq.dim() != 2 or wq.dtype != torch.uint8 or wq.shape[1] % (INT4_LINE // 2) != 0:
        raise ValueError(f"unpack_int4: a uint8 [N, K / 2] with K % {INT4_LINE} == 0, got {wq.dtype} {tuple(wq.shape)}")
    N, K = wq.shape[0], 2 * wq.shape[1]
    b = wq.reshape(N, K // INT4_LINE, 4, 8, 4).permute(0, 1, 3, 2, 4)        # [n, s, i, g, byte]
    u = torch.empty(N, K // INT4_LINE, 8, 4, 8, dtype=torch.uint8, device=wq.device)
    u[..., list(_NIB_LO)] = b & 15
    u[..., list(_NIB_HI)] = b >> 4
    q = u.to(torch.int8)
    return torch.where(q > 7, q - 16, q).reshape(N, K)


def quantize_groups_int4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w`` [N, K] bf16, K % 256 == 0 -> (``wq`` [N, K / 2] uint8 in ``pack_int4``'s layout, ``scale`` [K / 128, N]
    fp32, group-major), symmetric int4 with one scale per 128 consecutive k of a row, in fp32: amax over the group,
    scale = amax * (1 / 7) (1 for a zero group), q = clamp(rint(w * (7 / amax)), -7, 7), ties to even. The kernel on
    the GPU, the same formula in torch elsewhere (CPU, ``PDT_DISABLE_NATIVE=1``): equal bytes and scales. A NaN or
    Inf in ``w`` is refused."""
    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.shape[1] % INT4_LINE != 0 or w.numel() == 0:
        raise ValueError(f"quantize_groups_int4: a bf16 [N, K] weight with K % {INT4_LINE} == 0, got {w.dtype} "
                         f"{tuple(w.shape)}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_groups_int4: the weight holds NaN or Inf")
    if use_native(w):
        wc = w.contiguous()
        if wc.data_ptr() % 16 == 0:
            wq, scale = native().quantize_groups_int4(wc)
            return wq, scale
    N, K = w.shape
    wf = w.float().view(N, K // INT4_GROUP, INT4_GROUP)
    amax = wf.abs().amax(2)
    zero = amax == 0
    scale = torch.where(zero, torch.ones_like(amax), amax * torch.tensor(1.0 / INT4_MAX, dtype=torch.float32))
    # (a division of tensors, as in quantize_rows_e4m3_reference: ``7 / amax`` would round twice)
    inv = torch.where(zero, torch.zeros_like(amax), torch.full_like(amax, INT4_MAX) / amax)
    q = (wf * inv[:, :, None]).round().clamp(-INT4_MAX, INT4_MAX).to(torch.int8).view(N, K)
    return pack_int4(q), scale.t().contiguous()


def dequantize_groups_int4(wq: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K]: ``unpack_int4(wq)[n, k] * scale[k // 128, n]``, one exact-or-rounded fp32 product per element."""
    q = unpack_int4(wq).float()
    return q * scale.t().repeat_interleave(INT4_GROUP, 1)


def skinny_w4_ok(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, swiglu: bool = False) -> bool:
    """Inside gemm_skinny_w4.hip's contract: GPU, bf16 rows (1..64), packed int4 weights [N, K / 2] uint8 with fp32
    scales [K / 128, N], out features % 16 (% 32 with ``swiglu``), in features % 256 and below 2^24, contiguous
    16-byte aligned weights and scales, the weight below 2^31 bytes."""
    if not (x.is_cuda and wq.is_cuda and scale.is_cuda and x.dtype == torch.bfloat16 and wq.dtype == torch.uint8
            and scale.dtype == torch.float32 and wq.dim() == 2 and x.dim() >= 1 and x.shape[-1] == 2 * wq.shape[1]):
        return False
    N, K = wq.shape[0], 2 * wq.shape[1]
    rows = x.numel() // K if K else 0
    return (1 <= rows <= SKINNY_MAX_ROWS and N % (32 if swiglu else 16) == 0 and N > 0 and K % INT4_LINE == 0
            and 0 < K < 2 ** 24 and scale.shape == (K // INT4_GROUP, N) and wq.is_contiguous()
            and wq.data_ptr() % 16 == 0 and scale.is_contiguous() and scale.data_ptr() % 16 == 0
            and N * (K // 2) < 2 ** 31)


def linear_skinny_w4(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
                     splits: Optional[int] = None) -> torch.Tensor:
    """``x @ dequantize_groups_int4(wq, scale).T`` (``swiglu``: SwiGLU of it, ``wq`` the packed [gate; up] rows) for
    inference on at most 64 rows, on the W4A16 weight-streaming kernel: exact int4 operands in the matrix cores, one
    fp32 fma by the group's scale per 128 k. GPU bf16 rows inside the contract with no gradient to record; anything
    else (CPU, fp32, ``PDT_DISABLE_NATIVE=1``, a shape outside the contract, autograd on ``x``) is ``F.linear`` on
    the dequantised weight (then ``ops.swiglu.swiglu``). ``splits``: grid split-K override (None: the kernel's rule)."""
    needs_grad = torch.is_grad_enabled() and x.requires_grad
    if use_native(x) and not needs_grad and skinny_w4_ok(x, wq, scale, swiglu):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if x2.data_ptr() % 16 == 0:
            mode, sp = (1 if swiglu else 0), int(splits or 0)
            y = native().gemm_skinny_w4(x2, wq, scale, mode, sp)
            SKINNY_STATS["w4_calls"] += 1
            SKINNY_STATS["geo"] = tuple(int(v) for v in native().gemm_skinny_w4_geo(x2.shape[0], wq.shape[0],
                                                                                    2 * wq.shape[1], mode, sp))
            return y.view(*x.shape[:-1], y.shape[-1])
    y = F.linear(x, dequantize_groups_int4(wq, scale).to(x.dtype))
    if swiglu:
        from .swiglu import swiglu as _swiglu
        y = _swiglu(y)
    return y


# ---------------------------------------------------------------------------- W4A16 at any row count
def w4_ok(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor) -> bool:
    """Inside gemm_w4.hip's contract: ``skinny_w4_ok``'s operands (GPU, bf16 rows, packed int4 weights [N, K / 2]
    uint8 with fp32 scales [K / 128, N], out features % 16, in features % 256 and below 2^24, contiguous 16-byte
    aligned weights and scales, the weight below 2^31 bytes) at any row count >= 1."""
    if not (x.is_cuda and wq.is_cuda and scale.is_cuda and x.dtype == torch.bfloat16 and wq.dtype == torch.uint8
            and scale.dtype == torch.float32 and wq.dim() == 2 and x.dim() >= 1 and x.shape[-1] == 2 * wq.shape[1]):
        return False
    N, K = wq.shape[0], 2 * wq.shape[1]
    rows = x.numel() // K if K else 0
    return (1 <= rows <= 64 * 65535 and N % 16 == 0 and N > 0 and K % INT4_LINE == 0 and 0 < K < 2 ** 24
            and scale.shape == (K // INT4_GROUP, N) and wq.is_contiguous() and wq.data_ptr() % 16 == 0
            and scale.is_contiguous() and scale.data_ptr() % 16 == 0 and N * (K // 2) < 2 ** 31)


def linear_w4(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, swiglu: bool = False,
              splits: Optional[int] = None) -> torch.Tensor:
    """``linear_skinny_w4`` without its row limit. At most 64 rows: exactly ``linear_skinny_w4``. More rows on the
    GPU inside ``w4_ok`` with no gradient to record: the tiled W4A16 GEMM (csrc/kernels/gemm_w4.hip: the same
    arithmetic, weights dequantised once per workgroup and held in registers, rows through LDS), then
    ``ops.swiglu.swiglu`` for ``swiglu``. Anything else (CPU, fp32, ``PDT_DISABLE_NATIVE=1``, autograd on ``x``) is
    ``F.linear`` on the dequantised weight. ``splits``: grid split-K override (None: the kernel's rule)."""
    K = x.shape[-1]
    if K == 0 or x.numel() // K <= SKINNY_MAX_ROWS:
        return linear_skinny_w4(x, wq, scale, swiglu, splits)
    needs_grad = torch.is_grad_enabled() and x.requires_grad
    y = None
    if use_native(x) and not needs_grad and w4_ok(x, wq, scale):
        x2 = x.reshape(-1, K).contiguous()
        if x2.data_ptr() % 16 == 0:
            sp = int(splits or 0)
            y = native().gemm_w4(x2, wq, scale, sp)
            SKINNY_STATS["w4_tall_calls"] += 1
            SKINNY_STATS["geo"] = tuple(int(v) for v in native().gemm_w4_geo(x2.shape[0], wq.shape[0], K, sp))
            y = y.view(*x.shape[:-1], y.shape[-1])
    if y is None:
        y = F.linear(x, dequantize_groups_int4(wq, scale).to(x.dtype))
    if swiglu:
        from .swiglu import swiglu as _swiglu
        y = _swiglu(y)
    return y
