"""Llama-style decoder: RMSNorm, rotary position embedding, SwiGLU MLP, no biases, untied LM head.

The three pieces that differ from GPT-2 each run on a HIP kernel of their own (ops/rmsnorm.py,
ops/rope.py, ops/swiglu.py); everything else is the GPT-2 hot path: flash attention reading Q/K/V in
place from the packed QKV GEMM output at head dim 64, the bias-free GEMMs of ops/linear.py and the
fused cross-entropy. As in ``run_blocks`` every residual add is inside the RMSNorm that follows it,
one kernel per residual step each way.

Multi-head or grouped-query attention (``n_kv_head`` K/V heads, each shared by ``n_head / n_kv_head``
consecutive query heads, HF's ``repeat_kv`` order; the flash kernels read the shared heads in place),
head dim 64, no dropout sites, sequence length at most ``block_size`` (the RoPE table).

fp8 (``--precision fp8``, ops/fp8.py ``enable_fp8``): the four Linears of every block run their three GEMMs on
e4m3 operands, and the operations in front of them write e4m3 where the value is computed: the add+RMSNorm
in front of ``c_attn`` / ``c_fc`` (``add_rms_norm_fp8``) and SwiGLU in front of ``mlp.c_proj``
(``fp8_swiglu_mlp``, which also emits the packed gate/up gradient in e4m3 for ``c_fc``'s backward GEMMs). The
first ``ln_1`` stays the plain kernel plus ``c_attn``'s own cast, the LM head stays bf16. An untagged model,
``eval()``, fp32, the CPU and ``PDT_DISABLE_NATIVE=1`` take the bf16 path above unchanged.
Parameter names follow the nanoGPT-style layout of models/gpt2.py: ``transformer.wte``,
``transformer.h.{i}.ln_1``, ``.attn.c_attn`` (packed q, k, v rows: ``(n_head + 2·n_kv_head)·64`` of them),
``.attn.c_proj``, ``.ln_2``, ``.mlp.c_fc`` (packed [gate; up] rows), ``.mlp.c_proj``, ``transformer.ln_f``,
``lm_head``; ``from_hf_state_dict`` maps a Hugging Face Llama state dict onto it.

Weight-only 8-bit decoding: ``Llama.quantize_decode_weights()`` quantises every block Linear and the LM head
row-wise to e4m3 (ops/linear.py ``quantize_rows_e4m3``); calls on at most 64 rows in ``eval()`` under
``no_grad`` then run the W8A16 skinny GEMM (``linear_skinny_w8``), whatever ``PDT_DECODE_GEMM`` says. More rows
(a long prefill) and training keep the bf16 weights, which stay in place; ``drop_decode_weights()`` undoes it.
``quantize_decode_weights("int4")`` stores symmetric int4 with one fp32 scale per 128 inputs instead
(``quantize_groups_int4``, a quarter of the bf16 bytes plus the scales) and the same calls run the W4A16 skinny
GEMM (``linear_skinny_w4``); one call replaces the other's copies. ``quantize_decode_weights("int4",
all_rows=True)`` sends calls on more than 64 rows (a long prefill, an extend, a verify) to the int4 copies too, on
the tiled W4A16 GEMM (``linear_w4``): the whole of generation then computes from one set of weights.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F
from torch import nn

from ..config import SW
from ..ops.attention import (attention_decode, attention_decode_paged, attention_decode_paged_fp8, attention_extend,
                             attention_extend_paged, attention_qkv)
from ..ops.cross_entropy import cross_entropy
from ..ops.fp8 import Fp8Act, add_rms_norm_fp8, fp8_input_slot, fp8_linear, fp8_ok, fp8_swiglu_mlp, rms_fp8_ok
from ..ops.kv_cache import PAGE, KVCache, PagedKVCache
from ..ops.linear import (SKINNY_MAX_ROWS, linear, linear_skinny, linear_skinny_w8, linear_w4,
                          quantize_groups_int4, quantize_rows_e4m3)
from ..ops.rmsnorm import RMSNorm, add_rms_norm
from ..ops.rope import RotaryTable, rope_append_, rope_append_paged_, rope_append_paged_fp8_, rope_qkv_
from ..ops.sampling import SamplerState
from ..ops.sampling import sample as sample_fused
from ..ops.swiglu import swiglu
from .transformer import init_weights

HEAD_DIM = 64


@dataclass
class LlamaConfig:
    n_layer: int = 24
    n_head: int = 16
    n_embd: int = 1024
    ffn: int = 2816
    block_size: int = 1024
    vocab_size: int = 32000
    rope_base: float = 10000.0
    eps: float = 1e-5
    n_kv_head: int | None = None  # K/V heads (grouped-query attention); None: n_head, multi-head attention

    @property
    def kv_heads(self) -> int:
        return self.n_head if self.n_kv_head is None else self.n_kv_head


def _fp8_tag(mod: nn.Linear):
    """``mod``'s (state, slot) when ``enable_fp8`` tagged it and it is training; else None (the bf16 path)."""
    return getattr(mod, "_fp8", None) if mod.training else None


def _skinny(x, training: bool) -> bool:
    """Decode-time rows: ``PDT_DECODE_GEMM=1``, ``eval()``, no autograd and at most 64 rows of ``x``. Then the
    Linears go through ``linear_skinny`` (the weight-streaming kernel where its contract holds)."""
    return (SW.decode_gemm and not training and not torch.is_grad_enabled() and isinstance(x, torch.Tensor)
            and 0 < x.numel() // x.shape[-1] <= SKINNY_MAX_ROWS)


def _w8(x, mod: nn.Linear, attr: str = "_w8"):
    """``mod``'s (wq, scale) when ``quantize_decode_weights`` left them there (``attr``: ``_w8`` e4m3, ``_w4`` int4)
    and this call is decode-time (``eval()``, no autograd, at most 64 rows, or any row count when the int4 copy
    was made with ``all_rows=True``); else None. Weights updated in place since then are refused."""
    q = getattr(mod, attr, None)
    if q is None or mod.training or torch.is_grad_enabled() or not isinstance(x, torch.Tensor):
        return None
    rows = x.numel() // x.shape[-1]
    if rows < 1 or (rows > SKINNY_MAX_ROWS and not (len(q) > 3 and q[3])):  # q[3]: ``all_rows`` (int4 only)
        return None
    if q[2] != mod.weight._version:
        raise RuntimeError("a Linear's weight changed in place after quantize_decode_weights(): its e4m3 copy is "
                           "stale; call quantize_decode_weights() again (or drop_decode_weights())"
                           if attr == "_w8" else
                           "a Linear's weight changed in place after quantize_decode_weights(\"int4\"): its int4 copy "
                           "is stale; call quantize_decode_weights(\"int4\") again (or drop_decode_weights())")
    return q[0], q[1]


def _w4(x, mod: nn.Linear):
    return _w8(x, mod, "_w4")


def _linear(x, mod: nn.Linear) -> torch.Tensor:
    """``mod``'s bias-free GEMM: fp8 when ``enable_fp8`` tagged it and the shape is served (ops/fp8.py; ``x``
    may then be an ``Fp8Act``, already e4m3 from ``add_rms_norm_fp8``), else bf16 (ops/linear.py); decode-time
    rows on the W8A16 (W4A16) skinny GEMM after ``quantize_decode_weights()`` (``("int4")``), else under
    ``PDT_DECODE_GEMM=1`` on the bf16 skinny GEMM."""
    t = _fp8_tag(mod)
    if t is not None and (isinstance(x, Fp8Act) or fp8_ok(x, mod.weight)):
        return fp8_linear(x, mod.weight, None, t[0], t[1])
    q = _w8(x, mod)
    if q is not None:
        return linear_skinny_w8(x, q[0], q[1])
    q = _w4(x, mod)
    if q is not None:
        return linear_w4(x, q[0], q[1])
    if _skinny(x, mod.training):
        return linear_skinny(x, mod.weight)
    return linear(x, mod.weight)


class LlamaAttention(nn.Module):
    def __init__(self, dim: int, heads: int, kv_heads: int | None = None):
        super().__init__()
        assert dim == heads * HEAD_DIM, f"head dim must be {HEAD_DIM}: n_embd {dim}, n_head {heads}"
        kv_heads = heads if kv_heads is None else kv_heads
        if kv_heads <= 0 or heads % kv_heads != 0:
            raise ValueError(f"n_kv_head = {kv_heads} must be positive and divide n_head = {heads}")
        self.heads, self.kv_heads = heads, kv_heads
        self.c_attn = nn.Linear(dim, (heads + 2 * kv_heads) * HEAD_DIM, bias=False)  # q, then k, then v rows
        self.c_proj = nn.Linear(dim, dim, bias=False)

    def forward(self, x: torch.Tensor, rope: RotaryTable, cache: KVCache | None = None, layer: int = 0) -> torch.Tensor:
        if cache is not None:
            return self._forward_cached(x, rope, cache, layer)
        qkv = _linear(x, self.c_attn)  # [B, T, (H + 2 Hkv) 64]; its backward needs x and W only, so
        qkv = rope_qkv_(qkv, rope.cos, rope.sin, self.heads, self.kv_heads)  # Q and K are rotated in place
        y = attention_qkv(qkv, self.heads, causal=True, kv_heads=self.kv_heads)
        return _linear(y, self.c_proj)

    def _forward_cached(self, x, rope, cache: KVCache, layer: int):
        """Inference on a KV cache: the Tn new rows are rotated at positions lens[b] + t and appended (one
        kernel); a prefill (Tn > 1, empty cache) then runs the causal flash forward on them, a decode step
        (Tn == 1) the split-KV kernel on the cache, and ``Llama.extend`` (which sets ``cache.extending`` around
        its forward) with Tn > 1 the multi-token append kernel, whatever the cache holds. ``cache.lens`` is
        advanced by the caller after the last layer."""
        if isinstance(cache, PagedKVCache):
            return self._forward_paged(x, rope, cache, layer)
        Tn = x.shape[1]
        if Tn > 1 and cache.bound > 0 and not cache.extending:
            raise ValueError(f"{Tn} new tokens onto a cache that may hold {cache.bound} positions: chunked prefill "
                             "is not what prefill does (prefill an empty cache, then extend() or decode_step())")
        cache.require(Tn, rope.cos.shape[0])
        qkv = _linear(x, self.c_attn)
        qkv = rope_append_(qkv, rope.cos, rope.sin, self.heads, self.kv_heads, cache.k[layer], cache.v[layer],
                           cache.lens)
        if Tn > 1 and cache.extending:
            y = attention_extend(qkv, cache.k[layer], cache.v[layer], cache.lens, self.heads, self.kv_heads,
                                 cache=cache)
        elif Tn > 1:
            y = attention_qkv(qkv, self.heads, causal=True, kv_heads=self.kv_heads)
        else:
            y = attention_decode(qkv, cache.k[layer], cache.v[layer], cache.lens, self.heads, self.kv_heads,
                                 cache=cache)
        return _linear(y, self.c_proj)

    def _forward_paged(self, x, rope, cache: PagedKVCache, layer: int):
        """``_forward_cached`` on a paged cache, on the slots ``cache.select`` named: the paged append, then the
        causal flash forward on the new rows (Tn > 1: a prefill of empty slots), the paged split-KV kernel
        (Tn == 1) or, under ``Llama.extend`` with Tn > 1, the paged multi-token append kernel, whatever the slots
        hold."""
        Tn = x.shape[1]
        table, lens, slots = cache.view()
        if Tn > 1 and not cache.extending and any(
                cache.bounds[s] > 0 for s in (range(cache.slots) if slots is None else slots)):
            raise ValueError(f"{Tn} new tokens onto paged slots that may hold up to {cache.bound} positions: chunked "
                             "prefill is not what prefill does (prefill empty slots, then extend() or decode_step())")
        if cache.fp8:
            return self._forward_paged_fp8(x, rope, cache, layer, table, lens, slots)
        cache.require(Tn, rope.cos.shape[0], slots)
        qkv = _linear(x, self.c_attn)
        qkv = rope_append_paged_(qkv, rope.cos, rope.sin, self.heads, self.kv_heads, cache.k[layer], cache.v[layer],
                                 table, lens)
        if Tn > 1 and cache.extending:
            y = attention_extend_paged(qkv, cache.k[layer], cache.v[layer], table, lens, self.heads, self.kv_heads,
                                       cache=cache)
        elif Tn > 1:
            y = attention_qkv(qkv, self.heads, causal=True, kv_heads=self.kv_heads)
        else:
            y = attention_decode_paged(qkv, cache.k[layer], cache.v[layer], table, lens, self.heads, self.kv_heads,
                                       cache=cache)
        return _linear(y, self.c_proj)

    def _forward_paged_fp8(self, x, rope, cache: PagedKVCache, layer: int, table, lens, slots):
        """``_forward_paged`` on an e4m3 cache: the quantising append, then the causal flash forward on the bf16
        ``qkv`` (Tn > 1: a prefill of empty slots, which never reads the cache) or the e4m3 decode kernel
        (Tn == 1). The multi-token append on such a cache is refused before any launch."""
        Tn = x.shape[1]
        if Tn > 1 and cache.extending:
            raise NotImplementedError(f"extend of {Tn} tokens on an fp8 paged cache is out of scope: the e4m3 form of "
                                      "the multi-token append kernel is not built (prefill empty slots whole, then "
                                      "decode_step, or use a bf16 paged cache)")
        cache.require(Tn, rope.cos.shape[0], slots)
        qkv = _linear(x, self.c_attn)
        qkv = rope_append_paged_fp8_(qkv, rope.cos, rope.sin, self.heads, self.kv_heads, cache.k[layer], cache.v[layer],
                                     cache.k_scale[layer], cache.v_scale[layer], table, lens)
        if Tn > 1:
            y = attention_qkv(qkv, self.heads, causal=True, kv_heads=self.kv_heads)
        else:
            y = attention_decode_paged_fp8(qkv, cache.k[layer], cache.v[layer], cache.k_scale[layer],
                                           cache.v_scale[layer], table, lens, self.heads, self.kv_heads, cache=cache)
        return _linear(y, self.c_proj)


class LlamaMLP(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.c_fc = nn.Linear(dim, 2 * hidden, bias=False)  # rows [0, F): gate, [F, 2F): up
        self.c_proj = nn.Linear(hidden, dim, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _fp8_tag(self.c_fc) is not None:
            y = fp8_swiglu_mlp(x, self.c_fc, self.c_proj)  # SwiGLU emits e4m3 for c_proj (PDT_FP8_SWIGLU)
            if y is not None:
                return y
        q = _w8(x, self.c_fc)
        if q is not None:  # as below, on the e4m3 weights
            return _linear(linear_skinny_w8(x, q[0], q[1], swiglu=True), self.c_proj)
        q = _w4(x, self.c_fc)
        if q is not None:  # and on the int4 weights
            return _linear(linear_w4(x, q[0], q[1], swiglu=True), self.c_proj)
        if _skinny(x, self.c_fc.training):  # c_fc with SwiGLU in the GEMM's epilogue: no [rows, 2F] round trip
            return _linear(linear_skinny(x, self.c_fc.weight, swiglu=True), self.c_proj)
        return _linear(swiglu(_linear(x, self.c_fc)), self.c_proj)


class LlamaBlock(nn.Module):
    """Pre-norm block: x + attn(ln_1(x)), then x + mlp(ln_2(x))."""

    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.ln_1 = RMSNorm(cfg.n_embd, eps=cfg.eps)
        self.attn = LlamaAttention(cfg.n_embd, cfg.n_head, cfg.n_kv_head)
        self.ln_2 = RMSNorm(cfg.n_embd, eps=cfg.eps)
        self.mlp = LlamaMLP(cfg.n_embd, cfg.ffn)

    def forward(self, x: torch.Tensor, rope: RotaryTable, cache: KVCache | None = None, layer: int = 0) -> torch.Tensor:
        """Unfused path (PDT_FUSED_ADDLN=0, or a block called on its own)."""
        x = x + self.attn(self.ln_1(x), rope, cache, layer)
        return x + self.mlp(self.ln_2(x))


def run_llama_blocks(blocks, x: torch.Tensor, final_norm: RMSNorm, rope: RotaryTable,
                     cache: KVCache | None = None) -> torch.Tensor:
    """``final_norm(blocks(x))`` with every residual add fused into the RMSNorm that follows it (the
    block's ln_2, the next block's ln_1, finally ``final_norm``), as ``transformer.run_blocks`` does
    with LayerNorm: one add+RMSNorm kernel per residual step forward, one backward kernel that also
    accumulates the residual stream's gradient."""
    blocks = list(blocks)
    if not blocks or not SW.fused_addln:
        for i, blk in enumerate(blocks):
            x = blk(x, rope, cache, i)
        return final_norm(x)
    y = blocks[0].ln_1(x)
    for i, blk in enumerate(blocks):
        x, y = _add_norm(x, blk.attn(y, rope, cache, i), blk.ln_2, blk.mlp)
        nxt, cons = (blocks[i + 1].ln_1, blocks[i + 1].attn.c_attn) if i + 1 < len(blocks) else (final_norm, None)
        x, y = _add_norm(x, blk.mlp(y), nxt, cons)
    return y


def _add_norm(x, h, norm: RMSNorm, consumer):
    """add_rms_norm, or its fp8-emitting form when ``consumer`` (the module the normalised output feeds: a
    block's MLP, the next block's ``c_attn``, None for the final norm) runs an fp8 GEMM on it in training
    (ops/fp8.py fp8_input_slot; PDT_FP8_LN)."""
    if consumer is not None and consumer.training:
        t = fp8_input_slot(consumer, x)
        if t is not None and rms_fp8_ok(x, h, norm):
            return add_rms_norm_fp8(x, h, norm, t[0], t[1])
    return add_rms_norm(x, h, norm)


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig = LlamaConfig()):
        super().__init__()
        self.cfg = cfg
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(cfg.vocab_size, cfg.n_embd),
            h=nn.ModuleList([LlamaBlock(cfg) for _ in range(cfg.n_layer)]),
            ln_f=RMSNorm(cfg.n_embd, eps=cfg.eps),
        ))
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)  # untied
        self.rope = RotaryTable(cfg.block_size, cfg.rope_base, HEAD_DIM)  # non-persistent fp32 buffers
        init_weights(self, n_layer=cfg.n_layer)

    def _head(self, x: torch.Tensor) -> torch.Tensor:
        """The LM head on the cached path's rows (never the training fp8 path; decode-time rows as in
        ``_linear``)."""
        q = _w8(x, self.lm_head)
        if q is not None:
            return linear_skinny_w8(x, q[0], q[1])
        q = _w4(x, self.lm_head)
        if q is not None:
            return linear_w4(x, q[0], q[1])
        if _skinny(x, self.training):
            return linear_skinny(x, self.lm_head.weight)
        return linear(x, self.lm_head.weight)

    def forward(self, idx: torch.Tensor, targets: torch.Tensor | None = None):
        if idx.shape[1] > self.cfg.block_size:
            raise ValueError(f"sequence length {idx.shape[1]} exceeds block_size {self.cfg.block_size} "
                             "(the RoPE table)")
        x = F.embedding(idx, self.transformer.wte.weight)
        x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope)
        logits = linear(x, self.lm_head.weight)
        if targets is None:
            return logits
        return cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1))

    # ------------------------------------------------------------------ weight-only 8-bit decoding
    def _decode_linears(self):
        for blk in self.transformer.h:
            yield from (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj)
        yield self.lm_head

    @torch.no_grad()
    def quantize_decode_weights(self, dtype: str = "fp8", all_rows: bool = False) -> "Llama":
        """Quantise every block Linear and the LM head row-wise to e4m3 for decode-time calls (at most 64 rows,
        ``eval()``, no autograd): each module gets ``_w8 = (wq, scale, weight._version)`` as a plain attribute,
        not a parameter or buffer, so ``state_dict()`` is unchanged and the bf16 weights stay for everything
        else. ``dtype="int4"``: group-wise int4 instead (one fp32 scale per 128 inputs), kept as ``_w4`` in the
        same form. Either call removes what the other left. Call it again after the weights change.
        ``all_rows=True`` (int4 only) appends the flag to the ``_w4`` tuple: calls on more than 64 rows then run
        on the int4 copies too (``linear_w4``), so the prompt's K/V rows and the decode steps come from the same
        weights; the default leaves such calls on the bf16 weights."""
        if dtype not in ("fp8", "int4"):
            raise ValueError(f'quantize_decode_weights: dtype is "fp8" or "int4", got {dtype!r}')
        if all_rows and dtype == "fp8":
            raise NotImplementedError('quantize_decode_weights("fp8", all_rows=True): the W8A16 GEMM for more than 64 '
                                      'rows is not built (only the W8A16 skinny kernel reads e4m3 weights); use "int4"')
        self.drop_decode_weights()
        for mod in self._decode_linears():
            w = mod.weight.detach().to(torch.bfloat16)
            if dtype == "fp8":
                mod._w8 = (*quantize_rows_e4m3(w), mod.weight._version)
            else:
                mod._w4 = (*quantize_groups_int4(w), mod.weight._version, bool(all_rows))
        return self

    def drop_decode_weights(self) -> "Llama":
        for mod in self._decode_linears():
            for attr in ("_w8", "_w4"):
                if hasattr(mod, attr):
                    delattr(mod, attr)
        return self

    # ------------------------------------------------------------------ generation on a KV cache
    def new_cache(self, batch: int, capacity: int | None = None) -> KVCache:
        """A KV cache for ``batch`` sequences of up to ``capacity`` (default ``block_size``) positions, on the
        model's device and in its dtype."""
        w = self.lm_head.weight
        return KVCache(self.cfg.n_layer, batch, self.cfg.kv_heads, capacity or self.cfg.block_size, w.device, w.dtype)

    def new_paged_cache(self, slots: int, n_pages: int, max_pages_per_seq: int | None = None,
                        kv_dtype: str | None = None) -> PagedKVCache:
        """A paged KV cache of ``slots`` sequence slots on a pool of ``n_pages`` pages of 64 positions per layer;
        a slot may hold up to ``max_pages_per_seq`` pages (default: what ``block_size`` positions need). ``kv_dtype``
        None keeps the model's dtype; "fp8" stores e4m3 rows with one fp32 scale each (half the pool bytes per
        token and a bit: 66 against 128 per K or V row)."""
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f'new_paged_cache: kv_dtype is None or "fp8", got {kv_dtype!r}')
        w = self.lm_head.weight
        cache = PagedKVCache(self.cfg.n_layer, slots, self.cfg.kv_heads, n_pages,
                             max_pages_per_seq or -(-self.cfg.block_size // PAGE), w.device,
                             torch.float8_e4m3fn if kv_dtype == "fp8" else w.dtype)
        cache.table_len = self.cfg.block_size
        return cache

    def _prefill_paged(self, idx: torch.Tensor, cache: PagedKVCache, prompt_lens, slots) -> torch.Tensor:
        """``prefill`` of the admitted, empty slots ``slots`` (default: all of them) of a paged cache, whose pages
        ``cache.reserve(T0, slots)`` has handed out; the other slots are not touched."""
        b, T0 = idx.shape
        if slots is None:  # every slot runs: refuse before the forward, not after it has written the others' pages
            idle = [s for s in range(cache.slots) if not cache.is_active(s)]
            if idle:
                raise ValueError(f"prefill: slots {idle} of the paged cache are not admitted; admit() every slot, or "
                                 "name the ones to prefill with slots=")
        slots = list(range(cache.slots)) if slots is None else [int(s) for s in slots]
        if (cache.n_layer, cache.kv_heads) != (self.cfg.n_layer, self.cfg.kv_heads) or len(slots) != b:
            raise ValueError(f"paged cache for {cache.n_layer} layers x {cache.kv_heads} K/V heads does not fit this "
                             f"model ({self.cfg.n_layer} x {self.cfg.kv_heads}), or {len(slots)} slots for {b} prompts")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("the KV-cache path is inference only: call it under torch.no_grad()")
        if prompt_lens is not None:
            prompt_lens = _lens_arg(prompt_lens, b, 1, T0, idx.device, "prompt_lens")
        cache.select(slots)  # refuses slots that are not distinct and admitted
        try:
            x = F.embedding(idx, self.transformer.wte.weight)
            x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
        finally:
            cache.select(None)
        if prompt_lens is None:
            cache.set_lens(torch.full((b,), T0, dtype=torch.int32), slots=slots)
            last = x[:, -1]
        else:
            cache.set_lens(prompt_lens, bound=T0, slots=slots)
            last = x.gather(1, (prompt_lens.long() - 1)[:, None, None].expand(b, 1, x.shape[-1]))[:, 0]
        return self._head(last)

    def _check_cache(self, cache: KVCache, batch: int) -> None:
        if (cache.n_layer, cache.kv_heads) != (self.cfg.n_layer, self.cfg.kv_heads) or cache.batch != batch:
            raise ValueError(f"cache for {cache.n_layer} layers x {cache.kv_heads} K/V heads x batch {cache.batch} "
                             f"does not fit this model ({self.cfg.n_layer} x {self.cfg.kv_heads}) at batch {batch}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("the KV-cache path is inference only: call it under torch.no_grad()")

    def prefill(self, idx: torch.Tensor, cache: KVCache, prompt_lens=None, slots=None) -> torch.Tensor:
        """Run the prompts ``idx`` [B, T0] into an empty ``cache``; returns the logits [B, V] of every
        sequence's last prompt position (the LM head runs on those B rows only). Ragged prompts are
        right-padded and ``prompt_lens`` (B lengths in [1, T0]: a sequence, a CPU tensor, or a device tensor,
        which is clamped to that range rather than read) gives their lengths: all T0 rows are appended,
        then ``cache.lens = prompt_lens``; causality keeps the padding out of the real positions and the next
        append overwrites it.

        With a ``PagedKVCache`` and ``slots`` (B distinct admitted, empty slots, their pages reserved) only
        those sequences run and the other slots are not touched: this is how a sequence joins a running batch."""
        if isinstance(cache, PagedKVCache):
            return self._prefill_paged(idx, cache, prompt_lens, slots)
        if slots is not None:
            raise ValueError("prefill: slots names slots of a PagedKVCache; a KVCache's batch is fixed")
        B, T0 = idx.shape
        self._check_cache(cache, B)
        x = F.embedding(idx, self.transformer.wte.weight)
        x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
        if prompt_lens is None:
            cache.advance(T0)
            last = x[:, -1]
        else:
            if not isinstance(prompt_lens, torch.Tensor):
                prompt_lens = torch.as_tensor(prompt_lens, dtype=torch.int32)
            if prompt_lens.device.type == "cpu":
                if prompt_lens.shape != (B,) or int(prompt_lens.min()) < 1 or int(prompt_lens.max()) > T0:
                    raise ValueError(f"prompt_lens must be {B} lengths in [1, {T0}], got {prompt_lens.tolist()}")
                prompt_lens = prompt_lens.to(idx.device)
            else:
                prompt_lens = prompt_lens.clamp(1, T0)
            cache.set_lens(prompt_lens.to(torch.int32), bound=T0)
            last = x.gather(1, (prompt_lens.long() - 1)[:, None, None].expand(B, 1, x.shape[-1]))[:, 0]
        return self._head(last)

    def decode_step(self, tok: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """One token per sequence: ``tok`` [B] sits at position ``cache.lens[b]``; returns the logits [B, V]
        of the next one and advances ``cache.lens`` on the device after the last layer. Nothing here reads
        the device, so the step can be captured with ``torch.cuda.graph`` and replayed. On a ``PagedKVCache``
        ``tok`` is [slots] and every slot runs, so the shape is fixed: an inactive slot's row is computed and
        ignored (finite logits, its ``lens`` does not move); ``cache.reserve(1)`` comes before the step."""
        self._check_cache(cache, tok.shape[0])
        x = F.embedding(tok[:, None], self.transformer.wte.weight)
        x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
        cache.advance(1)
        return self._head(x[:, 0])

    def _extend_paged(self, idx: torch.Tensor, cache: PagedKVCache, new_lens, last_only: bool, slots) -> torch.Tensor:
        """``extend`` on the distinct admitted slots ``slots`` of a paged cache, whose pages
        ``cache.reserve(Tn, slots=slots)`` has handed out; the other slots are not touched."""
        b, Tn = idx.shape
        if slots is None:
            raise NotImplementedError("extend on a paged cache is a per-sequence operation: name the slots that run "
                                      "with slots= (slots=range(cache.slots) is the all-slot form)")
        slots = [int(s) for s in slots]
        if (cache.n_layer, cache.kv_heads) != (self.cfg.n_layer, self.cfg.kv_heads) or len(slots) != b:
            raise ValueError(f"paged cache for {cache.n_layer} layers x {cache.kv_heads} K/V heads does not fit this "
                             f"model ({self.cfg.n_layer} x {self.cfg.kv_heads}), or {len(slots)} slots for {b} rows")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("the KV-cache path is inference only: call it under torch.no_grad()")
        if Tn < 1:
            raise ValueError("extend: at least one new token per sequence")
        if new_lens is not None:
            new_lens = _lens_arg(new_lens, b, 0, Tn, idx.device, "new_lens")
        cache.select(slots)  # refuses slots that are not distinct and admitted
        cache.extending = True
        try:
            x = F.embedding(idx, self.transformer.wte.weight)
            x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
            if new_lens is not None:  # the selected rows of lens, gathered before the forward
                moved = cache.view()[1] + new_lens
        finally:
            cache.extending = False
            cache.select(None)
        if new_lens is None:
            cache.advance(Tn, slots)
        else:
            cache.set_lens(moved, bound=[cache.bounds[s] + Tn for s in slots], slots=slots)
        if last_only:
            if new_lens is None:
                x = x[:, -1]
            else:  # a sequence that got nothing returns its row 0: the caller keeps what it had
                x = x.gather(1, (new_lens.long() - 1).clamp(min=0)[:, None, None].expand(b, 1, x.shape[-1]))[:, 0]
        return self._head(x)

    def extend(self, idx: torch.Tensor, cache: KVCache, new_lens=None, last_only: bool = False,
               slots=None) -> torch.Tensor:
        """Append ``idx`` [B, Tn] at positions ``cache.lens[b] + t`` of a cache that may already hold a
        conversation (a later turn's prompt, a slice of a chunked prefill, drafted tokens to verify: the
        caller rolls back with ``cache.set_lens``). Returns the logits [B, Tn, V]; with ``last_only`` [B, V]
        of every sequence's last valid new row (the LM head runs on those B rows only). ``cache.lens``
        advances by Tn, or, for right-padded ragged input, by ``new_lens[b]`` in [0, Tn] (a sequence, a CPU
        tensor, or a device tensor, which is clamped rather than read); the next append overwrites the
        padding rows. Tn == 1 runs the split-KV decode kernel, Tn > 1 the multi-token append kernel, on an
        empty cache too. With ``new_lens`` None or on the device nothing here reads the device, so the call
        can be captured like ``decode_step``.

        On a ``PagedKVCache`` ``slots`` names the B distinct admitted slots that run (their pages come from
        ``cache.reserve(Tn, slots=slots)`` beforehand): the paged append kernel for Tn > 1, and only their
        ``lens`` and host bounds move; the other slots get no row and keep their ``lens``. This is how a long
        prompt joins a running batch in slices, a later turn lands on a slot's history and drafted tokens are
        verified (roll back with ``cache.set_lens(..., slots=slots)``). Without ``slots`` a paged cache raises
        ``NotImplementedError``: ``slots=range(cache.slots)`` is the all-slot form. The slot gather uploads an
        index, so this form is not captured."""
        if isinstance(cache, PagedKVCache):
            return self._extend_paged(idx, cache, new_lens, last_only, slots)
        if slots is not None:
            raise ValueError("extend: slots names slots of a PagedKVCache; a KVCache's batch is fixed")
        B, Tn = idx.shape
        self._check_cache(cache, B)
        if Tn < 1:
            raise ValueError("extend: at least one new token per sequence")
        if new_lens is not None:
            new_lens = _lens_arg(new_lens, B, 0, Tn, idx.device, "new_lens")
        x = F.embedding(idx, self.transformer.wte.weight)
        cache.extending = True
        try:
            x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
        finally:
            cache.extending = False
        if new_lens is None:
            cache.advance(Tn)
        else:
            cache.set_lens(cache.lens + new_lens, bound=cache.bound + Tn)
        if last_only:
            if new_lens is None:
                x = x[:, -1]
            else:  # a sequence that got nothing returns its row 0: the caller keeps what it had
                x = x.gather(1, (new_lens.long() - 1).clamp(min=0)[:, None, None].expand(B, 1, x.shape[-1]))[:, 0]
        return self._head(x)

    def _prefill_chunked(self, idx: torch.Tensor, cache: KVCache, prompt_lens, chunk: int) -> torch.Tensor:
        """``prefill`` in slices of ``chunk`` positions: the first through ``prefill``, the rest through
        ``extend(..., last_only=True)``; a sequence whose prompt ended in an earlier slice keeps its logits. On a
        paged cache (every slot admitted) each slice's pages are reserved just before it runs."""
        B, T0 = idx.shape
        if chunk < 1:
            raise ValueError(f"prefill_chunk must be positive, got {chunk}")
        if prompt_lens is not None:
            prompt_lens = _lens_arg(prompt_lens, B, 1, T0, idx.device, "prompt_lens")
        paged = isinstance(cache, PagedKVCache)
        kw = dict(slots=range(B)) if paged else {}
        first = min(chunk, T0)
        if paged:
            cache.reserve(first)
        logits = self.prefill(idx[:, :first], cache, None if prompt_lens is None else prompt_lens.clamp(max=first))
        for s in range(first, T0, chunk):
            part = idx[:, s:s + chunk]
            if paged:
                cache.reserve(part.shape[1])
            if prompt_lens is None:
                logits = self.extend(part, cache, last_only=True, **kw)
            else:
                n = (prompt_lens - s).clamp(0, part.shape[1])
                logits = torch.where((n > 0)[:, None], self.extend(part, cache, new_lens=n, last_only=True, **kw),
                                     logits)
        return logits

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, top_k: int | None = None,
                 eos_token: int | None = None, generator: torch.Generator | None = None, prompt_lens=None,
                 return_logits: bool = False, prefill_chunk: int | None = None, paged: bool = False,
                 kv_dtype: str | None = None, top_p=None, sampler: str = "torch"):
        """Sample ``max_new_tokens`` tokens after the prompts ``idx`` [B, T0] (right-padded when
        ``prompt_lens`` is given); returns them as [B, max_new_tokens] on the device, with ``return_logits``
        also the logits [B, max_new_tokens, V] each was drawn from. Greedy at ``temperature`` 0, otherwise
        ``torch.multinomial`` of softmax(logits / temperature) (restricted to the ``top_k`` largest) on
        ``generator``. With ``eos_token`` everything after a sequence's first EOS is EOS (a device-side mask:
        no step reads a token on the host). With ``prefill_chunk`` the prompt runs in slices of that many
        positions (``prefill`` of the first, ``extend`` of the rest), which bounds the activation memory of a
        long prompt by the slice. With ``paged`` the same loop runs on a ``PagedKVCache`` sized for the batch,
        which reserves pages before the prefill (with ``prefill_chunk``: before every slice) and before every
        step; ``kv_dtype="fp8"`` makes that cache an e4m3 one (``new_paged_cache``), which takes the prompt whole:
        with ``prefill_chunk`` it is refused. ``sampler="fused"`` draws every token with one launch of the
        HIP sampler instead (``ops/sampling.py``: adds nucleus sampling ``top_p``, accepts ``temperature`` /
        ``top_k`` / ``top_p`` as per-sequence [B] tensors, and draws from a Philox counter seeded from
        ``generator.initial_seed()``, 0 without one, so a run is a function of the seed); ``top_p`` with the
        ``"torch"`` sampler is refused. Runs in ``eval()`` and restores the mode."""
        B, T0 = idx.shape
        if sampler not in ("torch", "fused"):
            raise ValueError(f"generate: sampler must be 'torch' or 'fused', got {sampler!r}")
        if sampler == "torch" and top_p is not None:
            raise ValueError("generate: top_p needs sampler='fused' (the torch sampler has no nucleus filter)")
        if sampler == "fused":
            state = SamplerState(generator.initial_seed() if generator is not None else 0)

            def draw(logits):
                return sample_fused(logits.contiguous(), temperature, top_k, top_p, state=state)
        else:
            def draw(logits):
                return _sample(logits, temperature, top_k, generator)
        if kv_dtype is not None and not paged:
            raise NotImplementedError(f"generate: kv_dtype = {kv_dtype!r} needs paged=True; an fp8 contiguous KVCache is "
                                      "out of scope")
        if kv_dtype is not None and prefill_chunk is not None:
            raise NotImplementedError("generate: prefill_chunk on an fp8 paged cache is out of scope (it needs the e4m3 "
                                      "form of the multi-token append kernel)")
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be positive, got {max_new_tokens}")
        if T0 + max_new_tokens > self.cfg.block_size:
            raise ValueError(f"prompt of {T0} + {max_new_tokens} new tokens exceeds block_size {self.cfg.block_size} "
                             "(the RoPE table)")
        was_training = self.training
        self.eval()
        try:
            if paged:
                per_seq = -(-(T0 + max_new_tokens) // PAGE)
                cache = self.new_paged_cache(B, B * per_seq, per_seq, kv_dtype=kv_dtype)
                for s in range(B):
                    cache.admit(s)
                if prefill_chunk is None:
                    cache.reserve(T0)
            else:
                cache = self.new_cache(B, T0 + max_new_tokens)
            if prefill_chunk is None:
                logits = self.prefill(idx, cache, prompt_lens)
            else:
                logits = self._prefill_chunked(idx, cache, prompt_lens, prefill_chunk)
            toks, all_logits = [], []
            done = torch.zeros(B, dtype=torch.bool, device=idx.device)
            for i in range(max_new_tokens):
                tok = draw(logits)
                if eos_token is not None:
                    tok = torch.where(done, torch.full_like(tok, eos_token), tok)
                    done = done | (tok == eos_token)
                toks.append(tok)
                if return_logits:
                    all_logits.append(logits)
                if i + 1 < max_new_tokens:
                    if paged:
                        cache.reserve(1)
                    logits = self.decode_step(tok, cache)
        finally:
            self.train(was_training)
        out = torch.stack(toks, 1)
        return (out, torch.stack(all_logits, 1)) if return_logits else out


def _lens_arg(lens, batch: int, lo: int, hi: int, device, name: str) -> torch.Tensor:
    """``lens`` as int32 [batch] on ``device``: a sequence or a CPU tensor is checked against [lo, hi], a
    device tensor is clamped to it rather than read."""
    if not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(lens, dtype=torch.int32)
    if lens.device.type == "cpu":
        if lens.shape != (batch,) or int(lens.min()) < lo or int(lens.max()) > hi:
            raise ValueError(f"{name} must be {batch} lengths in [{lo}, {hi}], got {lens.tolist()}")
        return lens.to(device=device, dtype=torch.int32)
    return lens.clamp(lo, hi).to(torch.int32)


def _sample(logits: torch.Tensor, temperature: float, top_k: int | None, generator) -> torch.Tensor:
    """One token id per row of ``logits`` [B, V]: the argmax at temperature 0, else a draw from
    softmax(logits / temperature) over the ``top_k`` largest logits (all of them when None)."""
    if temperature <= 0.0:
        return logits.argmax(-1)
    z = logits.float() / temperature
    if top_k is not None and top_k < z.shape[-1]:
        kth = z.topk(top_k, dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    return torch.multinomial(torch.softmax(z, -1), 1, generator=generator)[:, 0]


def from_hf_state_dict(sd: Dict[str, torch.Tensor], n_kv_head: int | None = None) -> Dict[str, torch.Tensor]:
    """A Hugging Face ``LlamaForCausalLM`` state dict (head dim 64) in this file's layout: q/k/v rows
    concatenated into ``c_attn``, gate/up rows into ``c_fc``. A grouped-query checkpoint (k/v projections
    of ``num_key_value_heads·64`` rows) needs ``n_kv_head`` = that count, which is also the ``n_kv_head``
    of the ``LlamaConfig`` to load it into; without it only multi-head state dicts are accepted.

    No row permutation is needed: HF applies RoPE in the half-split ``rotate_half`` convention, pair
    (j, j + 32) of each head, which is the convention of ops/rope.py. (The interleaved pairs
    (2j, 2j + 1) of the original Meta checkpoints are permuted away when those are converted to HF.)"""
    out: Dict[str, torch.Tensor] = {
        "transformer.wte.weight": sd["model.embed_tokens.weight"],
        "transformer.ln_f.weight": sd["model.norm.weight"],
        "lm_head.weight": sd["lm_head.weight"] if "lm_head.weight" in sd else sd["model.embed_tokens.weight"],
    }
    i = 0
    while f"model.layers.{i}.input_layernorm.weight" in sd:
        src, dst = f"model.layers.{i}.", f"transformer.h.{i}."
        q, k, v = (sd[f"{src}self_attn.{n}_proj.weight"] for n in ("q", "k", "v"))
        if n_kv_head is None:
            if not (q.shape == k.shape == v.shape):
                raise ValueError(f"layer {i}: grouped-query attention (k/v {tuple(k.shape)} against q "
                                 f"{tuple(q.shape)}) needs n_kv_head: pass from_hf_state_dict(sd, n_kv_head="
                                 "num_key_value_heads)")
        elif not (k.shape == v.shape == (n_kv_head * HEAD_DIM, q.shape[1]) and q.shape[0] % k.shape[0] == 0):
            raise ValueError(f"layer {i}: k/v {tuple(k.shape)}, {tuple(v.shape)} are not n_kv_head·{HEAD_DIM} = "
                             f"{n_kv_head * HEAD_DIM} rows each dividing q's {q.shape[0]}")
        out[dst + "ln_1.weight"] = sd[src + "input_layernorm.weight"]
        out[dst + "attn.c_attn.weight"] = torch.cat([q, k, v], 0)
        out[dst + "attn.c_proj.weight"] = sd[src + "self_attn.o_proj.weight"]
        out[dst + "ln_2.weight"] = sd[src + "post_attention_layernorm.weight"]
        out[dst + "mlp.c_fc.weight"] = torch.cat([sd[src + "mlp.gate_proj.weight"], sd[src + "mlp.up_proj.weight"]], 0)
        out[dst + "mlp.c_proj.weight"] = sd[src + "mlp.down_proj.weight"]
        i += 1
    return out


# the registered presets: what each overrides of LlamaConfig's defaults (llama_medium's)
PRESETS = {
    "llama_medium": {},  # GPT-2-medium's depth and width (24 x 1024, 16 heads), F = 2816
    "llama_small": dict(n_layer=12, n_head=12, n_embd=768, ffn=2048),
    "llama_tiny": dict(n_layer=2, n_head=4, n_embd=256, ffn=768, block_size=64, vocab_size=512),  # for tests
}
PRESETS["llama_tiny_gqa"] = dict(PRESETS["llama_tiny"], n_kv_head=2)  # 2 K/V heads for its 4 query heads


def _preset(name: str, kw: dict) -> Llama:
    return Llama(LlamaConfig(**{**PRESETS[name], **kw}))


def llama_medium(**kw) -> Llama:
    return _preset("llama_medium", kw)


def llama_small(**kw) -> Llama:
    return _preset("llama_small", kw)


def llama_tiny(**kw) -> Llama:
    return _preset("llama_tiny", kw)


def llama_tiny_gqa(**kw) -> Llama:
    return _preset("llama_tiny_gqa", kw)


def n_heads(model_name: str) -> int | None:
    """The query-head count of a registered preset (None for any other name), without building the model."""
    return LlamaConfig(**PRESETS[model_name]).n_head if model_name in PRESETS else None


from . import register  # noqa: E402

register("llama_medium", llama_medium)
register("llama_small", llama_small)
register("llama_tiny", llama_tiny)
register("llama_tiny_gqa", llama_tiny_gqa)
