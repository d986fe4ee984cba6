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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F
from torch import nn

from ..config import SW
from ..ops.attention import attention_decode, attention_qkv
from ..ops.cross_entropy import cross_entropy
from ..ops.fp8 import Fp8Act, add_rms_norm_fp8, fp8_input_slot, fp8_linear, fp8_ok, fp8_swiglu_mlp, rms_fp8_ok
from ..ops.kv_cache import KVCache
from ..ops.linear import linear
from ..ops.rmsnorm import RMSNorm, add_rms_norm
from ..ops.rope import RotaryTable, rope_append_, rope_qkv_
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


def _linear(x, mod: nn.Linear) -> torch.Tensor:
    """``mod``'s bias-free GEMM: fp8 when ``enable_fp8`` tagged it and the shape is served (ops/fp8.py; ``x``
    may then be an ``Fp8Act``, already e4m3 from ``add_rms_norm_fp8``), else bf16 (ops/linear.py)."""
    t = _fp8_tag(mod)
    if t is not None and (isinstance(x, Fp8Act) or fp8_ok(x, mod.weight)):
        return fp8_linear(x, mod.weight, None, t[0], t[1])
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
        (Tn == 1) the split-KV kernel on the cache. ``cache.lens`` is advanced by the caller after the last layer."""
        Tn = x.shape[1]
        if Tn > 1 and cache.bound > 0:
            raise ValueError(f"{Tn} new tokens onto a cache that may hold {cache.bound} positions: chunked prefill "
                             "is not supported (prefill an empty cache, then decode one token at a time)")
        cache.require(Tn, rope.cos.shape[0])
        qkv = _linear(x, self.c_attn)
        qkv = rope_append_(qkv, rope.cos, rope.sin, self.heads, self.kv_heads, cache.k[layer], cache.v[layer],
                           cache.lens)
        if Tn > 1:
            y = attention_qkv(qkv, self.heads, causal=True, kv_heads=self.kv_heads)
        else:
            y = attention_decode(qkv, cache.k[layer], cache.v[layer], cache.lens, self.heads, self.kv_heads,
                                 cache=cache)
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

    # ------------------------------------------------------------------ generation on a KV cache
    def new_cache(self, batch: int, capacity: int | None = None) -> KVCache:
        """A KV cache for ``batch`` sequences of up to ``capacity`` (default ``block_size``) positions, on the
        model's device and in its dtype."""
        w = self.lm_head.weight
        return KVCache(self.cfg.n_layer, batch, self.cfg.kv_heads, capacity or self.cfg.block_size, w.device, w.dtype)

    def _check_cache(self, cache: KVCache, batch: int) -> None:
        if (cache.n_layer, cache.kv_heads) != (self.cfg.n_layer, self.cfg.kv_heads) or cache.batch != batch:
            raise ValueError(f"cache for {cache.n_layer} layers x {cache.kv_heads} K/V heads x batch {cache.batch} "
                             f"does not fit this model ({self.cfg.n_layer} x {self.cfg.kv_heads}) at batch {batch}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("the KV-cache path is inference only: call it under torch.no_grad()")

    def prefill(self, idx: torch.Tensor, cache: KVCache, prompt_lens=None) -> torch.Tensor:
        """Run the prompts ``idx`` [B, T0] into an empty ``cache``; returns the logits [B, V] of every
        sequence's last prompt position (the LM head runs on those B rows only). Ragged prompts are
        right-padded and ``prompt_lens`` (B lengths in [1, T0]: a sequence, a CPU tensor, or a device tensor,
        which is clamped to that range rather than read) gives their lengths: all T0 rows are appended,
        then ``cache.lens = prompt_lens``; causality keeps the padding out of the real positions and the next
        append overwrites it."""
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
        return linear(last, self.lm_head.weight)

    def decode_step(self, tok: torch.Tensor, cache: KVCache) -> torch.Tensor:
        """One token per sequence: ``tok`` [B] sits at position ``cache.lens[b]``; returns the logits [B, V]
        of the next one and advances ``cache.lens`` on the device after the last layer. Nothing here reads
        the device, so the step can be captured with ``torch.cuda.graph`` and replayed."""
        self._check_cache(cache, tok.shape[0])
        x = F.embedding(tok[:, None], self.transformer.wte.weight)
        x = run_llama_blocks(self.transformer.h, x, self.transformer.ln_f, self.rope, cache)
        cache.advance(1)
        return linear(x[:, 0], self.lm_head.weight)

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, top_k: int | None = None,
                 eos_token: int | None = None, generator: torch.Generator | None = None, prompt_lens=None,
                 return_logits: bool = False):
        """Sample ``max_new_tokens`` tokens after the prompts ``idx`` [B, T0] (right-padded when
        ``prompt_lens`` is given); returns them as [B, max_new_tokens] on the device, with ``return_logits``
        also the logits [B, max_new_tokens, V] each was drawn from. Greedy at ``temperature`` 0, otherwise
        ``torch.multinomial`` of softmax(logits / temperature) (restricted to the ``top_k`` largest) on
        ``generator``. With ``eos_token`` everything after a sequence's first EOS is EOS (a device-side mask:
        no step reads a token on the host). Runs in ``eval()`` and restores the mode."""
        B, T0 = idx.shape
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be positive, got {max_new_tokens}")
        if T0 + max_new_tokens > self.cfg.block_size:
            raise ValueError(f"prompt of {T0} + {max_new_tokens} new tokens exceeds block_size {self.cfg.block_size} "
                             "(the RoPE table)")
        was_training = self.training
        self.eval()
        try:
            cache = self.new_cache(B, T0 + max_new_tokens)
            logits = self.prefill(idx, cache, prompt_lens)
            toks, all_logits = [], []
            done = torch.zeros(B, dtype=torch.bool, device=idx.device)
            for i in range(max_new_tokens):
                tok = _sample(logits, temperature, top_k, generator)
                if eos_token is not None:
                    tok = torch.where(done, torch.full_like(tok, eos_token), tok)
                    done = done | (tok == eos_token)
                toks.append(tok)
                if return_logits:
                    all_logits.append(logits)
                if i + 1 < max_new_tokens:
                    logits = self.decode_step(tok, cache)
        finally:
            self.train(was_training)
        out = torch.stack(toks, 1)
        return (out, torch.stack(all_logits, 1)) if return_logits else out


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
