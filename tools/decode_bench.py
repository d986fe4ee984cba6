#!/usr/bin/env python
"""KV-cache decoding: the split-KV decode attention kernel against SDPA, and ``Llama.generate`` against
re-running the full forward on the growing sequence (all the parent commit can do).

Kernel: llama_medium's shape, B = 8, H = 16 query heads, Hkv in {16, 4, 1}, capacity 1024, lens in {128, 512,
1023} (lens + 1 keys are read), bf16. Candidates, taking turns within every round in one process, every
window timed with device events, median of the rounds (min-max). Every candidate is timed twice: "eager", a Python
loop of calls (at these sizes that is the host's launch rate, not the kernel), and "replayed", the same calls
captured once with torch.cuda.graph and replayed back to back, which is the device-side figure the bytes/s use:
  default   attention_decode with the default (S, C) of pdt_attn_decode_geo (split kernel + combine)
  S=1       splits=1: one workgroup per (sequence, K/V head) walks the whole cache, no combine
  sdpa      F.scaled_dot_product_attention on q [B, 16, 1, 64] and K/V materialised at 16 heads and cut to
            exactly lens + 1 keys (the expansion and the cut are not timed)
"must move" is the K and V bytes of the valid keys at Hkv heads, 2 B Hkv (lens + 1) 128, plus Q and O; the
achieved rate is that over the median time (for sdpa too, although it reads 16 heads: the rate of the
problem, not of its traffic).

Cache residency: one cache at this shape is 2 B Hkv 1024 128 bytes = 32 MiB at 16 K/V heads, 2 MiB at one: a
timing loop over one cache reads it from the 256 MB last-level cache, not from HBM. Each candidate is
therefore timed twice: "warm" on one cache, and "rotating" over as many distinct caches as make 512 MiB (at
most 64: the small shapes stay cache-resident even so, and their lines say how many bytes rotate).

Generation: llama_medium (and --kv-heads 4), bf16, 8 sequences, a 128-token prompt and 128 new tokens,
greedy, in one process on the same weights:
  generate  Llama.generate, eager
  graph     prefill, then one decode step captured with torch.cuda.graph and replayed (argmax and the token
            copy between replays stay on the device)
  full      128 times model(idx) on the growing sequence, argmax of the last position
and the per-token time of the decode steps alone, eager and replayed.

--extend: the multi-token append kernel instead. The same shape, Tn in {4, 8, 64} new tokens per sequence at
lens in {128, 1023 - Tn} (the count before the append; lens + Tn keys are read). Candidates, each captured
once and replayed, taking turns within every round, over rotating caches, device events, median of the rounds:
  extend    one attention_extend call (default geometry)
  decodes   Tn successive attention_decode calls at lens + t on the same cache (all the parent commit can do)
  sdpa      F.scaled_dot_product_attention with an explicit [Tn, lens + Tn] mask on K/V materialised at 16
            heads and cut to lens + Tn keys (the expansion and the cut are not timed)

--gemm-w8: the decode-time Linears on e4m3 weights. llama_medium's five Linears (and c_fc + SwiGLU) at M in
{1, 8, 16, 32, 64}: the W8A16 skinny GEMM, the bf16 skinny GEMM and F.linear, the --gemm recipe (captured and
replayed, weights rotating through 512 MiB of distinct copies, alternating, device events, median of the rounds);
each line's rate is over the bytes that candidate must move. Then the generation A/B under PDT_DECODE_GEMM=1:
the captured step and 128 tokens after a 128-token prompt, bf16 weights against quantize_decode_weights().

--gemm-w4: the decode-time Linears on group-wise int4 weights. The --gemm-w8 shapes and recipe with two candidates,
the W4A16 skinny GEMM and the W8A16 one (the reference of every time), each rotating through its own 512 MiB of
distinct copies; the bytes a candidate must move include its scales. Then the captured step and 128 tokens after a
128-token prompt on quantize_decode_weights() against quantize_decode_weights("int4").

--gemm-w4-tall: the any-row W4A16 GEMM (csrc/kernels/gemm_w4.hip). llama_medium's five weight shapes at M in
{128, 512, 2048}: the kernel, F.linear on the bf16 weight (what such rows run without all_rows) and dequantise +
F.linear take turns in one process, the --gemm-w4 recipe. Then llama_medium with 8 paged slots: a 512-token prefill
and the captured decode step on quantize_decode_weights("int4") with and without all_rows=True.

--paged: the paged decode kernel. The kernel table's shapes and recipe (captured and replayed, rotating caches,
alternating, device events, median of the rounds): attention_decode_paged with a sequential block table and
with a seeded shuffled one against attention_decode on the same keys, and whether the three give the same
bits; then llama_medium's captured decode step on a KVCache and on a PagedKVCache.

--paged-fp8: the e4m3 paged decode kernel. The --paged recipe with the bf16 paged kernel as the reference of every
time: attention_decode_paged and attention_decode_paged_fp8 under one shuffled block table take turns in one process,
then llama_medium's captured decode step on a bf16 and on an e4m3 PagedKVCache, and the pool bytes per token.

--paged --extend: the paged append kernel. The --extend table's shapes and recipe: attention_extend (the reference
of every time) and attention_extend_paged with a sequential and a seeded shuffled block table take turns in one
process, captured and replayed, over rotating caches, and whether the three give the same bits; then llama_medium
with 8 paged slots, a 512-token prompt joining in slices of 64 against the same prompt as one paged prefill.

--sampler: the fused top-k / top-p sampler (ops/sampling.py). bf16 logits [B, 32000], B in {1, 8, 64}, rotating through
16 distinct buffers; greedy, T = 0.8, T = 0.8 with k = 50, and that with p = 0.9. The fused call against the aten chain
of models/llama.py:_sample (which has no top-p), taking turns, device events, median of the rounds; the fused call
eager and captured, the chain eager only (its aten kernels record memset nodes, which do not replay safely here). Then llama_medium's 128-after-128-token generation on the
captured step with either sampler between the replays.

    python tools/decode_bench.py [--rounds 7] [--iters 50] [--gen-rounds 3] [--no-generate] [--extend] [--paged] [--paged-fp8] [--out FILE]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, H, DH, CAP = 8, 16, 64, 1024
KV_HEADS = (16, 4, 1)
LENS = (128, 512, 1023)
ROTATE_BYTES = 512 << 20


def _time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _graphed(fn, iters):
    """``iters`` calls captured once: a replay runs them back to back without the host's launch cost."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(iters):
            fn(i)
    return graph


def _alternate(cands, rounds, iters):
    """{name: ([ms per call eager], [ms per call replayed])}, one entry per round; the candidates take turns."""
    for fn in cands.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    graphs = {k: _graphed(fn, iters) for k, fn in cands.items()}
    out = {k: ([], []) for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k][0].append(_time_ms(fn, iters))
            out[k][1].append(_time_ms(lambda i, g=graphs[k]: g.replay(), 1) / iters)
    return out


def bench_kernel(rounds, iters, emit):
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode, attention_decode_geo
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    for hkv in KV_HEADS:
        cache_bytes = 2 * B * hkv * CAP * DH * 2
        ncopy = max(1, min(64, ROTATE_BYTES // cache_bytes))
        # one KVCache of ncopy "layers": distinct K/V allocations that share lens and the scratch
        cache = KVCache(ncopy, B, hkv, CAP, dev)
        for l in range(ncopy):
            cache.k[l].copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
            cache.v[l].copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
        qkv = torch.randn(B, 1, (H + 2 * hkv) * DH, device=dev, generator=g).bfloat16()
        S, C = attention_decode_geo(B, hkv, CAP, None, H // hkv)
        emit(f"## Hkv = {hkv} (G = {H // hkv}): default (S, C) = ({S}, {C}), {S * hkv * B} workgroups; S=1: {hkv * B} "
             f"workgroups; one cache {cache_bytes / 2**20:.0f} MiB, rotating over {ncopy} ({ncopy * cache_bytes / 2**20:.0f} MiB)")
        for lens in LENS:
            n = lens + 1
            cache.set_lens([lens] * B)
            must = 2 * B * hkv * n * DH * 2 + 2 * B * H * DH * 2
            q4 = qkv[:, 0, :H * DH].reshape(B, H, 1, DH)
            ke = [cache.k[l][:, :, :n].repeat_interleave(H // hkv, dim=1).contiguous() for l in range(ncopy)]
            ve = [cache.v[l][:, :, :n].repeat_interleave(H // hkv, dim=1).contiguous() for l in range(ncopy)]

            def ours(splits, rot):
                return lambda i: attention_decode(qkv, cache.k[i % ncopy if rot else 0], cache.v[i % ncopy if rot else 0],
                                                  cache.lens, H, hkv, scale, splits=splits, cache=cache)

            def sdpa(rot):
                return lambda i: F.scaled_dot_product_attention(q4, ke[i % ncopy if rot else 0],
                                                                ve[i % ncopy if rot else 0], scale=scale)

            cands = {}
            for rot in (False, True):
                tag = "rotating" if rot else "warm"
                cands[f"default {tag}"] = ours(None, rot)
                cands[f"S=1     {tag}"] = ours(1, rot)
                cands[f"sdpa    {tag}"] = sdpa(rot)
            # same answer before timing it (bf16 output: the two differ by roundings)
            a = attention_decode(qkv, cache.k[0], cache.v[0], cache.lens, H, hkv, scale, cache=cache)
            b_ = sdpa(False)(0).transpose(1, 2).reshape(B, 1, H * DH)
            err = (a.float() - b_.float()).abs().max().item()
            t = _alternate(cands, rounds, iters)
            for name, (te, tg) in t.items():
                me, m = statistics.median(te), statistics.median(tg)
                emit(f"lens {lens:5d}  {name:<17} eager {me * 1e3:6.1f} us  replayed {m * 1e3:6.1f} us "
                     f"({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  must move {must / 1e6:6.2f} MB  {must / m / 1e9:6.2f} TB/s")
            emit(f"lens {lens:5d}  max |ours - sdpa| = {err:.3g}")
        del cache, ke, ve


def bench_paged(rounds, iters, emit):
    """--paged: attention_decode_paged under a sequential and a seeded shuffled block table against
    attention_decode (the contiguous kernel, unchanged) on the shapes of bench_kernel, the same keys in all
    three, every candidate captured and replayed over rotating caches, and whether the bits agree."""
    from pytorch_distributed_training_example_amd.ops.attention import (attention_decode, attention_decode_geo,
                                                                         attention_decode_paged)
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    MP = CAP // 64
    perm = torch.randperm(B * MP, generator=torch.Generator().manual_seed(0)).to(dev)
    tables = {"paged seq ": torch.arange(B * MP, device=dev, dtype=torch.int32).view(B, MP),
              "paged shuf": perm.to(torch.int32).view(B, MP).contiguous()}
    for hkv in KV_HEADS:
        cache_bytes = 2 * B * hkv * CAP * DH * 2
        ncopy = max(1, min(64, ROTATE_BYTES // cache_bytes))
        cache = KVCache(ncopy, B, hkv, CAP, dev)
        pools = {k: ([], []) for k in tables}
        for l in range(ncopy):
            for c, which in ((cache.k[l], 0), (cache.v[l], 1)):
                c.copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
                seq = c.view(B, hkv, MP, 64, DH).permute(0, 2, 1, 3, 4).reshape(B * MP, hkv, 64, DH).contiguous()
                shuf = torch.empty_like(seq)
                shuf[perm] = seq  # logical page i lives in pool page perm[i]
                pools["paged seq "][which].append(seq)
                pools["paged shuf"][which].append(shuf)
        qkv = torch.randn(B, 1, (H + 2 * hkv) * DH, device=dev, generator=g).bfloat16()
        S, C = attention_decode_geo(B, hkv, CAP, None, H // hkv)
        emit(f"## Hkv = {hkv} (G = {H // hkv}): (S, C) = ({S}, {C}) for all three, {S * hkv * B} workgroups; one cache "
             f"{cache_bytes / 2**20:.0f} MiB, rotating over {ncopy} ({ncopy * cache_bytes / 2**20:.0f} MiB)")
        for lens in LENS:
            cache.set_lens([lens] * B)
            must = 2 * B * hkv * (lens + 1) * DH * 2 + 2 * B * H * DH * 2
            cands = {"contiguous": lambda i: attention_decode(qkv, cache.k[i % ncopy], cache.v[i % ncopy], cache.lens, H, hkv,
                                                              scale, cache=cache)}
            for name, table in tables.items():
                cands[name] = lambda i, kp=pools[name][0], vp=pools[name][1], t=table: attention_decode_paged(
                    qkv, kp[i % ncopy], vp[i % ncopy], t, cache.lens, H, hkv, scale, cache=cache)
            ref = attention_decode(qkv, cache.k[0], cache.v[0], cache.lens, H, hkv, scale, cache=cache, return_lse=True)
            same = []
            for name, table in tables.items():
                o, lse = attention_decode_paged(qkv, pools[name][0][0], pools[name][1][0], table, cache.lens, H, hkv, scale,
                                                cache=cache, return_lse=True)
                same.append(f"{name.strip()}: O {bool(torch.equal(o, ref[0]))}, LSE {bool(torch.equal(lse, ref[1]))}")
            t = _alternate(cands, rounds, iters)
            base = statistics.median(t["contiguous"][1])
            for name, (te, tg) in t.items():
                m = statistics.median(tg)
                emit(f"lens {lens:5d}  {name:<10} replayed {m * 1e3:6.1f} us ({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  "
                     f"{m / base:5.2f}x contiguous  must move {must / 1e6:6.2f} MB  {must / m / 1e9:6.2f} TB/s")
            emit(f"lens {lens:5d}  bits equal to the contiguous kernel's: " + "; ".join(same))
        del cache, pools


def bench_paged_fp8(rounds, iters, emit):
    """--paged-fp8: attention_decode_paged_fp8 against attention_decode_paged (the reference of every time) on the
    shapes of bench_kernel, the --paged recipe: shuffled block table, the e4m3 pools quantised from the bf16 pools'
    rows, both captured and replayed over rotating caches, taking turns in one process."""
    from pytorch_distributed_training_example_amd.ops.attention import (attention_decode_geo, attention_decode_paged,
                                                                         attention_decode_paged_fp8)
    from pytorch_distributed_training_example_amd.ops.kv_cache import PagedKVCache
    from pytorch_distributed_training_example_amd.ops.linear import quantize_rows_e4m3
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    MP = CAP // 64
    table = torch.randperm(B * MP, generator=torch.Generator().manual_seed(0)).to(dev).to(torch.int32).view(B, MP).contiguous()
    for hkv in KV_HEADS:
        cache_bytes = 2 * B * hkv * CAP * DH * 2
        ncopy = max(1, min(64, ROTATE_BYTES // cache_bytes))  # as many copies of both caches as the bf16 one rotates over
        cache = PagedKVCache(1, B, hkv, 1, MP, dev)  # lens and the split scratch
        bf, q8 = ([], []), ([], [], [], [])
        for l in range(ncopy):
            for which in (0, 1):
                pool = torch.randn(B * MP, hkv, 64, DH, device=dev, generator=g).bfloat16()
                bf[which].append(pool)
                q, sc = quantize_rows_e4m3(pool.view(-1, DH))
                q8[which].append(q.view(pool.shape))
                q8[2 + which].append(sc.view(pool.shape[:3]))
        qkv = torch.randn(B, 1, (H + 2 * hkv) * DH, device=dev, generator=g).bfloat16()
        S, C = attention_decode_geo(B, hkv, CAP, None, H // hkv)
        emit(f"## Hkv = {hkv} (G = {H // hkv}): (S, C) = ({S}, {C}) for both, {S * hkv * B} workgroups; one bf16 cache "
             f"{cache_bytes / 2**20:.0f} MiB, one e4m3 cache with scales {cache_bytes * 66 / 128 / 2**20:.0f} MiB, rotating over "
             f"{ncopy} of each")
        for lens in LENS:
            cache.lens.fill_(lens)
            rows = 2 * B * hkv * (lens + 1)
            must = {"paged bf16": rows * DH * 2 + 2 * B * H * DH * 2, "paged fp8 ": rows * (DH + 4) + 2 * B * H * DH * 2}
            cands = {"paged bf16": lambda i: attention_decode_paged(qkv, bf[0][i % ncopy], bf[1][i % ncopy], table, cache.lens,
                                                                    H, hkv, scale, cache=cache),
                     "paged fp8 ": lambda i: attention_decode_paged_fp8(qkv, q8[0][i % ncopy], q8[1][i % ncopy],
                                                                        q8[2][i % ncopy], q8[3][i % ncopy], table, cache.lens,
                                                                        H, hkv, scale, cache=cache)}
            err = (cands["paged fp8 "](0).float() - cands["paged bf16"](0).float()).abs().max().item()
            t = _alternate(cands, rounds, iters)
            base = statistics.median(t["paged bf16"][1])
            for name, (te, tg) in t.items():
                m = statistics.median(tg)
                emit(f"lens {lens:5d}  {name:<10} replayed {m * 1e3:6.1f} us ({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  "
                     f"{m / base:5.2f}x paged bf16  must move {must[name] / 1e6:6.2f} MB  {must[name] / m / 1e9:6.2f} TB/s")
            emit(f"lens {lens:5d}  max |O fp8 - O bf16| = {err:.3g} (the e4m3 rounding of the rows)")
        del cache, bf, q8


def bench_paged_step(rounds, emit, prompt=128, steps=32, names=("contiguous", "paged")):
    """--paged: llama_medium's captured decode step at positions prompt .. prompt + steps - 1 on a KVCache and on
    a PagedKVCache (pages reserved up front), the two graphs taking turns."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    tok = torch.zeros(B, dtype=torch.long, device="cuda")
    runs = {}
    with torch.no_grad():
        for name in names:
            if name != "contiguous":
                cache = model.new_paged_cache(B, B * 4, 4, kv_dtype="fp8" if name == "paged-fp8" else None)
                for s in range(B):
                    cache.admit(s)
                cache.reserve(prompt + steps + 4)
            else:
                cache = model.new_cache(B, prompt + steps + 4)
            model.prefill(idx, cache)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.set_lens([prompt] * B)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model.decode_step(tok, cache)
            runs[name] = (cache, graph, logits)
    out = {k: [] for k in runs}
    for _ in range(rounds + 1):  # the first round warms up
        for k, (cache, graph, _) in runs.items():
            cache.set_lens([prompt] * B)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            out[k].append(s.elapsed_time(e) / steps)
    for k, v in out.items():
        v = v[1:]
        emit(f"llama_medium kv_heads=16: captured decode step at position {prompt}..{prompt + steps - 1}, {k:<10} cache: "
             f"{statistics.median(v):.3f} ms ({min(v):.3f}-{max(v):.3f})")
    if "paged-fp8" in runs:
        per_tok = {k: sum(t.element_size() * t[0, 0, 0].numel() for pools in (c.k, c.v, c.k_scale or [], c.v_scale or [])
                          for t in pools) * c.kv_heads for k, (c, _, _) in runs.items()}
        emit("llama_medium: pool bytes per token, all layers: " + ", ".join(f"{k} {v}" for k, v in per_tok.items()))
        emit(f"llama_medium: max |logit| difference of the last replayed step between the two caches: "
             f"{(runs[names[0]][2].float() - runs[names[1]][2].float()).abs().max().item():.4g}")
        return
    emit("llama_medium: last replayed logits equal on the two caches: "
         f"{bool(torch.equal(runs['contiguous'][2], runs['paged'][2]))}")


def bench_paged_extend(rounds, iters, emit):
    """--paged --extend: attention_extend_paged under a sequential and a seeded shuffled block table against
    attention_extend (the contiguous kernel, the reference of every time) at bench_extend's shapes, the same keys
    in all three, each captured and replayed over rotating caches, taking turns; and whether the bits agree."""
    from pytorch_distributed_training_example_amd.ops.attention import (attention_extend, attention_extend_geo,
                                                                         attention_extend_paged)
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    MP = CAP // 64
    perm = torch.randperm(B * MP, generator=torch.Generator().manual_seed(0)).to(dev)
    tables = {"paged seq ": torch.arange(B * MP, device=dev, dtype=torch.int32).view(B, MP),
              "paged shuf": perm.to(torch.int32).view(B, MP).contiguous()}
    for hkv in KV_HEADS:
        cache_bytes = 2 * B * hkv * CAP * DH * 2
        ncopy = max(1, min(64, ROTATE_BYTES // cache_bytes))
        cache = KVCache(ncopy, B, hkv, CAP, dev)
        pools = {k: ([], []) for k in tables}
        for l in range(ncopy):
            for c, which in ((cache.k[l], 0), (cache.v[l], 1)):
                c.copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
                seq = c.view(B, hkv, MP, 64, DH).permute(0, 2, 1, 3, 4).reshape(B * MP, hkv, 64, DH).contiguous()
                shuf = torch.empty_like(seq)
                shuf[perm] = seq  # logical page i lives in pool page perm[i]
                pools["paged seq "][which].append(seq)
                pools["paged shuf"][which].append(shuf)
        emit(f"## Hkv = {hkv} (G = {H // hkv}): one cache {cache_bytes / 2**20:.0f} MiB, rotating over {ncopy} "
             f"({ncopy * cache_bytes / 2**20:.0f} MiB)")
        for tn in (4, 8, 64):
            qkv = torch.randn(B, tn, (H + 2 * hkv) * DH, device=dev, generator=g).bfloat16()
            geo = attention_extend_geo(B, hkv, CAP, tn, None, H // hkv)
            for lens in (128, CAP - 1 - tn):
                cache.set_lens([lens] * B)
                must = 2 * B * hkv * (lens + tn) * DH * 2 + 2 * B * tn * H * DH * 2
                cands = {"contiguous": lambda i: attention_extend(qkv, cache.k[i % ncopy], cache.v[i % ncopy], cache.lens,
                                                                  H, hkv, scale, cache=cache)}
                for name, table in tables.items():
                    cands[name] = lambda i, kp=pools[name][0], vp=pools[name][1], t=table: attention_extend_paged(
                        qkv, kp[i % ncopy], vp[i % ncopy], t, cache.lens, H, hkv, scale, cache=cache)
                ref = attention_extend(qkv, cache.k[0], cache.v[0], cache.lens, H, hkv, scale, cache=cache, return_lse=True)
                same = []
                for name, table in tables.items():
                    o, lse = attention_extend_paged(qkv, pools[name][0][0], pools[name][1][0], table, cache.lens, H, hkv,
                                                    scale, cache=cache, return_lse=True)
                    same.append(f"{name.strip()}: O {bool(torch.equal(o, ref[0]))}, LSE {bool(torch.equal(lse, ref[1]))}")
                graphs = {k: _graphed(fn, iters) for k, fn in cands.items()}
                t = {k: [] for k in cands}
                for _ in range(rounds):
                    for k in cands:
                        t[k].append(_time_ms(lambda i, gr=graphs[k]: gr.replay(), 1) / iters)
                base = statistics.median(t["contiguous"])
                for k, v in t.items():
                    m = statistics.median(v)
                    emit(f"Tn {tn:3d} lens {lens:5d}  {k:<10} {m * 1e3:7.1f} us ({min(v) * 1e3:.1f}-{max(v) * 1e3:.1f})  "
                         f"{m / base:5.2f}x contiguous ({(m - base) * 1e3:+.2f} us)  must move {must / 1e6:6.2f} MB  "
                         f"{must / m / 1e9:5.2f} TB/s")
                emit(f"Tn {tn:3d} lens {lens:5d}  geo (S, C, NB, NT) = {geo} for all three; bits equal to the contiguous "
                     "kernel's: " + "; ".join(same))
                del graphs
        del cache, pools


def bench_paged_join(rounds, emit, prompt=512, chunk=64):
    """--paged --extend: llama_medium, 8 slots of a PagedKVCache: a 512-token prompt per slot as one paged prefill
    against the same prompt joining in slices of 64 through extend(..., slots=range(8)), eager, taking turns."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()

    cache = model.new_paged_cache(B, B * (prompt // 64 + 1))

    def fresh():  # every slot given back and admitted again: both candidates pay it
        for s in range(B):
            cache.free(s)
            cache.admit(s)
        return cache

    @torch.no_grad()
    def whole():
        fresh().reserve(prompt)
        return model.prefill(idx, cache)

    @torch.no_grad()
    def sliced():
        return model._prefill_chunked(idx, fresh(), None, chunk)

    cands = {"one prefill": whole, f"slices of {chunk}": sliced}
    last = {k: fn() for k, fn in cands.items()}
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            out[k].append(s.elapsed_time(e))
    for k, v in out.items():
        emit(f"llama_medium kv_heads=16, {B} paged slots, {prompt}-token prompt, {k:<13}: {statistics.median(v):8.2f} ms "
             f"({min(v):.2f}-{max(v):.2f})")
    a, b = (v.float() for v in last.values())
    emit(f"llama_medium: last-position logits, slices against one prefill: max |difference| = {(a - b).abs().max().item():.3g} "
         f"of max |logit| = {b.abs().max().item():.3g}; argmax equal in {int((a.argmax(-1) == b.argmax(-1)).sum())} of {B}")


def bench_extend(rounds, iters, emit):
    from pytorch_distributed_training_example_amd.ops.attention import (attention_decode, attention_extend,
                                                                       attention_extend_geo)
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    for hkv in KV_HEADS:
        cache_bytes = 2 * B * hkv * CAP * DH * 2
        ncopy = max(1, min(64, ROTATE_BYTES // cache_bytes))
        cache = KVCache(ncopy, B, hkv, CAP, dev)
        for l in range(ncopy):
            cache.k[l].copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
            cache.v[l].copy_(torch.randn(B, hkv, CAP, DH, device=dev, generator=g))
        emit(f"## Hkv = {hkv} (G = {H // hkv}): one cache {cache_bytes / 2**20:.0f} MiB, rotating over {ncopy} "
             f"({ncopy * cache_bytes / 2**20:.0f} MiB)")
        for tn in (4, 8, 64):
            qkv = torch.randn(B, tn, (H + 2 * hkv) * DH, device=dev, generator=g).bfloat16()
            rows = [qkv[:, t:t + 1].contiguous() for t in range(tn)]
            geo = attention_extend_geo(B, hkv, CAP, tn, None, H // hkv)
            for lens in (128, CAP - 1 - tn):
                n = lens + tn
                cache.set_lens([lens] * B)
                lens_t = [cache.lens + t for t in range(tn)]
                must = 2 * B * hkv * n * DH * 2 + 2 * B * tn * H * DH * 2
                q4 = qkv[:, :, :H * DH].reshape(B, tn, H, DH).transpose(1, 2)
                ke = [cache.k[l][:, :, :n].repeat_interleave(H // hkv, dim=1).contiguous() for l in range(ncopy)]
                ve = [cache.v[l][:, :, :n].repeat_interleave(H // hkv, dim=1).contiguous() for l in range(ncopy)]
                mask = torch.arange(n, device=dev)[None, :] <= lens + torch.arange(tn, device=dev)[:, None]

                def extend(i):
                    return attention_extend(qkv, cache.k[i % ncopy], cache.v[i % ncopy], cache.lens, H, hkv, scale,
                                            cache=cache)

                def decodes(i):
                    return [attention_decode(rows[t], cache.k[i % ncopy], cache.v[i % ncopy], lens_t[t], H, hkv, scale,
                                             cache=cache) for t in range(tn)]

                def sdpa(i):
                    return F.scaled_dot_product_attention(q4, ke[i % ncopy], ve[i % ncopy], attn_mask=mask, scale=scale)

                a = extend(0)
                same = torch.equal(a, torch.cat(decodes(0), 1))  # equal bits when both ran the same (S, C)
                err = (a.float() - sdpa(0).transpose(1, 2).reshape(B, tn, H * DH).float()).abs().max().item()
                cands = {"extend": extend, "decodes": decodes, "sdpa": sdpa}
                graphs = {k: _graphed(fn, iters) for k, fn in cands.items()}
                t = {k: [] for k in cands}
                for _ in range(rounds):
                    for k in cands:
                        t[k].append(_time_ms(lambda i, gr=graphs[k]: gr.replay(), 1) / iters)
                med = {k: statistics.median(v) for k, v in t.items()}
                for k in cands:
                    emit(f"Tn {tn:3d} lens {lens:5d}  {k:<8} {med[k] * 1e3:7.1f} us ({min(t[k]) * 1e3:.1f}-{max(t[k]) * 1e3:.1f})  "
                         f"{med[k] / med['extend']:5.2f}x extend  must move {must / 1e6:6.2f} MB  {must / med[k] / 1e9:5.2f} TB/s")
                emit(f"Tn {tn:3d} lens {lens:5d}  geo (S, C, NB, NT) = {geo}; bits equal to the decodes: {same}; "
                     f"max |extend - sdpa| = {err:.3g}")
                del graphs, ke, ve
        del cache


def bench_generate(rounds, emit, prompt=128, new=128):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    for kvh in (None, 4):
        torch.manual_seed(0)
        model = to_bf16_mixed(get_model("llama_medium", n_kv_head=kvh).cuda()).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()

        @torch.no_grad()
        def gen_eager():
            return model.generate(idx, new)

        # the captured step: built once, replayed by every graph run
        state = {}

        @torch.no_grad()
        def build_graph():
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            tok = torch.zeros(B, dtype=torch.long, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model.decode_step(tok, cache)
            state.update(cache=cache, tok=tok, graph=graph, logits=logits)

        @torch.no_grad()
        def gen_graph():
            cache, tok, graph, logits = state["cache"], state["tok"], state["graph"], state["logits"]
            cache.reset()
            first = model.prefill(idx, cache)
            cache.set_lens(cache.lens, bound=prompt + new)  # the replays advance lens on the device only
            toks = [first.argmax(-1)]
            for _ in range(new - 1):
                tok.copy_(toks[-1])
                graph.replay()
                toks.append(logits.argmax(-1))
            return torch.stack(toks, 1)

        @torch.no_grad()
        def gen_full():
            seq = idx
            for _ in range(new):
                seq = torch.cat([seq, model(seq)[:, -1].argmax(-1)[:, None]], 1)
            return seq[:, prompt:]

        @torch.no_grad()
        def steps_eager(cache, tok, n=32):
            cache.set_lens([prompt] * B)
            for _ in range(n):
                model.decode_step(tok, cache)

        build_graph()
        a, g_, f_ = gen_eager(), gen_graph(), gen_full()
        torch.cuda.synchronize()
        same_g = bool(torch.equal(a, g_))
        agree = float((a == f_).float().mean())  # bf16 paths may part ways after a near-tie; then the rest differs
        cands = {"generate": gen_eager, "graph": gen_graph, "full": gen_full}
        out = {k: [] for k in cands}
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        for _ in range(rounds):
            for k, fn in cands.items():
                s, e = ev(), ev()
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                out[k].append(s.elapsed_time(e))
        # the decode steps alone
        cache, tok = model.new_cache(B, prompt + new), torch.zeros(B, dtype=torch.long, device="cuda")
        model_prefill = torch.no_grad()(lambda: model.prefill(idx, cache))
        model_prefill()
        step_e, step_g = [], []
        for _ in range(rounds):
            s, e = ev(), ev()
            s.record()
            steps_eager(cache, tok)
            e.record()
            torch.cuda.synchronize()
            step_e.append(s.elapsed_time(e) / 32)
            state["cache"].set_lens([prompt] * B)
            s, e = ev(), ev()
            s.record()
            for _ in range(32):
                state["graph"].replay()
            e.record()
            torch.cuda.synchronize()
            step_g.append(s.elapsed_time(e) / 32)
        med = {k: statistics.median(v) for k, v in out.items()}
        name = f"llama_medium kv_heads={kvh or 16}"
        for k in cands:
            emit(f"{name}: {k:<8} {prompt}+{new} tokens x {B}: {med[k]:9.1f} ms ({min(out[k]):.1f}-{max(out[k]):.1f})  "
                 f"{B * new / med[k] * 1e3:8.0f} new tok/s  {med['full'] / med[k]:6.2f}x full")
        me, mg = statistics.median(step_e), statistics.median(step_g)
        emit(f"{name}: decode step at position {prompt}..{prompt + 31}: eager {me:.3f} ms ({min(step_e):.3f}-{max(step_e):.3f}), "
             f"replayed {mg:.3f} ms ({min(step_g):.3f}-{max(step_g):.3f}): eager is {me / mg:.2f}x the replay (launch-bound "
             f"by the difference)")
        emit(f"{name}: graph tokens == eager tokens: {same_g}; eager tokens == full-forward tokens: {agree:.3f} of positions")
        del model, state


GEMM_SHAPES = (("c_attn", 3072, 1024, False), ("attn c_proj", 1024, 1024, False), ("c_fc", 5632, 1024, False),
               ("c_fc + SwiGLU", 5632, 1024, True), ("mlp c_proj", 1024, 2816, False), ("lm_head", 32000, 1024, False))
GEMM_ROWS = (1, 8, 16, 32, 64)


def bench_gemm(rounds, iters, emit):
    """llama_medium's decode-time Linears: the skinny GEMM against F.linear (+ the SwiGLU kernel), each captured
    and replayed, alternating, the weights rotating through >= 512 MiB of distinct copies (a window has at least
    as many calls as there are copies, so no replay finds its weights in the Infinity Cache)."""
    from pytorch_distributed_training_example_amd.ops._native import native
    from pytorch_distributed_training_example_amd.ops.swiglu import swiglu
    C, dev = native(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, fused in GEMM_SHAPES:
        ncopy = -(-ROTATE_BYTES // (N * K * 2))
        calls = max(iters, ncopy)
        w = (torch.randn(ncopy, N, K, device=dev, generator=g) / math.sqrt(K)).bfloat16()
        emit(f"## {name}: N = {N}, K = {K}, {N * K * 2 / 2**20:.1f} MiB of weights x {ncopy} copies, {calls} calls per window")
        for M in GEMM_ROWS:
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            mode = 1 if fused else 0
            geo = tuple(C.gemm_skinny_geo(M, N, K, mode, 0))
            must = N * K * 2 + M * K * 2 + M * (N // 2 if fused else N) * 2

            def ours(i):
                return C.gemm_skinny(x, w[i % ncopy], mode, 0)

            def lib(i):
                y = F.linear(x, w[i % ncopy])
                return swiglu(y) if fused else y

            cands = {"skinny": ours, "library": lib}
            if M == 8:  # the W loads without the non-temporal bit, same kernel otherwise
                def plain(i):
                    C.gemm_skinny_tune(0)
                    y = C.gemm_skinny(x, w[i % ncopy], mode, 0)
                    C.gemm_skinny_tune(1)
                    return y
                cands["skinny, plain W loads"] = plain
            err = (ours(0).float() - lib(0).float()).abs().max().item()
            t = _alternate(cands, rounds, calls)
            med = {k: statistics.median(v[1]) for k, v in t.items()}
            for k, (_, tg) in t.items():
                emit(f"M {M:2d}  {k:<22} (S, FT, NT) = {geo}  replayed {med[k] * 1e3:6.1f} us ({min(tg) * 1e3:.1f}-"
                     f"{max(tg) * 1e3:.1f})  {must / med[k] / 1e9:5.2f} TB/s  {med['library'] / med[k]:5.2f}x library")
            emit(f"M {M:2d}  max |skinny - library| = {err:.3g}")
        del w


def bench_gemm_generate(rounds, emit, prompt=128, new=128):
    """The captured llama_medium decode step and the 128-after-128-token generation on it, PDT_DECODE_GEMM 0
    against 1 (and 1 with plain instead of non-temporal weight loads) in one process, alternating."""
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.ops._native import native
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    configs = {"0": (False, 1), "1": (True, 1), "1, plain W loads": (True, 0)}  # name: (switch, gemm_skinny_tune)
    states = {}

    def select(name):
        SW.decode_gemm = configs[name][0]
        native().gemm_skinny_tune(configs[name][1])

    with torch.no_grad():
        for name in configs:
            select(name)
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            tok = torch.zeros(B, dtype=torch.long, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model.decode_step(tok, cache)
            states[name] = (cache, tok, graph, logits)

        def gen(name):
            select(name)
            cache, tok, graph, logits = states[name]
            cache.reset()
            toks = [model.prefill(idx, cache).argmax(-1)]
            cache.set_lens(cache.lens, bound=prompt + new)
            for _ in range(new - 1):
                tok.copy_(toks[-1])
                graph.replay()
                toks.append(logits.argmax(-1))
            return torch.stack(toks, 1)

        toks = {name: gen(name) for name in configs}
        torch.cuda.synchronize()
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        t_gen, t_step = {n: [] for n in configs}, {n: [] for n in configs}
        for _ in range(rounds):
            for name in configs:
                s, e = ev(), ev()
                s.record()
                gen(name)
                e.record()
                torch.cuda.synchronize()
                t_gen[name].append(s.elapsed_time(e))
                states[name][0].set_lens([prompt] * B)
                s, e = ev(), ev()
                s.record()
                for _ in range(32):
                    states[name][2].replay()
                e.record()
                torch.cuda.synchronize()
                t_step[name].append(s.elapsed_time(e) / 32)
    SW.reload()
    native().gemm_skinny_tune(1)
    for name in configs:
        mg, ms = statistics.median(t_gen[name]), statistics.median(t_step[name])
        emit(f"llama_medium PDT_DECODE_GEMM={name}: {prompt}+{new} tokens x {B} on the captured step {mg:8.1f} ms "
             f"({min(t_gen[name]):.1f}-{max(t_gen[name]):.1f}), {B * new / mg * 1e3:7.0f} new tok/s; replayed step at "
             f"position {prompt}..{prompt + 31}: {ms:.3f} ms ({min(t_step[name]):.3f}-{max(t_step[name]):.3f})")
    emit(f"llama_medium: tokens with the switch on == off: {float((toks['1'] == toks['0']).float().mean()):.3f} of "
         "positions (the two paths round differently; after a near-tie the rest differs)")


def bench_gemm_w8(rounds, iters, emit):
    """As bench_gemm, with the e4m3-weight kernel as a third candidate; every candidate rotates through its own
    >= 512 MiB of distinct weight copies."""
    from pytorch_distributed_training_example_amd.ops._native import native
    from pytorch_distributed_training_example_amd.ops.swiglu import swiglu
    C, dev = native(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, fused in GEMM_SHAPES:
        ncopy, ncopy8 = -(-ROTATE_BYTES // (N * K * 2)), -(-ROTATE_BYTES // (N * K))
        calls = max(iters, ncopy8)
        w = (torch.randn(ncopy, N, K, device=dev, generator=g) / math.sqrt(K)).bfloat16()
        q = [C.quantize_rows_e4m3(w[i % ncopy]) for i in range(ncopy8)]
        wq, sc = torch.stack([a for a, _ in q]), torch.stack([b for _, b in q])
        del q
        emit(f"## {name}: N = {N}, K = {K}: {N * K / 2**20:.1f} MiB e4m3 x {ncopy8} copies, {N * K * 2 / 2**20:.1f} MiB bf16 "
             f"x {ncopy} copies, {calls} calls per window")
        for M in GEMM_ROWS:
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            mode = 1 if fused else 0
            geo8, geo = tuple(C.gemm_skinny_w8_geo(M, N, K, mode, 0)), tuple(C.gemm_skinny_geo(M, N, K, mode, 0))
            io = M * K * 2 + M * (N // 2 if fused else N) * 2
            must = {"w8": N * K + N * 4 + io, "skinny": N * K * 2 + io, "library": N * K * 2 + io}

            def w8(i):
                return C.gemm_skinny_w8(x, wq[i % ncopy8], sc[i % ncopy8], mode, 0)

            def ours(i):
                return C.gemm_skinny(x, w[i % ncopy], mode, 0)

            def lib(i):
                y = F.linear(x, w[i % ncopy])
                return swiglu(y) if fused else y

            cands = {"w8": w8, "skinny": ours, "library": lib}
            err = (w8(0).float() - ours(0).float()).abs().max().item()
            t = _alternate(cands, rounds, calls)
            med = {k: statistics.median(v[1]) for k, v in t.items()}
            for k, (_, tg) in t.items():
                emit(f"M {M:2d}  {k:<8} (S, FT, NT) = {geo8 if k == 'w8' else geo}  replayed {med[k] * 1e3:6.1f} us "
                     f"({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  {must[k] / med[k] / 1e9:5.2f} TB/s  "
                     f"{med['skinny'] / med[k]:5.2f}x skinny")
            emit(f"M {M:2d}  max |w8 - skinny| = {err:.3g} (the quantisation)")
        del w, wq, sc


def bench_gemm_w8_generate(rounds, emit, prompt=128, new=128):
    """The captured llama_medium decode step and the 128-after-128-token generation on it under PDT_DECODE_GEMM=1:
    bf16 weights against quantize_decode_weights(), one process, alternating."""
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    SW.decode_gemm = True
    quantised = model.quantize_decode_weights()._decode_linears
    saved = [m._w8 for m in quantised()]
    model.drop_decode_weights()
    states = {}

    def select(name):
        for m, q in zip(quantised(), saved):
            if name == "e4m3":
                m._w8 = q
            elif hasattr(m, "_w8"):
                del m._w8

    with torch.no_grad():
        for name in ("bf16", "e4m3"):
            select(name)
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            tok = torch.zeros(B, dtype=torch.long, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model.decode_step(tok, cache)
            states[name] = (cache, tok, graph, logits)

        def gen(name):
            select(name)
            cache, tok, graph, logits = states[name]
            cache.reset()
            toks = [model.prefill(idx, cache).argmax(-1)]
            cache.set_lens(cache.lens, bound=prompt + new)
            for _ in range(new - 1):
                tok.copy_(toks[-1])
                graph.replay()
                toks.append(logits.argmax(-1))
            return torch.stack(toks, 1)

        toks = {name: gen(name) for name in states}
        torch.cuda.synchronize()
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        t_gen, t_step = {n: [] for n in states}, {n: [] for n in states}
        for _ in range(rounds):
            for name in states:
                s, e = ev(), ev()
                s.record()
                gen(name)
                e.record()
                torch.cuda.synchronize()
                t_gen[name].append(s.elapsed_time(e))
                states[name][0].set_lens([prompt] * B)
                s, e = ev(), ev()
                s.record()
                for _ in range(32):
                    states[name][2].replay()
                e.record()
                torch.cuda.synchronize()
                t_step[name].append(s.elapsed_time(e) / 32)
    SW.reload()
    for name in states:
        mg, ms = statistics.median(t_gen[name]), statistics.median(t_step[name])
        emit(f"llama_medium PDT_DECODE_GEMM=1, {name} weights: {prompt}+{new} tokens x {B} on the captured step {mg:8.1f} ms "
             f"({min(t_gen[name]):.1f}-{max(t_gen[name]):.1f}), {B * new / mg * 1e3:7.0f} new tok/s; replayed step at "
             f"position {prompt}..{prompt + 31}: {ms:.3f} ms ({min(t_step[name]):.3f}-{max(t_step[name]):.3f})")
    emit(f"llama_medium: tokens with e4m3 weights == bf16 weights: {float((toks['e4m3'] == toks['bf16']).float().mean()):.3f} "
         "of positions (a random-weight model: the quantisation moves near-ties, after which the rest differs)")


def bench_gemm_w4(rounds, iters, emit):
    """As bench_gemm_w8 with the int4-weight kernel against the e4m3-weight one, the reference of every time; each
    rotates through its own >= 512 MiB of distinct weight copies (more copies than the bf16 size would need), and a
    window makes at least as many calls as there are copies. The bytes a candidate must move include its scales."""
    from pytorch_distributed_training_example_amd.ops._native import native
    C, dev = native(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, fused in GEMM_SHAPES:
        ncopy, ncopy8, ncopy4 = (-(-ROTATE_BYTES // (N * K * 2)), -(-ROTATE_BYTES // (N * K)),
                                 -(-ROTATE_BYTES // (N * K // 2)))
        calls = max(iters, ncopy4)
        w = (torch.randn(ncopy, N, K, device=dev, generator=g) / math.sqrt(K)).bfloat16()
        q8 = [C.quantize_rows_e4m3(w[i % ncopy]) for i in range(ncopy8)]
        w8q, s8 = torch.stack([a for a, _ in q8]), torch.stack([b for _, b in q8])
        q4 = [C.quantize_groups_int4(w[i % ncopy]) for i in range(ncopy4)]
        w4q, s4 = torch.stack([a for a, _ in q4]), torch.stack([b for _, b in q4])
        del q8, q4
        emit(f"## {name}: N = {N}, K = {K}: {N * K / 2**21:.2f} MiB int4 + {N * K / 32 / 2**20:.2f} MiB scales x {ncopy4} "
             f"copies, {N * K / 2**20:.1f} MiB e4m3 x {ncopy8} copies, {calls} calls per window")
        for M in GEMM_ROWS:
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            mode = 1 if fused else 0
            geo = {"w4": tuple(C.gemm_skinny_w4_geo(M, N, K, mode, 0)), "w8": tuple(C.gemm_skinny_w8_geo(M, N, K, mode, 0))}
            io = M * K * 2 + M * (N // 2 if fused else N) * 2
            must = {"w4": N * K // 2 + (K // 128) * N * 4 + io, "w8": N * K + N * 4 + io}

            def w4(i):
                return C.gemm_skinny_w4(x, w4q[i % ncopy4], s4[i % ncopy4], mode, 0)

            def w8(i):
                return C.gemm_skinny_w8(x, w8q[i % ncopy8], s8[i % ncopy8], mode, 0)

            err = (w4(0).float() - w8(0).float()).abs().max().item()
            t = _alternate({"w4": w4, "w8": w8}, rounds, calls)
            med = {k: statistics.median(v[1]) for k, v in t.items()}
            for k, (_, tg) in t.items():
                emit(f"M {M:2d}  {k:<3} (S, FT, NT) = {geo[k]}  replayed {med[k] * 1e3:6.1f} us "
                     f"({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  {must[k] / 2**20:6.2f} MiB  {must[k] / med[k] / 1e9:5.2f} TB/s  "
                     f"{med['w8'] / med[k]:5.2f}x w8")
            emit(f"M {M:2d}  max |w4 - w8| = {err:.3g} (the two quantisations)")
        del w, w8q, s8, w4q, s4


def bench_gemm_w4_generate(rounds, emit, prompt=128, new=128):
    """The captured llama_medium decode step and the 128-after-128-token generation on it: quantize_decode_weights()
    (e4m3, the reference) against quantize_decode_weights("int4"), one process, alternating."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    mods = list(model._decode_linears())
    saved = {"e4m3": ("_w8", [m._w8 for m in model.quantize_decode_weights()._decode_linears()]),
             "int4": ("_w4", [m._w4 for m in model.quantize_decode_weights("int4")._decode_linears()])}
    states = {}

    def select(name):
        model.drop_decode_weights()
        for m, q in zip(mods, saved[name][1]):
            setattr(m, saved[name][0], q)

    with torch.no_grad():
        for name in saved:
            select(name)
            cache = model.new_cache(B, prompt + new)
            model.prefill(idx, cache)
            tok = torch.zeros(B, dtype=torch.long, device="cuda")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                logits = model.decode_step(tok, cache)
            states[name] = (cache, tok, graph, logits)

        def gen(name):
            select(name)
            cache, tok, graph, logits = states[name]
            cache.reset()
            toks = [model.prefill(idx, cache).argmax(-1)]
            cache.set_lens(cache.lens, bound=prompt + new)
            for _ in range(new - 1):
                tok.copy_(toks[-1])
                graph.replay()
                toks.append(logits.argmax(-1))
            return torch.stack(toks, 1)

        toks = {name: gen(name) for name in states}
        torch.cuda.synchronize()
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        t_gen, t_step = {n: [] for n in states}, {n: [] for n in states}
        for _ in range(rounds):
            for name in states:
                s, e = ev(), ev()
                s.record()
                gen(name)
                e.record()
                torch.cuda.synchronize()
                t_gen[name].append(s.elapsed_time(e))
                states[name][0].set_lens([prompt] * B)
                s, e = ev(), ev()
                s.record()
                for _ in range(32):
                    states[name][2].replay()
                e.record()
                torch.cuda.synchronize()
                t_step[name].append(s.elapsed_time(e) / 32)
    for name in states:
        mg, ms = statistics.median(t_gen[name]), statistics.median(t_step[name])
        emit(f"llama_medium, {name} weights: {prompt}+{new} tokens x {B} on the captured step {mg:8.1f} ms "
             f"({min(t_gen[name]):.1f}-{max(t_gen[name]):.1f}), {B * new / mg * 1e3:7.0f} new tok/s; replayed step at "
             f"position {prompt}..{prompt + 31}: {ms:.3f} ms ({min(t_step[name]):.3f}-{max(t_step[name]):.3f})")
    emit(f"llama_medium: tokens with int4 weights == e4m3 weights: {float((toks['int4'] == toks['e4m3']).float().mean()):.3f} "
         "of positions (a random-weight model: the quantisation moves near-ties, after which the rest differs)")


W4_TALL_ROWS = (128, 512, 2048)


def bench_gemm_w4_tall(rounds, iters, emit):
    """--gemm-w4-tall: llama_medium's five weight shapes at M in {128, 512, 2048}: the any-row W4A16 GEMM against
    F.linear on the bf16 weight (what these rows run without all_rows) and against dequantise + F.linear
    (linear_skinny_w4's fallback). The --gemm-w4 recipe: captured and replayed (the fallback eagerly), the weights
    rotating through >= 512 MiB of bf16 copies and their int4 forms, taking turns, device events, median of the
    rounds."""
    from pytorch_distributed_training_example_amd.ops._native import native
    from pytorch_distributed_training_example_amd.ops.linear import dequantize_groups_int4
    C, dev = native(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for name, N, K, fused in GEMM_SHAPES:
        if fused:
            continue  # SwiGLU above 64 rows is the SwiGLU kernel on this kernel's output
        ncopy = -(-ROTATE_BYTES // (N * K * 2))
        calls = max(iters, ncopy)
        w = (torch.randn(ncopy, N, K, device=dev, generator=g) / math.sqrt(K)).bfloat16()
        q4 = [C.quantize_groups_int4(w[i]) for i in range(ncopy)]
        w4q, s4 = torch.stack([a for a, _ in q4]), torch.stack([b for _, b in q4])
        del q4
        emit(f"## {name}: N = {N}, K = {K}: {N * K / 2**21:.2f} MiB int4 + {N * K / 32 / 2**20:.2f} MiB scales, "
             f"{N * K / 2**19:.1f} MiB bf16, x {ncopy} copies, {calls} calls per window")
        for M in W4_TALL_ROWS:
            x = torch.randn(M, K, device=dev, generator=g).bfloat16()
            geo = tuple(C.gemm_w4_geo(M, N, K, 0))

            def w4(i):
                return C.gemm_w4(x, w4q[i % ncopy], s4[i % ncopy], 0)

            def lib(i):
                return F.linear(x, w[i % ncopy])

            def deq(i):
                return F.linear(x, dequantize_groups_int4(w4q[i % ncopy], s4[i % ncopy]).to(torch.bfloat16))

            err = (w4(0).float() - deq(0).float()).abs().max().item()
            # (the torch dequantisation uploads an index, so it cannot be captured: that candidate is timed eagerly,
            # ten calls of several kernels each, where the launch cost is small beside them)
            graphs = {"w4": _graphed(w4, calls), "bf16 F.linear": _graphed(lib, calls)}
            t = {"w4": ([], []), "bf16 F.linear": ([], []), "dequantise + F.linear": ([], [])}
            for _ in range(rounds):
                for k in t:
                    if k in graphs:
                        t[k][1].append(_time_ms(lambda i, g=graphs[k]: g.replay(), 1) / calls)
                    else:
                        t[k][1].append(_time_ms(deq, 10))
            med = {k: statistics.median(v[1]) for k, v in t.items()}
            for k, (_, tg) in t.items():
                emit(f"M {M:4d}  {k:<21} {'(S, BM, BN) = ' + str(geo) if k == 'w4' else '':<30} replayed {med[k] * 1e3:8.1f} us "
                     f"({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})  {2 * M * N * K / med[k] / 1e9:7.1f} TFLOP/s  "
                     f"{med['bf16 F.linear'] / med[k]:5.2f}x bf16 F.linear")
            emit(f"M {M:4d}  max |w4 - dequantise + F.linear| = {err:.3g} (one bf16 rounding of the weight)")
        del w, w4q, s4


def bench_gemm_w4_tall_model(rounds, emit, prompt=512):
    """llama_medium, 8 paged slots: a 512-token prefill and the captured decode step on
    quantize_decode_weights("int4") with and without all_rows=True, one process, taking turns."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    mods = list(model._decode_linears())
    model.quantize_decode_weights("int4")
    saved = {"int4": [m._w4 for m in mods], "int4 all_rows": [(*m._w4[:3], True) for m in mods]}
    steps = 32
    pages = -(-(prompt + steps + 4) // 64)
    cache = model.new_paged_cache(B, B * pages, pages)
    tok = torch.zeros(B, dtype=torch.long, device="cuda")

    def select(name):
        for m, q in zip(mods, saved[name]):
            m._w4 = q

    def prefill(name):
        select(name)
        for s in range(B):
            cache.free(s)
            cache.admit(s)
        cache.reserve(prompt + steps + 4)  # the steps' pages too: a replay runs no host code
        return model.prefill(idx, cache)

    with torch.no_grad():
        last, graphs = {}, {}
        for name in saved:
            last[name] = prefill(name)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model.decode_step(tok, cache)
            torch.cuda.current_stream().wait_stream(side)
            cache.set_lens([prompt] * B)
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                model.decode_step(tok, cache)
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        t_pre, t_step = {n: [] for n in saved}, {n: [] for n in saved}
        for _ in range(rounds):
            for name in saved:
                s, e = ev(), ev()
                s.record()
                prefill(name)
                e.record()
                torch.cuda.synchronize()
                t_pre[name].append(s.elapsed_time(e))
                s, e = ev(), ev()
                s.record()
                for _ in range(steps):
                    graphs[name].replay()
                e.record()
                torch.cuda.synchronize()
                t_step[name].append(s.elapsed_time(e) / steps)
    for name in saved:
        mp, ms = statistics.median(t_pre[name]), statistics.median(t_step[name])
        emit(f"llama_medium, {B} paged slots, {name:<13}: {prompt}-token prefill {mp:8.2f} ms ({min(t_pre[name]):.2f}-"
             f"{max(t_pre[name]):.2f}), {B * prompt / mp:6.0f} prompt tok/ms; replayed decode step at position {prompt}.."
             f"{prompt + steps - 1}: {ms:.3f} ms ({min(t_step[name]):.3f}-{max(t_step[name]):.3f})")
    a, b = last["int4 all_rows"].float(), last["int4"].float()
    emit(f"llama_medium: last-position logits, all_rows against the bf16-weight prefill: max |difference| = "
         f"{(a - b).abs().max().item():.3g} of max |logit| = {b.abs().max().item():.3g} (the quantisation of the prompt's "
         f"Linears); argmax equal in {int((a.argmax(-1) == b.argmax(-1)).sum())} of {B}")


SAMPLER_SETTINGS = (("greedy", 0.0, None, None), ("T=0.8", 0.8, None, None), ("T=0.8 k=50", 0.8, 50, None),
                    ("T=0.8 k=50 p=0.9", 0.8, 50, 0.9))


def bench_sampler(rounds, iters, emit, V=32000, ncopy=16):
    """--sampler: ops.sampling.sample (one HIP launch plus the ticket launch) against the aten chain of
    models/llama.py:_sample on bf16 logits [B, 32000] rotating through distinct buffers, taking turns. The fused call
    is timed eager and captured. The chain is timed eager only: its multi-block reductions and topk clear their
    counters with memset nodes, and a replay of a graph that holds them faulted the device when this was first run."""
    from pytorch_distributed_training_example_amd.models.llama import _sample
    from pytorch_distributed_training_example_amd.ops.sampling import SamplerState, sample
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for rows in (1, 8, 64):
        bufs = [(3 * torch.randn(rows, V, device=dev, generator=g)).bfloat16() for _ in range(ncopy)]
        for name, T, k, p in SAMPLER_SETTINGS:
            st, gen = SamplerState(0), torch.Generator(device=dev).manual_seed(0)
            cands = {"fused": lambda i: sample(bufs[i % ncopy], T, k, p, state=st)}
            if p is None:  # the chain has no nucleus filter
                cands["chain"] = lambda i: _sample(bufs[i % ncopy], T, k, gen)
            for fn in cands.values():
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            graphs = {"fused": _graphed(cands["fused"], iters)}
            t = {c: ([], []) for c in cands}
            for _ in range(rounds):
                for c, fn in cands.items():
                    t[c][0].append(_time_ms(fn, iters))
                    if c in graphs:
                        t[c][1].append(_time_ms(lambda i, gr=graphs[c]: gr.replay(), 1) / iters)
            for c, (te, tg) in t.items():
                rep = f"replayed {statistics.median(tg) * 1e3:6.1f} us ({min(tg) * 1e3:.1f}-{max(tg) * 1e3:.1f})" if tg else "replayed n/a"
                emit(f"B {rows:2d}  {name:<17} {c:<5} eager {statistics.median(te) * 1e3:6.1f} us "
                     f"({min(te) * 1e3:.1f}-{max(te) * 1e3:.1f})  {rep}")
            del graphs


def bench_sampler_generate(rounds, emit, prompt=128, new=128):
    """--sampler: llama_medium, 8 sequences, 128 tokens after a 128-token prompt on the captured decode step, the
    token between two replays drawn by the aten chain and by the fused sampler (eager launches), taking turns."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.llama import _sample
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.ops.sampling import SamplerState, sample
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_medium").cuda()).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, prompt), generator=torch.Generator().manual_seed(1)).cuda()
    gen, st = torch.Generator(device="cuda").manual_seed(0), SamplerState(0)
    draws = {"chain  T=0.8 k=50": lambda l: _sample(l, 0.8, 50, gen),
             "fused  T=0.8 k=50": lambda l: sample(l, 0.8, 50, None, state=st),
             "fused  T=0.8 k=50 p=0.9": lambda l: sample(l, 0.8, 50, 0.9, state=st),
             "argmax (greedy, as the other tables)": lambda l: l.argmax(-1)}
    with torch.no_grad():
        cache = model.new_cache(B, prompt + new)
        model.prefill(idx, cache)
        tok = torch.zeros(B, dtype=torch.long, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.decode_step(tok, cache)
        torch.cuda.current_stream().wait_stream(side)
        cache.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = model.decode_step(tok, cache)

        def gen_tokens(draw):
            cache.reset()
            toks = [draw(model.prefill(idx, cache))]
            cache.set_lens(cache.lens, bound=prompt + new)
            for _ in range(new - 1):
                tok.copy_(toks[-1])
                graph.replay()
                toks.append(draw(logits))
            return torch.stack(toks, 1)

        for d in draws.values():
            gen_tokens(d)
        torch.cuda.synchronize()
        out = {k: [] for k in draws}
        for _ in range(rounds):
            for k, d in draws.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                gen_tokens(d)
                e.record()
                torch.cuda.synchronize()
                out[k].append(s.elapsed_time(e))
    for k, v in out.items():
        m = statistics.median(v)
        emit(f"llama_medium: {prompt}+{new} tokens x {B} on the captured step, draw = {k:<37} {m:8.1f} ms "
             f"({min(v):.1f}-{max(v):.1f})  {B * new / m * 1e3:7.0f} new tok/s")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sampler", action="store_true", help="the fused top-k / top-p sampler against the aten chain of "
                    "_sample on [B, 32000] bf16 logits, then the llama_medium generation with either between the replays")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="kernel calls per timed window")
    ap.add_argument("--gen-rounds", type=int, default=3)
    ap.add_argument("--no-generate", action="store_true", help="kernel only")
    ap.add_argument("--no-kernel", action="store_true", help="generation only")
    ap.add_argument("--extend", action="store_true", help="the multi-token append kernel instead")
    ap.add_argument("--gemm", action="store_true", help="the decode-time Linears: skinny GEMM against the library, "
                    "then the generation with PDT_DECODE_GEMM 0 and 1")
    ap.add_argument("--gemm-w8", action="store_true", help="the decode-time Linears on e4m3 weights: the W8A16 skinny "
                    "GEMM against the bf16 one and the library, then the generation with and without "
                    "quantize_decode_weights() under PDT_DECODE_GEMM=1")
    ap.add_argument("--gemm-w4", action="store_true", help="the decode-time Linears on group-wise int4 weights: the W4A16 "
                    "skinny GEMM against the W8A16 one, then the generation on quantize_decode_weights() and on "
                    "quantize_decode_weights(\"int4\")")
    ap.add_argument("--gemm-w4-tall", action="store_true", help="the any-row W4A16 GEMM at M in {128, 512, 2048} against "
                    "F.linear on the bf16 weight and dequantise + F.linear, then llama_medium's 512-token paged prefill "
                    "and captured decode step with and without all_rows=True")
    ap.add_argument("--paged-fp8", action="store_true", help="the e4m3 paged decode kernel against the bf16 paged "
                    "kernel (both captured, rotating caches, taking turns), then the captured llama_medium step on both caches")
    ap.add_argument("--paged", action="store_true", help="the paged decode kernel under a sequential and a shuffled "
                    "block table against the contiguous kernel, then llama_medium's captured step on both caches")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: no GPU (a timing needs the device; nothing is measured on the CPU)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; B={B} H={H} Dh={DH} capacity={CAP} bf16; median of {a.rounds} alternating "
         f"rounds (min-max), {a.iters} calls per window, device events")
    if a.sampler:
        if not a.no_kernel:
            with torch.no_grad():
                bench_sampler(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_sampler_generate(a.gen_rounds, emit)
    elif a.paged and a.extend:
        if not a.no_kernel:
            bench_paged_extend(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_paged_join(a.gen_rounds, emit)
    elif a.paged_fp8:
        with torch.no_grad():
            bench_paged_fp8(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_paged_step(a.gen_rounds, emit, names=("paged", "paged-fp8"))
    elif a.paged:
        if not a.no_kernel:
            bench_paged(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_paged_step(a.gen_rounds, emit)
    elif a.gemm_w4_tall:
        if not a.no_kernel:
            with torch.no_grad():
                bench_gemm_w4_tall(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_gemm_w4_tall_model(a.rounds, emit)
    elif a.gemm_w4:
        if not a.no_kernel:
            bench_gemm_w4(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_gemm_w4_generate(a.gen_rounds, emit)
    elif a.gemm_w8:
        if not a.no_kernel:
            bench_gemm_w8(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_gemm_w8_generate(a.gen_rounds, emit)
    elif a.gemm:
        if not a.no_kernel:
            bench_gemm(a.rounds, a.iters, emit)
        if not a.no_generate:
            bench_gemm_generate(a.gen_rounds, emit)
    elif a.extend:
        bench_extend(a.rounds, a.iters, emit)
    elif not a.no_kernel:
        bench_kernel(a.rounds, a.iters, emit)
    if not a.no_generate and not a.extend and not a.gemm and not a.gemm_w8 and not a.gemm_w4 and not a.gemm_w4_tall \
            and not a.paged \
            and not a.paged_fp8 and not a.sampler:
        bench_generate(a.gen_rounds, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
