#!/usr/bin/env python
"""Grouped-query attention: the GQA instantiations of the flash kernels against their multi-head twins and
against SDPA on expanded K/V, and the llama_medium step with 4 K/V heads against 16.

Kernels: B = 8, T = 1024, H = 16 query heads, Hkv in {16, 4, 1}, causal, bf16, on views of the packed
[B, T, (H + 2 Hkv) 64] tensor the model hands them. Forward and backward (delta + dQ + dK/dV) are timed
separately; the candidates take turns within every round in one process, every window timed with device
events, and the median of the rounds (min-max) is reported. ``mha`` is attn_fwd_out / attn_bwd_out at
Hkv = 16; ``gqa16`` is the GQA instantiation at G = 1 (the cost of the variant itself); ``sdpa`` is
F.scaled_dot_product_attention on K/V materialised at 16 heads (the expansion is not timed; its backward
returns gradients of the expanded K/V, the group sum is not timed either). The FLOPs are those of the
multi-head problem in every row: 4 B H T^2 D / 2 forward, 2.5x that backward.

dK/dV of GQA runs H / Hkv times fewer, H / Hkv times longer workgroups: (T / 128) Hkv B of them, 256 at
Hkv = 4 and 64 at Hkv = 1 on 256 CUs.

Whole step: forward + backward + AdamW of llama_medium, bf16 parameters with fp32 masters, 8 x 1024 tokens,
eager, ``n_kv_head`` 16 and 4 alternating in one process.

    python tools/gqa_bench.py [--rounds 7] [--iters 20] [--steps 5] [--no-step] [--out FILE]
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

B, T, H, DH = 8, 1024, 16, 64
KV_HEADS = (16, 4, 1)


def _time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _alternate(cands, rounds, iters):
    """{name: [ms per call, one per round]}: the candidates take turns within every round."""
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(_time_ms(fn, iters))
    return out


def _views(buf, h, hkv):
    x = buf.permute(0, 2, 1, 3)  # [B, heads, T, 64]
    return x[:, :h], x[:, h:h + hkv], x[:, h + hkv:]


def bench_kernels(rounds, iters, emit):
    from pytorch_distributed_training_example_amd.ops._native import native
    C = native()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 / math.sqrt(DH)
    flops = 4 * B * H * T * T * DH * 0.5
    do = torch.randn(B, T, H, DH, device=dev, generator=g).bfloat16().permute(0, 2, 1, 3)
    fwd, bwd = {}, {}
    keep = []  # the tensors the closures use
    for hkv in KV_HEADS:
        qkv = torch.randn(B, T, H + 2 * hkv, DH, device=dev, generator=g).bfloat16()
        dqkv = torch.empty_like(qkv)
        q, k, v = _views(qkv, H, hkv)
        dq, dk, dv = _views(dqkv, H, hkv)
        o = torch.empty(B, T, H, DH, device=dev, dtype=torch.bfloat16).permute(0, 2, 1, 3)
        lse = torch.empty(B, H, T, device=dev, dtype=torch.float32)
        keep.append((qkv, dqkv, o, lse))
        if hkv == H:
            C.attn_fwd_out(q, k, v, o, lse, True, scale)
            fwd["mha"] = lambda q=q, k=k, v=v, o=o, lse=lse: C.attn_fwd_out(q, k, v, o, lse, True, scale)
            bwd["mha"] = lambda q=q, k=k, v=v, o=o, lse=lse, dq=dq, dk=dk, dv=dv: C.attn_bwd_out(
                do, q, k, v, o, lse, dq, dk, dv, True, scale)
            qs, ks, vs = (t.contiguous().requires_grad_() for t in (q, k, v))
            ys = F.scaled_dot_product_attention(qs, ks, vs, is_causal=True, scale=scale)
            fwd["sdpa"] = lambda qs=qs, ks=ks, vs=vs: F.scaled_dot_product_attention(qs, ks, vs, is_causal=True, scale=scale)
            bwd["sdpa"] = lambda qs=qs, ks=ks, vs=vs, ys=ys: torch.autograd.grad(ys, (qs, ks, vs), do, retain_graph=True)
        C.attn_fwd_gqa_out(q, k, v, o, lse, True, scale)
        fwd[f"gqa{hkv}"] = lambda q=q, k=k, v=v, o=o, lse=lse: C.attn_fwd_gqa_out(q, k, v, o, lse, True, scale)
        bwd[f"gqa{hkv}"] = lambda q=q, k=k, v=v, o=o, lse=lse, dq=dq, dk=dk, dv=dv: C.attn_bwd_gqa_out(
            do, q, k, v, o, lse, dq, dk, dv, True, scale)
    tf, tb = _alternate(fwd, rounds, iters), _alternate(bwd, rounds, iters)
    base = {"fwd": statistics.median(tf["mha"]), "bwd": statistics.median(tb["mha"])}
    for name in fwd:
        for kind, times, fl in (("fwd", tf[name], flops), ("bwd", tb[name], 2.5 * flops)):
            m = statistics.median(times)
            emit(f"{name:<6} {kind}  {m * 1e3:8.1f} us ({min(times) * 1e3:.1f}-{max(times) * 1e3:.1f})  "
                 f"{fl / m / 1e9:6.0f} TFLOP/s  {m / base[kind]:5.2f}x mha")
    wg = lambda hkv: (T // 128) * hkv * B  # noqa: E731
    emit("dK/dV workgroups: " + ", ".join(f"Hkv={hkv}: {wg(hkv)}" for hkv in KV_HEADS))


def bench_step(rounds, steps, emit):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.optim import FusedAdamW

    def make(n_kv_head):
        torch.manual_seed(0)
        m = to_bf16_mixed(get_model("llama_medium", n_kv_head=n_kv_head).cuda())
        opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
        g = torch.Generator().manual_seed(1)
        x = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()
        y = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()

        def step():
            opt.zero_grad(set_to_none=True)
            loss = m(x, y)
            loss.backward()
            opt.step()
            return loss
        return step

    cands = {"kv16": make(None), "kv4": make(4)}
    for fn in cands.values():  # warm-up: GEMM algorithm choices, split-K timing, allocator
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(_time_ms(fn, steps))
    m16, m4 = statistics.median(out["kv16"]), statistics.median(out["kv4"])
    tok = B * T
    emit(f"llama_medium step bf16 AdamW {B}x{T} eager: 16 K/V heads {m16:7.2f} ms ({min(out['kv16']):.2f}-"
         f"{max(out['kv16']):.2f}) {tok / m16 * 1e3:8.0f} tok/s | --kv-heads 4 {m4:7.2f} ms ({min(out['kv4']):.2f}-"
         f"{max(out['kv4']):.2f}) {tok / m4 * 1e3:8.0f} tok/s | kv4/kv16 {m4 / m16:5.3f}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed window")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gqa_bench: no GPU (a timing needs the device; nothing is measured on the CPU)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; B={B} T={T} H={H} Dh={DH} causal bf16; median of {a.rounds} alternating "
         f"rounds (min-max), {a.iters} calls / {a.steps} steps per window, device events")
    bench_kernels(a.rounds, a.iters, emit)
    if not a.no_step:
        bench_step(a.rounds, a.steps, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
