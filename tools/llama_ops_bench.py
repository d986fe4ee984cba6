#!/usr/bin/env python
"""RMSNorm / RoPE / SwiGLU kernels and the llama_medium step: our HIP path against the aten composition
that PDT_DISABLE_NATIVE=1 runs.

Kernel microbenchmarks at llama_medium's shapes (8 x 1024 tokens: N = 8192, D = 1024, F = 2816, H = 16,
bf16): forward and backward of each op, ours and aten alternating round by round in one process, every
window timed with device events. GB/s is the bytes the operation must move (each operand read once, each
result written once; the weight, rstd and table are left out) over the measured time.

Whole step: forward + backward + AdamW of llama_medium, bf16 parameters, batch 8 x 1024, native against
PDT_DISABLE_NATIVE=1, again alternating in one process.

``--fp8``: instead, the two fp8-emitting producers (rms_fwd_fp8, fp8_swiglu_cast forward and backward)
against their unfused chains (the bf16 kernel, then fp8_cast_transpose) at the same shapes, and the
llama_medium step in three configurations alternating in one process: bf16, fp8 with PDT_FP8_LN and
PDT_FP8_SWIGLU on, fp8 with both off (the per-Linear fp8 path).

    python tools/llama_ops_bench.py [--fp8] [--rounds 5] [--iters 20] [--steps 5] [--no-step] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, D, F, H, B, T = 8192, 1024, 2816, 16, 8, 1024
ELT = 2  # bf16


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
    for fn in cands.values():  # warm-up: code objects loaded, allocator pools filled
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(_time_ms(fn, iters))
    return out


def _line(label, nbytes, times):
    ours, aten = times["ours"], times["aten"]
    mo, ma = statistics.median(ours), statistics.median(aten)
    return (f"{label:<28} ours {mo * 1e3:8.1f} us ({min(ours) * 1e3:.1f}-{max(ours) * 1e3:.1f})  "
            f"{nbytes / mo / 1e6:7.0f} GB/s | aten {ma * 1e3:8.1f} us ({min(aten) * 1e3:.1f}-{max(aten) * 1e3:.1f})  "
            f"{nbytes / ma / 1e6:7.0f} GB/s | aten/ours {ma / mo:5.2f}x")


def bench_kernels(rounds, iters, emit):
    from pytorch_distributed_training_example_amd.ops import rmsnorm, rope, swiglu
    from pytorch_distributed_training_example_amd.ops._native import native
    nat = native()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g).bfloat16()  # noqa: E731

    # ---- RMSNorm with the residual add (what every residual step of the model runs)
    x, h, dy, ds = r(N, D), r(N, D), r(N, D), r(N, D)
    w = (torch.rand(D, device=dev, generator=g) + 0.5)
    _, rstd, s = nat.rms_fwd(x, w, 1e-5, h)

    def aten_add_rms(xx, hh):
        ss = xx + hh
        return ss, rmsnorm.rms_norm_reference(ss, w, 1e-5)

    xa, ha = x.clone().requires_grad_(), h.clone().requires_grad_()
    wa = w.clone().requires_grad_()

    def aten_add_rms_graph():
        ss = xa + ha
        return ss, rmsnorm.rms_norm_reference(ss, wa, 1e-5)

    sa, ya = aten_add_rms_graph()
    emit(_line("rmsnorm+add fwd", 4 * N * D * ELT, _alternate(
        {"ours": lambda: nat.rms_fwd(x, w, 1e-5, h), "aten": lambda: aten_add_rms(x, h)}, rounds, iters)))
    emit(_line("rmsnorm+add bwd (+ds)", 4 * N * D * ELT, _alternate(
        {"ours": lambda: nat.rms_bwd(dy, s, w, rstd, ds),
         "aten": lambda: torch.autograd.grad([sa, ya], [xa, wa], [ds, dy], retain_graph=True)}, rounds, iters)))
    del sa, ya

    # ---- RoPE in place on the packed qkv (the backward is the same kernel, conj)
    cos, sin = [t.to(dev) for t in rope.rope_table(T)]
    qkv = r(B, T, 3 * H * 64)
    qkv2 = qkv.clone()
    rope_bytes = 2 * N * 2 * H * 64 * ELT
    emit(_line("rope fwd (in place)", rope_bytes, _alternate(
        {"ours": lambda: nat.rope_qkv(qkv, cos, sin, H, False),
         "aten": lambda: rope._rotate_reference_(qkv2, cos, sin, H, H, False)}, rounds, iters)))
    emit(_line("rope bwd (in place, conj)", rope_bytes, _alternate(
        {"ours": lambda: nat.rope_qkv(qkv, cos, sin, H, True),
         "aten": lambda: rope._rotate_reference_(qkv2, cos, sin, H, H, True)}, rounds, iters)))
    del qkv, qkv2

    # ---- SwiGLU on the packed gate/up
    gu, dyf = r(N, 2 * F), r(N, F)
    ga = gu.clone().requires_grad_()
    ya = swiglu.swiglu_reference(ga)
    emit(_line("swiglu fwd", 3 * N * F * ELT, _alternate(
        {"ours": lambda: nat.swiglu_fwd(gu), "aten": lambda: swiglu.swiglu_reference(gu)}, rounds, iters)))
    emit(_line("swiglu bwd", 5 * N * F * ELT, _alternate(
        {"ours": lambda: nat.swiglu_bwd(dyf, gu),
         "aten": lambda: torch.autograd.grad(ya, ga, dyf, retain_graph=True)}, rounds, iters)))


def _line2(label, nbytes_fused, nbytes_chain, times):
    fu, ch = times["fused"], times["chain"]
    mf, mc = statistics.median(fu), statistics.median(ch)
    return (f"{label:<28} fused {mf * 1e3:8.1f} us ({min(fu) * 1e3:.1f}-{max(fu) * 1e3:.1f})  "
            f"{nbytes_fused / mf / 1e6:7.0f} GB/s | chain {mc * 1e3:8.1f} us ({min(ch) * 1e3:.1f}-{max(ch) * 1e3:.1f})  "
            f"{nbytes_chain / mc / 1e6:7.0f} GB/s | chain/fused {mc / mf:5.2f}x")


def bench_fp8_producers(rounds, iters, emit):
    """The fp8-emitting producers against bf16 kernel + fp8_cast_transpose. Bytes: bf16 operands read once,
    the two e4m3 copies written once (1 B each); the chain also writes and re-reads the bf16 result."""
    from pytorch_distributed_training_example_amd.ops._native import native
    nat = native()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g).bfloat16()  # noqa: E731
    row = torch.zeros(3 + 4, device=dev)
    row[1], row[2] = 16.0, 1 / 16.0
    x, h = r(N, D), r(N, D)
    w = (torch.rand(D, device=dev, generator=g) + 0.5)

    def rms_chain():
        y, _, _ = nat.rms_fwd(x, w, 1e-5, h)
        return nat.fp8_cast_transpose(y, row, True)
    nd = N * D
    emit(_line2("rmsnorm+add -> e4m3", nd * (3 * ELT + 2), nd * (3 * ELT + 2 * ELT + 2), _alternate(
        {"fused": lambda: nat.rms_fwd_fp8(x, w, 1e-5, h, row), "chain": rms_chain}, rounds, iters)))
    gu, dyf = r(N, 2 * F), r(N, F)

    def fwd_chain():
        return nat.fp8_cast_transpose(nat.swiglu_fwd(gu), row, True)

    def bwd_chain():
        return nat.fp8_cast_transpose(nat.swiglu_bwd(dyf, gu), row, True)
    nf = N * F
    emit(_line2("swiglu fwd -> e4m3", nf * (2 * ELT + 2), nf * (2 * ELT + 2 * ELT + 2), _alternate(
        {"fused": lambda: nat.fp8_swiglu_cast(gu, None, row), "chain": fwd_chain}, rounds, iters)))
    emit(_line2("swiglu bwd -> e4m3", nf * (3 * ELT + 4), nf * (3 * ELT + 4 * ELT + 4), _alternate(
        {"fused": lambda: nat.fp8_swiglu_cast(gu, dyf, row), "chain": bwd_chain}, rounds, iters)))


def bench_fp8_step(rounds, steps, emit):
    """llama_medium, 8 x 1024 tokens, AdamW, eager: bf16 | fp8 fused producers | fp8 per-Linear casts."""
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    from pytorch_distributed_training_example_amd.optim import FusedAdamW

    def make(precision, fused):
        torch.manual_seed(0)
        m = apply_precision(get_model("llama_medium").cuda(), precision)
        opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
        g = torch.Generator().manual_seed(1)
        x = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()
        y = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()

        def step():
            SW.fp8_ln = SW.fp8_swiglu = fused
            opt.zero_grad(set_to_none=True)
            loss = m(x, y)
            loss.backward()
            opt.step()
            return loss
        return step

    saved = (SW.fp8_ln, SW.fp8_swiglu)
    cands = {"bf16": make("bf16", True), "fp8 fused": make("fp8", True), "fp8 per-Linear": make("fp8", False)}
    try:
        for fn in cands.values():  # warm-up: GEMM algorithm choices, the delayed scales, allocator
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        out = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                out[k].append(_time_ms(fn, steps))
    finally:
        SW.fp8_ln, SW.fp8_swiglu = saved
    med = {k: statistics.median(v) for k, v in out.items()}
    tok = B * T
    for k, v in out.items():
        emit(f"llama_medium step AdamW {B}x{T} {k:<15} {med[k]:7.1f} ms ({min(v):.1f}-{max(v):.1f}) "
             f"{tok / med[k] * 1e3:8.0f} tok/s | bf16 / this {med['bf16'] / med[k]:5.2f}x")


def bench_step(rounds, steps, emit):
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.optim import FusedAdamW

    def make(native_on):
        torch.manual_seed(0)
        m = to_bf16_mixed(get_model("llama_medium").cuda())
        opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
        g = torch.Generator().manual_seed(1)
        x = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()
        y = torch.randint(0, m.cfg.vocab_size, (B, T), generator=g).cuda()

        def step():
            if native_on:
                os.environ.pop("PDT_DISABLE_NATIVE", None)
            else:
                os.environ["PDT_DISABLE_NATIVE"] = "1"
            SW.reload()
            opt.zero_grad(set_to_none=True)
            loss = m(x, y)
            loss.backward()
            opt.step()
            return loss
        return step

    cands = {"ours": make(True), "aten": make(False)}
    try:
        for fn in cands.values():  # warm-up: GEMM algorithm choices, split-K timing, allocator
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        out = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                out[k].append(_time_ms(fn, steps))
    finally:
        os.environ.pop("PDT_DISABLE_NATIVE", None)
        SW.reload()
    mo, ma = statistics.median(out["ours"]), statistics.median(out["aten"])
    tok = B * T
    emit(f"llama_medium step bf16 AdamW {B}x{T}: ours {mo:7.1f} ms ({min(out['ours']):.1f}-{max(out['ours']):.1f}) "
         f"{tok / mo * 1e3:8.0f} tok/s | PDT_DISABLE_NATIVE=1 {ma:7.1f} ms ({min(out['aten']):.1f}-{max(out['aten']):.1f}) "
         f"{tok / ma * 1e3:8.0f} tok/s | {ma / mo:5.2f}x")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed window")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--fp8", action="store_true", help="the fp8 producers against their unfused chains, and the "
                    "step in bf16 / fp8 fused / fp8 per-Linear")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("llama_ops_bench: no GPU (a timing needs the device; nothing is measured on the CPU)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; N={N} D={D} F={F} H={H} bf16; median of {a.rounds} alternating rounds "
         f"(min-max), {a.iters} calls / {a.steps} steps per window, device events")
    if a.fp8:
        bench_fp8_producers(a.rounds, a.iters, emit)
        if not a.no_step:
            bench_fp8_step(a.rounds, a.steps, emit)
    else:
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
