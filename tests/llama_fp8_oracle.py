"""The e4m3 envelope shared by tests/test_llama_fp8_cpu.py and tests/test_llama_fp8_gpu.py: what a correct
fp8-emitting RMSNorm / SwiGLU producer may differ by from the float64 oracle of tests/llama_oracle.py. A
helper module imported by plain name.

A producer quantizes v, its bf16-rounded result, as e4m3(clamp(v * scale, +-448)). Dequantized, an
unsaturated element must satisfy

    |q / scale - ref| <= 2^-4 |v| + 2^-10 / scale + E_bf16

2^-4: e4m3's half-ulp relative to the value (3 mantissa bits); 2^-10: half its smallest subnormal (2^-9);
E_bf16 = c * (env + FLOOR): the element's existing bf16 envelope from llama_oracle.py with its existing
constant. v is taken as round_bf16(ref): a kernel's own v lies within E_bf16 of ref, a few bf16 ulps, so it
shares v's e4m3 binade (and with it the half-ulp) unless v * scale is within 2^-7 of a power of two, where
both round to that power of two with an error far inside the first term. The first two terms were checked
against torch's own e4m3 cast at scales 0.5 to 1000: worst error / bound 0.94. An element is unsaturated
when |v| * scale <= 448; up to 448 / (1 - 2^-4) the clamp's error is inside the first term as well, so the
edge of the mask needs no care.
"""
from __future__ import annotations

import torch

from oracle_envelope import FLOOR

E4M3_MAX = 448.0


def e4m3_emulate(v: torch.Tensor, scale: float) -> torch.Tensor:
    """What the producers emit for the bf16 value ``v``: torch's own saturating e4m3 cast."""
    return (v.float() * scale).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def fp8_worst_ratio(q: torch.Tensor, scale: float, ref: torch.Tensor, env: torch.Tensor, c: float):
    """(worst |q / scale - ref| / bound over the unsaturated elements, how many of them exceed the bound,
    how many are unsaturated). ``q``: e4m3 (or its bytes) shaped like ``ref``; ``ref`` / ``env``: float64."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    v = ref.to(torch.bfloat16).double()
    unsat = v.abs() * scale <= E4M3_MAX
    bound = 2.0 ** -4 * v.abs() + 2.0 ** -10 / scale + c * (env.double() + FLOOR)
    err = (q.float().double().cpu() / scale - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(unsat, err / bound, torch.zeros_like(err))
    return ratio.max().item(), int((ratio > 1.0).sum()), int(unsat.sum())
