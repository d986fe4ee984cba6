"""fp64 oracle and envelopes for grouped-query attention and its RoPE launch (the GQA instantiations of
attention.hip, rope.hip's H + Hkv form), built on oracle_envelope.py and llama_oracle.py, which are
imported and not changed. A helper module imported by plain name; tests/test_gqa_oracle_cpu.py proves on
the CPU that the bounds hold for an emulation of the kernels' roundings and reject planted bugs.

Attention. H query heads, Hkv K/V heads, G = H / Hkv; query head h reads K/V head h // G (HF's
``repeat_kv``: consecutive query heads share a K/V head). The oracle expands K and V to H heads with
``repeat_interleave(G)``, calls ``attention_oracle`` (multi-head, float64) and sums dK, dV and their
envelopes over the G heads of each group. O, LSE and dQ are the multi-head ones unchanged.

The constant stays ATTN_C = 3; it is not fitted. With E_g the multi-head envelope term of head g of a
group (E_dK or E_dV of oracle_envelope.py, without the factor u):
  * operand rounding: each head's P (for dV) or dS (for dK) is rounded to bf16 before its MFMA, which
    moves that head's contribution by at most u E_g, and the group's sum by at most u sum_g E_g;
  * output rounding: the kernel accumulates all G heads and all their query tiles in fp32 registers of
    one workgroup and rounds to bf16 once, u |sum_g dK_g| <= u sum_g |dK_g| <= u sum_g E_g;
  * fp32 accumulation over G times more terms is still about 2^-16 of that (u_fp32 / u_bf16 per add).
So 2 u sum_g E_g remains the ceiling, exactly the multi-head statement with E replaced by the group sum,
and the same 50 % allowance for what the bound does not model gives 3.

RoPE. ``rope_oracle``'s formula on the H + Hkv rotated heads of the packed [B, T, (H + 2 Hkv) 64] tensor:
    2 u (|x[j] cos| + |x[j+32] sin|) + u_out |x'|,     ROPE_C = 2,
with the Hkv value heads behind them unchanged (envelope 0: bit for bit). The round trip bound is
``rope_roundtrip_envelope``'s, (u_out (1 + u_out) + 4 u) (|x'[j] cos| + |x'[j+32] sin|) + u_out |x|, c = 1.
"""
from __future__ import annotations

import torch

import oracle_envelope as oe
from llama_oracle import ROPE_C  # noqa: F401  (re-exported to the tests)
from oracle_envelope import ATTN_C, FLOOR, U_FP32, u_of  # noqa: F401


def expand_kv(x, G):
    """[B, Hkv, T, D] -> [B, Hkv * G, T, D]: head h of the result is head h // G of x."""
    return x.repeat_interleave(G, dim=1)


def group_sum(x, G):
    """[B, H, T, D] -> [B, H / G, T, D]: the sum over each group of G consecutive heads."""
    B, H, T, D = x.shape
    return x.reshape(B, H // G, G, T, D).sum(2)


def gqa_attention_oracle(q, k, v, do=None, causal=False, scale=None):
    """q, do [B, H, T, Dh]; k, v [B, Hkv, T, Dh]. Returns (ref, env) as ``attention_oracle`` does, with dK and
    dV (and their envelopes) [B, Hkv, T, Dh]: the sums over each group's query heads."""
    H, Hkv = q.shape[1], k.shape[1]
    assert H % Hkv == 0, (H, Hkv)
    G = H // Hkv
    ref, env = oe.attention_oracle(q, expand_kv(k, G), expand_kv(v, G), do, causal=causal, scale=scale)
    if do is not None:
        for name in ("dK", "dV"):
            ref[name], env[name] = group_sum(ref[name], G), group_sum(env[name], G)
    return ref, env


def split_packed(qkv, H, Hkv):
    """Packed [B, T, (H + 2 Hkv) 64] -> (q [B, H, T, 64], k [B, Hkv, T, 64], v [B, Hkv, T, 64]) views."""
    B, T, C = qkv.shape
    x = qkv.view(B, T, H + 2 * Hkv, 64).permute(0, 2, 1, 3)
    return x[:, :H], x[:, H:H + Hkv], x[:, H + Hkv:]


# ----------------------------------------------------------------------------- RoPE
def _rot_terms(X, cos, sin, T, conj):
    c = cos[:T].double().view(1, T, 1, 32)
    s = sin[:T].double().view(1, T, 1, 32) * (-1.0 if conj else 1.0)
    return X[..., :32], X[..., 32:], c, s


def gqa_rope_oracle(qkv, cos, sin, H, Hkv, conj=False):
    """qkv [B, T, (H + 2 Hkv) 64] bf16, cos / sin fp32 [T_max, 32]. Returns (ref, env), float64, of qkv's shape;
    the V heads of ref are qkv's and their envelope is 0."""
    B, T, C = qkv.shape
    R = H + Hkv
    X = qkv.double().view(B, T, H + 2 * Hkv, 64)
    lo_, hi, c, s = _rot_terms(X[:, :, :R], cos, sin, T, conj)
    ref, env = X.clone(), torch.zeros_like(X)
    ref[:, :, :R, :32] = lo_ * c - hi * s
    ref[:, :, :R, 32:] = hi * c + lo_ * s
    env[:, :, :R, :32] = 2 * U_FP32 * ((lo_ * c).abs() + (hi * s).abs())
    env[:, :, :R, 32:] = 2 * U_FP32 * ((hi * c).abs() + (lo_ * s).abs())
    env[:, :, :R] += u_of(qkv.dtype) * ref[:, :, :R].abs()
    return ref.view(B, T, C), env.view(B, T, C)


def gqa_rope_roundtrip_envelope(qkv, cos, sin, H, Hkv):
    """``rope_roundtrip_envelope`` on the H + Hkv rotated heads; 0 on the V heads."""
    B, T, C = qkv.shape
    R = H + Hkv
    u_out = u_of(qkv.dtype)
    rot, _ = gqa_rope_oracle(qkv, cos, sin, H, Hkv)
    Rt = rot.view(B, T, H + 2 * Hkv, 64)
    lo_, hi, c, s = _rot_terms(Rt[:, :, :R].abs(), cos, sin, T, False)
    c, s = c.abs(), s.abs()
    env = torch.zeros_like(Rt)
    k = u_out * (1 + u_out) + 4 * U_FP32
    env[:, :, :R, :32] = k * (lo_ * c + hi * s)
    env[:, :, :R, 32:] = k * (hi * c + lo_ * s)
    X = qkv.double().view(B, T, H + 2 * Hkv, 64).clone()
    X[:, :, R:] = 0
    return (env + u_out * X.abs()).view(B, T, C)


def gqa_rope_inputs(B, T, H, Hkv, seed=None):
    g = torch.Generator().manual_seed(100000 * B + 1000 * H + 100 * Hkv + T if seed is None else seed)
    return torch.randn(B, T, (H + 2 * Hkv) * 64, generator=g).to(torch.bfloat16)
