"""fp64 oracle, envelope, inputs and a CPU emulation for KV-cache decoding (csrc/kernels/attn_decode.hip:
the cache append and the split-KV decode attention), built on oracle_envelope.py, gqa_oracle.py and
llama_oracle.py, which are imported and not changed. A helper module imported by plain name;
tests/test_decode_oracle_cpu.py proves on the CPU that the bound holds for an emulation of the kernel's
rounding points and rejects planted faults.

Decode attention. One query row per (sequence b, head h); K/V head h // G of the cache, G = H / Hkv, keys
0 .. n[b] - 1 with n[b] = lens[b] + 1 (the new token is already appended); whatever the cache holds from
n[b] on is not part of the problem. The oracle is ``oracle_envelope.attention_oracle`` per (b, h), q[b, h]
against K/V[b, h // G, :n[b]], non-causal; the envelope is E_O = P |V| 2^-8.

The constant stays ATTN_C = 3; it is not fitted. A split-KV kernel rounds at the points the flash forward
rounds at, and its splits add fp32 roundings only:
  * P is rounded to bf16 before P V, in each split relative to that split's own maximum m_s. A bf16
    rounding is relative, so p 2^(m - m_s) rounded and scaled back by the fp32 weight 2^(m_s - m) is p
    moved by at most u p (plus 2^-24 for the weight): the operand term u P|V| of the forward, unchanged;
  * the partial (m_s, l_s, O_s) are fp32 and the merge (a maximum, one 2^x, one multiply-add per split, one
    division) is fp32: each costs 2^-24 relative, 2^-16 of the envelope, over at most a few dozen splits;
  * the output is rounded to bf16 once, after the merge: u |O| <= u P|V|.
So 2 u E_O remains the ceiling and the forward's 50 % allowance for what is not modelled (MFMA
accumulation order, the raw 2^x instruction, log2-unit bookkeeping) gives 3. The emulation below, which
rounds where the kernel rounds, reaches about half of it (tests/test_decode_oracle_cpu.py prints the figure).

Cache append. Row (b, t) of the new qkv sits at position p = lens[b] + t and must be rotated as row p of a
full sequence: ``full_sequence`` places the new rows at their positions of a [B, T_full, C] tensor, on which
``gqa_oracle.gqa_rope_oracle`` (float64, ROPE_C) and the existing ``rope_qkv_`` kernel (bit for bit) are the
two references.
"""
from __future__ import annotations

import math

import torch

import oracle_envelope as oe
from gqa_oracle import ROPE_C, gqa_rope_oracle  # noqa: F401  (re-exported to the tests)
from oracle_envelope import ATTN_C, LSE_TOL_PEAKED, LSE_TOL_SMOOTH  # noqa: F401

D = 64
LOG2E = 1.4426950408889634


# ----------------------------------------------------------------------------- inputs
def decode_inputs(B, H, Hkv, cap, lens, amplitude=1.0, seed=0, stale="randn"):
    """q [B, H, 64], k_cache, v_cache [B, Hkv, cap, 64] bf16 and lens (int32 [B]). Keys 0 .. lens[b] are the
    problem; the rows behind them hold ``stale``: "randn" (plausible left-overs), "nan", or "zero"."""
    g = torch.Generator().manual_seed(seed)
    q = (amplitude * torch.randn(B, H, D, generator=g)).to(torch.bfloat16)
    k = (amplitude * torch.randn(B, Hkv, cap, D, generator=g)).to(torch.bfloat16)
    v = torch.randn(B, Hkv, cap, D, generator=g).to(torch.bfloat16)
    lens = torch.as_tensor(lens, dtype=torch.int32)
    assert lens.shape == (B,) and int(lens.min()) >= 0 and int(lens.max()) < cap
    past = torch.arange(cap)[None, :] > lens[:, None]  # [B, cap]
    if stale != "randn":
        fill = float("nan") if stale == "nan" else 0.0
        k = torch.where(past[:, None, :, None], torch.tensor(fill, dtype=torch.bfloat16), k)
        v = torch.where(past[:, None, :, None], torch.tensor(fill, dtype=torch.bfloat16), v)
    return q, k, v, lens


def pack_q(q, Hkv):
    """q [B, H, 64] as the decode step's packed qkv [B, 1, (H + 2 Hkv) 64] (the K/V columns are zeros: the
    kernel reads K and V from the cache)."""
    B, H, _ = q.shape
    qkv = torch.zeros(B, 1, (H + 2 * Hkv) * D, dtype=q.dtype, device=q.device)
    qkv[:, 0, :H * D] = q.reshape(B, H * D)
    return qkv


def onehot_probe(B, H, Hkv, cap, lens, hot):
    """All valid keys -32 on dim 0 except key ``hot[b]`` at +32, queries +32 on dim 0, scale 1/8: the scores are
    -128 and +128, so every probability but the hot key's underflows to exactly 0 in fp32 (2^-369) and O
    must be V's row ``hot[b]`` bit for bit, whatever the split. V is position-coded in integers that bf16
    holds exactly (|x| <= 256): V[b, hk, j, d] = j - 160 on even d (the key, unique for cap <= 416) and
    16 hk + d // 2 - 100 on odd d (the K/V head and the column)."""
    lens = torch.as_tensor(lens, dtype=torch.int32)
    q = torch.zeros(B, H, D)
    q[:, :, 0] = 32.0
    k = torch.zeros(B, Hkv, cap, D)
    k[:, :, :, 0] = -32.0
    for b in range(B):
        assert 0 <= hot[b] <= int(lens[b])
        k[b, :, hot[b], 0] = 32.0
    j = torch.arange(cap, dtype=torch.float32)[None, :, None]
    hk = torch.arange(Hkv, dtype=torch.float32)[:, None, None]
    d = torch.arange(D, dtype=torch.float32)[None, None, :]
    assert cap <= 416 and Hkv <= 8
    v = torch.where(d % 2 == 0, (j - 160.0).expand(Hkv, cap, D), (16.0 * hk + d // 2 - 100.0).expand(Hkv, cap, D))
    v = v[None].expand(B, Hkv, cap, D).contiguous()
    assert torch.equal(v.to(torch.bfloat16).float(), v)
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16), lens


def describe_onehot_mismatch(out, v, lens, hot, H, Hkv, C):
    """None when out [B, H, 64] equals V[b, h // G, hot[b]] bit for bit; else a message naming the first
    wrong (sequence, head), its hot key and the chunk that key is in."""
    G = H // Hkv
    for b in range(out.shape[0]):
        for h in range(H):
            want = v[b, h // G, hot[b]]
            if not torch.equal(out[b, h].view(torch.int16), want.view(torch.int16)):
                dd = int((out[b, h].float() != want.float()).nonzero()[0]) if (out[b, h].float() != want.float()).any() else 0
                return (f"one-hot probe: sequence {b} (lens {int(lens[b])}), head {h} (K/V head {h // G}), hot key "
                        f"{hot[b]} in chunk {hot[b] // C} (C = {C}), 16-key subtile {hot[b] // 16}: "
                        f"O[{dd}] = {float(out[b, h, dd])}, V row has {float(want[dd])}")
    return None


# ----------------------------------------------------------------------------- oracle
def decode_oracle(q, k_cache, v_cache, lens, scale=None):
    """ref O [B, H, 64], LSE [B, H] (float64) and the envelope of O, per (b, h) from ``attention_oracle``."""
    B, H, _ = q.shape
    Hkv = k_cache.shape[1]
    G = H // Hkv
    O = torch.zeros(B, H, D, dtype=torch.float64)
    E = torch.zeros(B, H, D, dtype=torch.float64)
    L = torch.zeros(B, H, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b]) + 1
        for h in range(H):
            ref, env = oe.attention_oracle(q[b, h][None, :].cpu(), k_cache[b, h // G, :n].cpu(),
                                           v_cache[b, h // G, :n].cpu(), causal=False, scale=scale)
            O[b, h], E[b, h], L[b, h] = ref["O"][0], env["O"][0], ref["LSE"][0]
    return {"O": O, "LSE": L}, {"O": E}


# ----------------------------------------------------------------------------- emulation of the kernel's roundings
FAULTS = ("last_key_out", "split_missing", "ignore_m", "head_mod", "stale_row")


def emulate_decode(q, k_cache, v_cache, lens, C, scale=None, fault=None):
    """What the kernel computes, in fp32 with its rounding points: per split of C keys the scores and the
    split's maximum in log2 units, P = 2^(s - m_s) rounded to bf16 for P V (l_s from the unrounded P), fp32
    partials; the fp32 merge; one rounding of O to bf16. Returns (O bf16 [B, H, 64], LSE fp32 [B, H]).
    ``fault`` plants one of FAULTS."""
    assert fault is None or fault in FAULTS
    B, H, _ = q.shape
    Hkv, cap = k_cache.shape[1], k_cache.shape[2]
    G = H // Hkv
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    S = -(-cap // C)
    O = torch.zeros(B, H, D, dtype=torch.bfloat16)
    LSE = torch.zeros(B, H, dtype=torch.float32)
    for b in range(B):
        n = int(lens[b]) + 1
        if fault == "last_key_out":
            n -= 1
        if fault == "stale_row":
            n = min(n + 1, cap)
        for h in range(H):
            hk = h % Hkv if fault == "head_mod" else h // G
            parts = []
            for s in range(S):
                lo, hi = s * C, min(s * C + C, n)
                if hi <= lo:
                    parts.append((torch.tensor(float("-inf")), torch.tensor(0.0), torch.zeros(D)))
                    continue
                sc = (k_cache[b, hk, lo:hi].float() @ q[b, h].float()) * sl2
                m = sc.max()
                p = torch.exp2(sc - m)
                parts.append((m, p.sum(), p.to(torch.bfloat16).float() @ v_cache[b, hk, lo:hi].float()))
            if fault == "split_missing":
                last = max(i for i, pt in enumerate(parts) if pt[0] > float("-inf"))
                parts[last] = (torch.tensor(float("-inf")), torch.tensor(0.0), torch.zeros(D))
            M = torch.stack([pt[0] for pt in parts]).max()
            Lsum, acc = torch.tensor(0.0), torch.zeros(D)
            for m, l, o in parts:
                if m == float("-inf"):
                    continue
                w = torch.tensor(1.0) if fault == "ignore_m" else torch.exp2(m - M)
                Lsum = Lsum + l * w
                acc = acc + o * w
            O[b, h] = (acc / Lsum).to(torch.bfloat16)
            LSE[b, h] = (M + torch.log2(Lsum)) / LOG2E
    return O, LSE


# ----------------------------------------------------------------------------- cache append
def full_sequence(qkv_new, lens, T_full, fill_seed=1):
    """[B, T_full, C]: random rows, with row t of ``qkv_new`` [B, Tn, C] at position lens[b] + t (positions
    past T_full are dropped). What a full-sequence RoPE makes of those positions is the append's reference."""
    B, Tn, C = qkv_new.shape
    g = torch.Generator().manual_seed(fill_seed)
    full = torch.randn(B, T_full, C, generator=g).to(qkv_new.dtype).to(qkv_new.device)
    for b in range(B):
        for t in range(Tn):
            p = int(lens[b]) + t
            if 0 <= p < T_full:
                full[b, p] = qkv_new[b, t]
    return full


def emulate_append(qkv_new, cos, sin, H, Hkv, lens, at_t=False):
    """The append's rotation in fp32 with one rounding (rope.hip's formula) at position lens[b] + t, or, the
    planted fault ``at_t``, at position t. Returns the rotated [B, Tn, C] (V columns unchanged)."""
    B, Tn, C = qkv_new.shape
    x = qkv_new.clone().view(B, Tn, H + 2 * Hkv, D)
    pos = torch.arange(Tn)[None, :] + (0 if at_t else torch.as_tensor(lens).long()[:, None])
    pos = pos.expand(B, Tn)
    c, s = cos[pos][:, :, None, :], sin[pos][:, :, None, :]
    lo, hi = x[:, :, :H + Hkv, :32].float(), x[:, :, :H + Hkv, 32:].float()
    x[:, :, :H + Hkv, :32] = (lo * c - hi * s).to(x.dtype)
    x[:, :, :H + Hkv, 32:] = (hi * c + lo * s).to(x.dtype)
    return x.view(B, Tn, C)
