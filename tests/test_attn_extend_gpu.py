"""The multi-token append attention kernel (csrc/kernels/attn_decode.hip, attn_extend) on the binding itself:
every output element inside decode_oracle.py's envelope at every seam of the column tiling and the chunking,
the bits of the one-token kernel at every token, a causal one-hot probe that must return V rows bit for bit,
NaN behind the appended run, sentinels behind every buffer the kernel writes, and the binding's refusals."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe
from test_attn_decode_gpu import _native

pytestmark = pytest.mark.gpu

CAP, B, DEV = 320, 3, "cuda"
# R = G Tn columns: 2 (NT 1), 20 (NT 2, partial tile), 51 (NT 4, a token's heads straddle a tile), 120 (two
# blocks, the last partial), 160 (three blocks, a token's heads straddle a block)
SHAPES = [(4, 4, 2), (4, 1, 5), (6, 2, 17), (6, 2, 40), (32, 1, 5)]


def _lens(Tn):  # from an empty cache; across key 64 (a 16-key, 64-key and C = 64 chunk seam); up to the capacity
    return torch.tensor([0, 64 - (Tn + 1) // 2, CAP - Tn], dtype=torch.int32)


def _pack(q, Hkv):
    Bq, Tn, H, _ = q.shape
    qkv = torch.zeros(Bq, Tn, (H + 2 * Hkv) * 64, dtype=q.dtype)
    qkv[:, :, :H * 64] = q.reshape(Bq, Tn, H * 64)
    return qkv.to(DEV)


def _run(q, k, v, lens, Hkv, splits, scale=0.125, pad=256):
    """attn_extend on buffers with sentinel tails. Returns (O [B, Tn, H, 64] cpu, LSE [B, Tn, H] cpu, geo)."""
    _, Tn, H, _ = q.shape
    S, C, NB, NT = _native().attn_extend_geo(B, Hkv, CAP, Tn, H // Hkv, int(splits or 0))
    rows = B * Tn * H
    sizes = {"out": rows * 64, "lse": rows, "o_part": rows * S * 64, "ml_part": rows * S * 2}
    buf = {n: torch.full((sz + pad,), 7.0, device=DEV, dtype=torch.bfloat16 if n == "out" else torch.float32)
           for n, sz in sizes.items()}
    geo = _native().attn_extend(_pack(q, Hkv), k.to(DEV), v.to(DEV), lens.to(DEV), H, Hkv, scale, int(splits or 0),
                                buf["out"][:rows * 64].view(B, Tn, H * 64), buf["o_part"][:sizes["o_part"]],
                                buf["ml_part"][:sizes["ml_part"]], buf["lse"][:rows].view(B, Tn, H))
    torch.cuda.synchronize()
    assert tuple(geo) == (S, C, NB, NT)
    for n, sz in sizes.items():
        assert bool((buf[n][sz:] == 7.0).all()), f"{n}: sentinel behind the buffer overwritten (geo {tuple(geo)})"
    return buf["out"][:rows * 64].view(B, Tn, H, 64).cpu(), buf["lse"][:rows].view(B, Tn, H).cpu(), tuple(geo)


_CASES = {}


def _case(H, Hkv, Tn, amplitude):
    """Inputs (NaN behind the appended run) and the fp64 reference of every token, once per case."""
    key = (H, Hkv, Tn, amplitude)
    if key not in _CASES:
        lens = _lens(Tn)
        _, k, v, _ = do.decode_inputs(B, H, Hkv, CAP, lens + Tn - 1, amplitude, seed=31 * H + Hkv + Tn, stale="nan")
        g = torch.Generator().manual_seed(7 * H + Tn)
        q = (amplitude * torch.randn(B, Tn, H, 64, generator=g)).to(torch.bfloat16)
        refs = [do.decode_oracle(q[:, t], k, v, lens + t) for t in range(Tn)]
        ref = {n: torch.stack([r[0][n] for r in refs], 1) for n in ("O", "LSE")}
        _CASES[key] = (q, k, v, lens, ref, torch.stack([r[1]["O"] for r in refs], 1))
    return _CASES[key]


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("splits", [1, 5, None])
@pytest.mark.parametrize("H,Hkv,Tn", SHAPES)
def test_envelope_at_every_seam(H, Hkv, Tn, splits, amplitude):
    q, k, v, lens, ref, env = _case(H, Hkv, Tn, amplitude)
    O, lse, geo = _run(q, k, v, lens, Hkv, splits)
    NT = {2: 1, 20: 2}.get(H // Hkv * Tn, 4)
    assert geo[2:] == (-(-H // Hkv * Tn // (16 * NT)), NT) and (not splits or geo[:2] == {1: (1, 320), 5: (5, 64)}[splits])
    assert not torch.isnan(O.float()).any(), f"NaN behind the appended run reached O (geo {geo})"
    name = f"H{H} Hkv{Hkv} Tn{Tn} geo{geo} a{amplitude}"
    worst = oe.assert_within(O, ref["O"], env, oe.ATTN_C, oe.FLOOR, name="O " + name)
    oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE " + name)
    print(f"{name}: worst O ratio {worst:.3f} of {oe.ATTN_C}")


def test_one_token_geometry_is_the_append_rule_at_one_token():
    """Up to 64 heads per group (one column block) the two rules give one (S, C): what lets a cache's scratch
    and a captured grid serve either kernel."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_geo, attention_extend_geo
    for Hkv in (1, 8):
        for G in (1, 4, 16, 17, 32, 64):
            for cap in (40, 320, 1024, 4096):
                for s in (None, 1, 5):
                    one, ext = attention_decode_geo(B, Hkv, cap, s, G), attention_extend_geo(B, Hkv, cap, 1, s, G)
                    assert one == ext[:2] and ext[2] == 1, f"Hkv {Hkv} G {G} capacity {cap} splits {s}: {one}, {ext}"


@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("H,Hkv,Tn", [(6, 2, 17), (32, 1, 5)])
def test_bits_of_the_one_token_kernel_at_every_token(H, Hkv, Tn, splits):
    q, k, v, lens, _, _ = _case(H, Hkv, Tn, 4.0)
    O, lse, geo = _run(q, k, v, lens, Hkv, splits)
    O2, lse2, _ = _run(q, k, v, lens, Hkv, splits)
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16)) and torch.equal(lse, lse2), "two runs differ"
    n, kd, vd = _native(), k.to(DEV), v.to(DEV)
    S = geo[0]
    for t in range(Tn):
        out = torch.empty(B, 1, H * 64, device=DEV, dtype=torch.bfloat16)
        l1 = torch.empty(B, H, device=DEV)
        part = torch.empty(B * H * S * 66, device=DEV)
        g1 = n.attn_decode(_pack(q[:, t:t + 1], Hkv), kd, vd, (lens + t).to(DEV), H, Hkv, 0.125, splits, out,
                           part[:B * H * S * 64], part[B * H * S * 64:], l1)
        assert tuple(g1) == geo[:2]
        assert torch.equal(out.view(B, H, 64).cpu().view(torch.int16), O[:, t].view(torch.int16)), f"O, token {t}"
        assert torch.equal(l1.cpu(), lse[:, t]), f"LSE, token {t}"


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (32, 1)])
def test_causal_onehot_probe_bit_for_bit(H, Hkv, splits):
    """q[b, t] = 32 e_t, appended key i = 32 e_i + 64 e_(i-1), older keys zero, scale 1/8: query t scores 128 on
    its own key, 256 on key t + 1 (which must be masked) and 0 elsewhere (weight 2^-184, 0 in fp32 next to 1),
    so O[b, t, h] is V's row lens[b] + t exactly; a mask one key too wide returns row t + 1."""
    Tn = 17
    lens = torch.tensor([0, 56, CAP - Tn], dtype=torch.int32)  # 56 .. 72 crosses the chunk seam at 64
    _, _, v, _ = do.onehot_probe(B, H, Hkv, CAP, lens + Tn - 1, (lens + Tn - 1).tolist())
    q = torch.zeros(B, Tn, H, 64)
    k = torch.zeros(B, Hkv, CAP, 64)
    for t in range(Tn):
        q[:, t, :, t] = 32.0
        for b in range(B):
            k[b, :, int(lens[b]) + t, t] = 32.0
            if t > 0:
                k[b, :, int(lens[b]) + t, t - 1] = 64.0
    O, _, geo = _run(q.to(torch.bfloat16), k.to(torch.bfloat16), v, lens, Hkv, splits)
    for b in range(B):
        for t in range(Tn):
            want = v[b, :, int(lens[b]) + t].repeat_interleave(H // Hkv, 0)  # [H, 64]
            assert torch.equal(O[b, t].view(torch.int16), want.view(torch.int16)), \
                f"sequence {b} (lens {int(lens[b])}), token {t}, geo {geo}: got key {O[b, t, :, 0] + 160}"


def test_binding_refusals():
    n, H, Hkv, Tn = _native(), 4, 2, 3
    qkv = torch.zeros(B, Tn, (H + 2 * Hkv) * 64, device=DEV, dtype=torch.bfloat16)
    k = torch.zeros(B, Hkv, CAP, 64, device=DEV, dtype=torch.bfloat16)
    lens = torch.zeros(B, device=DEV, dtype=torch.int32)
    out = torch.empty(B, Tn, H * 64, device=DEV, dtype=torch.bfloat16)
    n.attn_extend(qkv, k, k, lens, H, Hkv, 0.125, 1, out)  # the baseline is accepted
    one = (torch.empty(B * H * 2 * 64, device=DEV), torch.empty(B * H * 2 * 2, device=DEV))  # one token's worth
    with pytest.raises(RuntimeError, match="too small"):
        n.attn_extend(qkv, k, k, lens, H, Hkv, 0.125, 2, out, *one)
    with pytest.raises(RuntimeError, match="at least one new token"):
        n.attn_extend(qkv[:, :0], k, k, lens, H, Hkv, 0.125, 1, out[:, :0])
