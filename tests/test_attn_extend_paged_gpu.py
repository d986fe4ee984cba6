"""The paged multi-token append attention kernel (csrc/kernels/attn_paged_extend.hip) on the binding itself: the
cases of test_attn_extend_gpu.py scattered over the pages of test_attn_paged_gpu.py (B = 3 slots of up to 5 pages
in a pool of 24 whose unused pages, and the rows behind the appended run, hold NaN)."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe
from test_attn_decode_gpu import _native
from test_attn_extend_gpu import B, CAP, DEV, SHAPES, _case, _pack
from test_attn_paged_gpu import MP, NP, _paged

pytestmark = pytest.mark.gpu


def _run(q, k, v, lens, Hkv, splits, seed=0, pad=256):
    """attn_extend_paged on buffers with sentinel tails. Returns (O [B, Tn, H, 64] cpu, LSE [B, Tn, H] cpu, geo)."""
    _, Tn, H, _ = q.shape
    want = tuple(_native().attn_extend_geo(B, Hkv, CAP, Tn, H // Hkv, int(splits or 0)))
    S, rows = want[0], B * Tn * H
    kp, vp, table = _paged(k, v, lens + Tn - 1, seed)
    sizes = {"out": rows * 64, "lse": rows, "o_part": rows * S * 64, "ml_part": rows * S * 2}
    buf = {n: torch.full((sz + pad,), 7.0, device=DEV, dtype=torch.bfloat16 if n == "out" else torch.float32)
           for n, sz in sizes.items()}
    geo = _native().attn_extend_paged(_pack(q, Hkv), kp, vp, table, lens.to(DEV), H, Hkv, 0.125, int(splits or 0),
                                      buf["out"][:rows * 64].view(B, Tn, H * 64), buf["o_part"][:sizes["o_part"]],
                                      buf["ml_part"][:sizes["ml_part"]], buf["lse"][:rows].view(B, Tn, H))
    torch.cuda.synchronize()
    assert tuple(geo) == want
    for n, sz in sizes.items():
        assert bool((buf[n][sz:] == 7.0).all()), f"{n}: sentinel behind the buffer overwritten (geo {want})"
    return buf["out"][:rows * 64].view(B, Tn, H, 64).cpu(), buf["lse"][:rows].view(B, Tn, H).cpu(), want


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("splits", [1, 5, None])
@pytest.mark.parametrize("H,Hkv,Tn", SHAPES)
def test_envelope_at_every_seam(H, Hkv, Tn, splits, amplitude):
    q, k, v, lens, ref, env = _case(H, Hkv, Tn, amplitude)
    O, lse, geo = _run(q, k, v, lens, Hkv, splits)
    assert not torch.isnan(O.float()).any(), f"NaN behind the appended run or from an unused page reached O (geo {geo})"
    name = f"H{H} Hkv{Hkv} Tn{Tn} geo{geo} a{amplitude}"
    worst = oe.assert_within(O, ref["O"], env, oe.ATTN_C, oe.FLOOR, name="O " + name)
    oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE " + name)
    print(f"{name}: worst O ratio {worst:.3f} of {oe.ATTN_C}")


@pytest.mark.parametrize("splits", [1, 5])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (32, 1)])
def test_causal_onehot_probe_bit_for_bit(H, Hkv, splits):
    """test_attn_extend_gpu's probe through pages: q[b, t] = 32 e_t, appended key i = 32 e_i + 64 e_(i-1), older
    keys zero, so O[b, t, h] is V's row lens[b] + t exactly and a mask one key too wide returns row t + 1."""
    Tn = 17
    lens = torch.tensor([0, 56, CAP - Tn], dtype=torch.int32)  # 56 .. 72 crosses the page boundary at 64
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
        want = v[b, :, int(lens[b]):int(lens[b]) + Tn].transpose(0, 1).repeat_interleave(H // Hkv, 1)  # [Tn, H, 64]
        assert torch.equal(O[b].view(torch.int16), want.view(torch.int16)), \
            f"slot {b} (lens {int(lens[b])}), geo {geo}: got keys {(O[b, :, :, 0] + 160).tolist()}"


@pytest.mark.parametrize("splits", [1, 5, None])
def test_the_page_permutation_does_not_change_a_bit(splits):
    q, k, v, lens, _, _ = _case(6, 2, 17, 4.0)
    a, la, _ = _run(q, k, v, lens, 2, splits, seed=0)
    b, lb, _ = _run(q, k, v, lens, 2, splits, seed=1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(la, lb)


@pytest.mark.parametrize("what,match", [("pool rank", "n_pages, kv_heads, 64, 64"), ("table dtype", "int32"),
                                        ("zero tokens", "at least one new token"), ("small scratch", "too small")])
def test_binding_refusals(what, match):
    H, Hkv, Tn = 4, 2, 3
    qkv = torch.zeros(B, Tn, (H + 2 * Hkv) * 64, device=DEV, dtype=torch.bfloat16)
    pool = torch.zeros(NP, Hkv, 64, 64, device=DEV, dtype=torch.bfloat16)
    table = torch.full((B, MP), -1, device=DEV, dtype=torch.int32)
    lens = torch.zeros(B, device=DEV, dtype=torch.int32)
    out = torch.empty(B, Tn, H * 64, device=DEV, dtype=torch.bfloat16)
    _native().attn_extend_paged(qkv, pool, pool, table, lens, H, Hkv, 0.125, 1, out)  # the baseline is accepted
    scratch = ()
    if what == "pool rank":
        pool = pool.view(NP * Hkv, 64, 64)
    if what == "table dtype":
        table = table.long()
    if what == "zero tokens":
        qkv, out = qkv[:, :0], out[:, :0]
    if what == "small scratch":  # one token's worth
        scratch = (torch.empty(B * H * 2 * 64, device=DEV), torch.empty(B * H * 2 * 2, device=DEV))
    with pytest.raises(RuntimeError, match=match):
        _native().attn_extend_paged(qkv, pool, pool, table, lens, H, Hkv, 0.125, 2 if scratch else 1, out, *scratch)
