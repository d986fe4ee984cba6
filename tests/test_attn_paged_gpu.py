"""The paged decode attention and append kernels (csrc/kernels/attn_paged.hip) against decode_oracle.py and
the contiguous append: B = 3 slots of up to 5 pages (320 positions) in a pool of 24 pages whose unused pages
hold NaN, the logical cache of decode_oracle scattered over a seeded page permutation."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe

pytestmark = pytest.mark.gpu

B, MP, NP, CAP = 3, 5, 24, 320
SHAPES = [(4, 2), (6, 2), (32, 1)]  # (32, 1): two passes of 16 query heads
LENS = [(0, 14, 15), (16, 62, 63), (64, 126, 127), (128, 191, 192), (129, 255, 256), (65, 318, 319)]  # test_attn_decode_gpu's
SPLITS = [1, 5, None]  # 5: chunks of one page each; None: the default rule
DEV = "cuda"


def _native():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _paged(k, v, lens, seed=0, fill=float("nan")):
    """(k_pool, v_pool, table) on the GPU: the contiguous [B, Hkv, 320, 64] caches scattered into pages under
    permutation ``seed``; table entries past a sequence's last page are -1, every other pool page holds ``fill``."""
    perm = torch.randperm(NP, generator=torch.Generator().manual_seed(seed))
    table = perm[:B * MP].view(B, MP).clone()
    table[torch.arange(MP)[None, :] > (lens.long()[:, None] >> 6)] = -1
    ok = table >= 0
    pools = []
    for c in (k, v):
        pool = torch.full((NP, c.shape[1], 64, 64), fill, dtype=c.dtype)
        pool[table[ok]] = c.view(B, c.shape[1], MP, 64, 64).permute(0, 2, 1, 3, 4)[ok]
        pools.append(pool.to(DEV))
    return pools[0], pools[1], table.to(torch.int32).to(DEV)


def _run(q, k, v, lens, H, Hkv, splits, seed=0, pad=256):
    """The binding on buffers with sentinel tails behind the output, the LSE and both scratch tensors.
    Returns (O [B, H, 64] cpu, LSE cpu, (S, C))."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_geo
    S, C = attention_decode_geo(B, Hkv, CAP, splits, H // Hkv)
    kp, vp, table = _paged(k, v, lens, seed)
    sizes = {"out": B * H * 64, "lse": B * H, "o_part": B * H * S * 64, "ml_part": B * H * S * 2}
    buf = {name: torch.full((n + pad,), 7.0, device=DEV, dtype=torch.bfloat16 if name == "out" else torch.float32)
           for name, n in sizes.items()}
    geo = _native().attn_decode_paged(do.pack_q(q, Hkv).to(DEV), kp, vp, table, lens.to(DEV), H, Hkv, 0.125,
                                      int(splits or 0), buf["out"][:sizes["out"]].view(B, 1, H * 64),
                                      buf["o_part"][:sizes["o_part"]], buf["ml_part"][:sizes["ml_part"]],
                                      buf["lse"][:sizes["lse"]].view(B, H))
    torch.cuda.synchronize()
    assert tuple(geo) == (S, C)
    for name, n in sizes.items():
        assert bool((buf[name][n:] == 7.0).all()), f"{name}: sentinel behind the buffer overwritten (S = {S}, C = {C})"
    return buf["out"][:sizes["out"]].view(B, H, 64).cpu(), buf["lse"][:sizes["lse"]].view(B, H).cpu(), (S, C)


_CASES = {}


def _case(H, Hkv, i, amplitude):
    """Inputs and their fp64 reference, computed once and shared by the cases that differ in the split only."""
    key = (H, Hkv, i, amplitude)
    if key not in _CASES:
        q, k, v, lens_t = do.decode_inputs(B, H, Hkv, CAP, LENS[i], amplitude, seed=31 * H + Hkv + i, stale="nan")
        _CASES[key] = (q, k, v, lens_t) + do.decode_oracle(q, k, v, lens_t)
    return _CASES[key]


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_envelope_at_every_seam(H, Hkv, splits, amplitude):
    worst = 0.0
    for i, lens in enumerate(LENS):
        q, k, v, lens_t, ref, env = _case(H, Hkv, i, amplitude)
        O, lse, (S, C) = _run(q, k, v, lens_t, H, Hkv, splits)
        assert not torch.isnan(O.float()).any(), f"NaN behind the last key or from an unused page reached O (lens {lens}, S = {S})"
        name = f"H{H} Hkv{Hkv} S{S} C{C} lens{lens} a{amplitude}"
        worst = max(worst, oe.assert_within(O, ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="O " + name))
        oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE " + name)
    print(f"H{H} Hkv{Hkv} splits {splits} amplitude {amplitude}: worst O ratio {worst:.3f} of {oe.ATTN_C}")


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_onehot_probe_bit_for_bit(H, Hkv, splits):
    lens = (319, 200, 64)
    # the hot key either side of the 16-key, page and chunk boundaries, and at the last valid position
    for hot in [(0, 0, 0), (15, 16, 17), (63, 64, 64), (127, 128, 48), (191, 192, 63), (255, 199, 1), (319, 200, 64)]:
        q, k, v, lens_t = do.onehot_probe(B, H, Hkv, CAP, lens, hot)
        O, _, (S, C) = _run(q, k, v, lens_t, H, Hkv, splits)
        msg = do.describe_onehot_mismatch(O, v, lens_t, hot, H, Hkv, C)
        assert msg is None, f"S = {S}: {msg}"


@pytest.mark.parametrize("splits", SPLITS)
def test_the_page_permutation_does_not_change_a_bit(splits):
    q, k, v, lens_t = do.decode_inputs(B, 6, 2, CAP, (100, 255, 319), 4.0, seed=2, stale="nan")
    a, la, _ = _run(q, k, v, lens_t, 6, 2, splits, seed=0)
    b, lb, _ = _run(q, k, v, lens_t, 6, 2, splits, seed=1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(la, lb)


@pytest.mark.parametrize("Tn", [1, 5, 70])
def test_append_equals_the_contiguous_append(Tn):
    """lens (0, 60, 130): a run from 60 crosses into page 1 with Tn = 5, Tn = 70 crosses a boundary from every
    start. Slot 2 has no page 3 (positions 192 ..): its rows there are rotated in qkv and stored nowhere."""
    from pytorch_distributed_training_example_amd.ops.rope import rope_append_, rope_append_paged_, rope_table
    H, Hkv = 4, 2
    g = torch.Generator().manual_seed(Tn)
    qkv = torch.randn(B, Tn, (H + 2 * Hkv) * 64, generator=g).to(torch.bfloat16).to(DEV)
    cos, sin = (t.to(DEV) for t in rope_table(CAP))
    lens = torch.tensor([0, 60, 130], dtype=torch.int32, device=DEV)
    kc = torch.full((B, Hkv, CAP, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    kp, vp, table = _paged(kc.cpu(), vc.cpu(), torch.tensor([319, 319, 191]), seed=3, fill=7.0)  # before any append
    assert bool((kp == 7.0).all()) and bool((vp == 7.0).all())  # every stored row below is the paged kernel's own
    want = rope_append_(qkv.clone(), cos, sin, H, Hkv, kc, vc, lens)
    got = rope_append_paged_(qkv.clone(), cos, sin, H, Hkv, kp, vp, table, lens)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not bool((kc[0, :, :Tn] == 7.0).all())  # the contiguous append did store: the comparison is not 7 == 7
    named = table >= 0
    for pool, c in ((kp, kc), (vp, vc)):
        rows = c.view(B, Hkv, MP, 64, 64).permute(0, 2, 1, 3, 4)[named]  # the contiguous rows of the named pages
        assert torch.equal(pool[table[named].long()].view(torch.int16), rows.view(torch.int16))
        unnamed = torch.ones(NP, dtype=torch.bool, device=DEV)
        unnamed[table[named].long()] = False
        assert int(unnamed.sum()) == NP - 13 and bool((pool[unnamed] == 7.0).all()), "a page outside the table was written"


@pytest.mark.parametrize("what,match", [("pool rank", "n_pages, kv_heads, 64, 64"), ("table dtype", "int32"),
                                        ("two tokens", "one new token"), ("no scratch", "scratch")])
def test_binding_refusals(what, match):
    H, Hkv = 4, 2
    qkv = torch.zeros(B, 2 if what == "two tokens" else 1, (H + 2 * Hkv) * 64, device=DEV, dtype=torch.bfloat16)
    pool = torch.zeros(NP, Hkv, 64, 64, device=DEV, dtype=torch.bfloat16)
    table = torch.full((B, MP), -1, device=DEV, dtype=torch.int32)
    lens = torch.zeros(B, device=DEV, dtype=torch.int32)
    out = torch.empty(B, 1, H * 64, device=DEV, dtype=torch.bfloat16)
    if what == "pool rank":
        pool = pool.view(NP * Hkv, 64, 64)
    if what == "table dtype":
        table = table.long()
    with pytest.raises(RuntimeError, match=match):
        _native().attn_decode_paged(qkv, pool, pool, table, lens, H, Hkv, 0.125, 2 if what == "no scratch" else 1, out)
