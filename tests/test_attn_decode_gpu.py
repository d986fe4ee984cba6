"""The split-KV decode attention kernel (csrc/kernels/attn_decode.hip) against decode_oracle.py: every
output element inside the envelope at every seam of the chunking, a one-hot probe that must return a V
row bit for bit, NaN behind the last key, sentinels behind every buffer the kernel writes, run-to-run
bits, and the binding's refusals. B = 3 with three different lens per launch; capacity 320, so a forced
chunk of 64 gives five splits."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe

pytestmark = pytest.mark.gpu

CAP = 320
SHAPES = [(4, 4), (4, 2), (4, 1), (6, 2), (32, 1)]  # (32, 1): two passes of 16 query heads
# every seam: one key, the 16-key subtile and 64-key step boundaries, either side of the chunk boundaries of
# C = 64 / 128 / 192 / 256, and the last position of the cache
LENS = [(0, 14, 15), (16, 62, 63), (64, 126, 127), (128, 191, 192), (129, 255, 256), (65, 318, 319)]
SPLITS = [1, 2, 3, 5, None]  # None: the default rule, (2, 256) here; 5: chunks of 64, every 64-key seam a chunk seam


def _native():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _geo(Hkv, G, splits):
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_geo
    return attention_decode_geo(3, Hkv, CAP, splits, G)


def _run(q, k, v, lens, H, Hkv, splits, scale=None, pad=256):
    """The binding itself, on buffers with sentinel tails behind the output, the LSE and both scratch
    tensors. Returns (O [B, H, 64] cpu, LSE cpu, (S, C))."""
    dev = "cuda"
    B = q.shape[0]
    S, C = _geo(Hkv, H // Hkv, splits)
    qkv = do.pack_q(q, Hkv).to(dev)
    out = torch.full((B * H * 64 + pad,), 7.0, device=dev, dtype=torch.bfloat16)
    lse = torch.full((B * H + pad,), 7.0, device=dev)
    o_part = torch.full((B * H * S * 64 + pad,), 7.0, device=dev)
    ml_part = torch.full((B * H * S * 2 + pad,), 7.0, device=dev)
    geo = _native().attn_decode(qkv, k.to(dev), v.to(dev), lens.to(dev), H, Hkv, scale or 0.125, int(splits or 0),
                                out[:B * H * 64].view(B, 1, H * 64), o_part[:B * H * S * 64],
                                ml_part[:B * H * S * 2], lse[:B * H].view(B, H))
    torch.cuda.synchronize()
    assert tuple(geo) == (S, C)
    for name, buf, n in (("out", out, B * H * 64), ("lse", lse, B * H), ("o_part", o_part, B * H * S * 64),
                         ("ml_part", ml_part, B * H * S * 2)):
        assert bool((buf[n:] == 7.0).all()), f"{name}: sentinel behind the buffer overwritten (S = {S}, C = {C})"
    return out[:B * H * 64].view(B, H, 64).cpu(), lse[:B * H].view(B, H).cpu(), (S, C)


_CASES = {}


def _case(H, Hkv, i, amplitude):
    """Inputs and their fp64 reference, computed once and shared by the cases that differ in the split only."""
    key = (H, Hkv, i, amplitude)
    if key not in _CASES:
        q, k, v, lens_t = do.decode_inputs(3, H, Hkv, CAP, LENS[i], amplitude, seed=31 * H + Hkv + i, stale="nan")
        _CASES[key] = (q, k, v, lens_t) + do.decode_oracle(q, k, v, lens_t)
    return _CASES[key]


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_geometry(H, Hkv, splits):
    S, C = _geo(Hkv, H // Hkv, splits)
    assert C % 64 == 0 and S * C >= CAP and (S - 1) * C < CAP
    want = {1: (1, 320), 2: (2, 192), 3: (3, 128), 5: (5, 64)}
    if splits is not None:
        assert (S, C) == want[splits]
    elif H // Hkv <= 4:
        assert (S, C) == (2, 256)  # B Hkv <= 12 workgroups alone: the default rule splits down to its 256-key floor
    else:
        assert (S, C) == (1, 320)  # G = 32: chunks of at least 16 G keys keep the merge small


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_envelope_at_every_seam(H, Hkv, splits, amplitude):
    worst = 0.0
    for i, lens in enumerate(LENS):
        q, k, v, lens_t, ref, env = _case(H, Hkv, i, amplitude)
        O, lse, (S, C) = _run(q, k, v, lens_t, H, Hkv, splits)
        assert not torch.isnan(O.float()).any(), f"NaN behind the last key reached O (lens {lens}, S = {S})"
        name = f"H{H} Hkv{Hkv} S{S} C{C} lens{lens} a{amplitude}"
        worst = max(worst, oe.assert_within(O, ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="O " + name))
        oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE " + name)
    print(f"H{H} Hkv{Hkv} splits {splits} amplitude {amplitude}: worst O ratio {worst:.3f} of {oe.ATTN_C}")


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("H,Hkv", [(4, 2), (6, 2), (32, 1)])
def test_onehot_probe_bit_for_bit(H, Hkv, splits):
    lens = (319, 200, 64)
    # the hot key across 16-key, 64-key and chunk boundaries, and at the last valid position
    for hot in [(0, 0, 0), (15, 16, 17), (63, 64, 64), (127, 128, 48), (191, 192, 63), (255, 199, 1), (319, 200, 64)]:
        q, k, v, lens_t = do.onehot_probe(3, H, Hkv, CAP, lens, hot)
        O, _, (S, C) = _run(q, k, v, lens_t, H, Hkv, splits, scale=0.125)
        msg = do.describe_onehot_mismatch(O, v, lens_t, hot, H, Hkv, C)
        assert msg is None, f"S = {S}: {msg}"


@pytest.mark.parametrize("splits", [1, None])
def test_two_runs_give_identical_bits(splits):
    q, k, v, lens_t = do.decode_inputs(3, 6, 2, CAP, (100, 255, 319), 4.0, seed=2, stale="nan")
    a, la, _ = _run(q, k, v, lens_t, 6, 2, splits)
    b, lb, _ = _run(q, k, v, lens_t, 6, 2, splits)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(la, lb)


def test_op_uses_the_kernel_and_the_cache_scratch():
    from pytorch_distributed_training_example_amd.ops import attention as A
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    q, k, v, lens_t = do.decode_inputs(3, 4, 2, CAP, (5, 77, 300), 1.0, seed=9, stale="nan")
    cache = KVCache(1, 3, 2, CAP, "cuda")
    cache.k[0].copy_(k)
    cache.v[0].copy_(v)
    cache.set_lens(lens_t)
    assert cache.bound == 300
    before = A.DECODE_STATS["native_calls"]
    out = A.attention_decode(do.pack_q(q, 2).cuda(), cache.k[0], cache.v[0], cache.lens, 4, 2, cache=cache)
    assert A.DECODE_STATS["native_calls"] == before + 1 and A.DECODE_STATS["geo"] == (2, 256)
    part = cache.scratch(4, 2)
    assert part[0].shape == (3, 4, 2, 64) and cache.scratch(4, 2)[0] is part[0]  # allocated once
    ref, env = do.decode_oracle(q, k, v, lens_t)
    oe.assert_within(out.view(3, 4, 64).cpu(), ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="op O")
    with pytest.raises(RuntimeError, match="inference only"):
        with torch.enable_grad():
            A.attention_decode(do.pack_q(q, 2).cuda().requires_grad_(), cache.k[0], cache.v[0], cache.lens, 4, 2)


def test_binding_refusals():
    n = _native()
    dev = "cuda"
    H, Hkv, B = 4, 2, 3
    qkv = torch.zeros(B, 1, (H + 2 * Hkv) * 64, device=dev, dtype=torch.bfloat16)
    k = torch.zeros(B, Hkv, CAP, 64, device=dev, dtype=torch.bfloat16)
    lens = torch.zeros(B, device=dev, dtype=torch.int32)
    out = torch.empty(B, 1, H * 64, device=dev, dtype=torch.bfloat16)

    def call(qkv=qkv, k=k, v=k, lens=lens, heads=H, kv_heads=Hkv, out=out):
        return n.attn_decode(qkv, k, v, lens, heads, kv_heads, 0.125, 1, out)

    call()  # the baseline is accepted
    with pytest.raises(RuntimeError, match="bf16"):
        call(qkv=qkv.float())
    with pytest.raises(RuntimeError, match="bf16"):
        call(k=k.float(), v=k.float())
    with pytest.raises(RuntimeError, match="head dim"):
        call(k=torch.zeros(B, Hkv, CAP, 128, device=dev, dtype=torch.bfloat16), v=torch.zeros(B, Hkv, CAP, 128, device=dev, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="head dim"):
        call(qkv=torch.zeros(B, 1, (H + 2 * Hkv) * 32, device=dev, dtype=torch.bfloat16))
    wide = torch.zeros(B, Hkv, CAP, 128, device=dev, dtype=torch.bfloat16)[..., :64]
    with pytest.raises(RuntimeError, match="contiguous"):
        call(k=wide, v=wide)
    with pytest.raises(RuntimeError, match="multiple"):
        call(qkv=torch.zeros(B, 1, (3 + 2 * Hkv) * 64, device=dev, dtype=torch.bfloat16), heads=3)
    with pytest.raises(RuntimeError, match="int32"):
        call(lens=lens.long())
    with pytest.raises(RuntimeError, match="int32"):
        call(lens=lens.cpu())
    with pytest.raises(RuntimeError, match="scratch"):
        n.attn_decode(qkv, k, k, lens, H, Hkv, 0.125, 2, out)  # two splits and no scratch
    small = torch.empty(8, device=dev)
    with pytest.raises(RuntimeError, match="too small"):
        n.attn_decode(qkv, k, k, lens, H, Hkv, 0.125, 2, out, small, small)
