"""decode_oracle.py is sharp: on the CPU, an emulation of the split-KV kernel's rounding points fits the
envelope with room, and each planted fault leaves it. Also proves the one-hot probe's claim (bit-for-bit V
row at any split) and the append's position rule, all without a GPU."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe

CAP = 320
SHAPES = [(4, 4), (4, 2), (4, 1), (32, 2)]  # G = 1, 2, 4, 16
LENS = [(0, 15, 63), (64, 127, 128), (191, 192, 319), (16, 62, 126)]

_worst = {}


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("C", [64, 128, 320])
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_emulation_fits_the_envelope(H, Hkv, C, amplitude):
    for i, lens in enumerate(LENS):
        q, k, v, lens_t = do.decode_inputs(3, H, Hkv, CAP, lens, amplitude, seed=7 * H + Hkv + i, stale="nan")
        ref, env = do.decode_oracle(q, k, v, lens_t)
        O, lse = do.emulate_decode(q, k, v, lens_t, C)
        r = oe.assert_within(O, ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name=f"O H{H} Hkv{Hkv} C{C} a{amplitude}",
                             record=_worst)
        oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE")
        assert r <= oe.ATTN_C
    print("worst emulation / envelope ratio so far:", max(_worst.values()))


@pytest.mark.parametrize("fault", do.FAULTS)
def test_planted_faults_leave_the_envelope(fault):
    # three splits of 64 with different maxima (amplitude 4), two K/V heads of two query heads each,
    # stale rows that look like real ones
    # an off-by-one in n shows where one key carries weight: few keys, smooth scores
    lens, amplitude = ((1, 2, 65), 1.0) if fault in ("last_key_out", "stale_row") else ((140, 150, 191), 4.0)
    q, k, v, lens_t = do.decode_inputs(3, 4, 2, 192, lens, amplitude, seed=11, stale="randn")
    ref, env = do.decode_oracle(q, k, v, lens_t)
    good, _ = do.emulate_decode(q, k, v, lens_t, 64)
    assert oe.worst_ratio(good, ref["O"], env["O"], oe.FLOOR)[0] <= oe.ATTN_C
    bad, _ = do.emulate_decode(q, k, v, lens_t, 64, fault=fault)
    ratio, _ = oe.worst_ratio(bad, ref["O"], env["O"], oe.FLOOR)
    assert ratio > 10 * oe.ATTN_C, (fault, ratio)
    with pytest.raises(AssertionError):
        oe.assert_within(bad, ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name=fault)


@pytest.mark.parametrize("C", [64, 128, 320])
def test_onehot_probe_is_exact_at_any_split(C):
    lens = (319, 130, 64)
    for hot in [(0, 0, 0), (63, 64, 64), (64, 127, 15), (319, 130, 16), (128, 129, 63)]:
        q, k, v, lens_t = do.onehot_probe(3, 4, 2, CAP, lens, hot)
        O, _ = do.emulate_decode(q, k, v, lens_t, C, scale=0.125)
        assert do.describe_onehot_mismatch(O, v, lens_t, hot, 4, 2, C) is None
    # and the report names the key, the chunk and the head when the wrong row comes back
    q, k, v, lens_t = do.onehot_probe(3, 4, 2, CAP, lens, (5, 70, 20))
    O, _ = do.emulate_decode(q, k, v, lens_t, C, scale=0.125)
    msg = do.describe_onehot_mismatch(O, v, lens_t, (5, 71, 20), 4, 2, C)
    assert msg is not None and "sequence 1" in msg and "hot key 71" in msg and f"chunk {71 // C}" in msg and "head 0" in msg


def test_append_position_rule_and_its_planted_fault():
    from pytorch_distributed_training_example_amd.ops.rope import rope_table
    H, Hkv, Tn, T_full = 4, 2, 5, 40
    cos, sin = rope_table(T_full)
    lens = torch.tensor([0, 7, 35], dtype=torch.int32)
    g = torch.Generator().manual_seed(3)
    new = torch.randn(3, Tn, (H + 2 * Hkv) * 64, generator=g).to(torch.bfloat16)
    full = do.full_sequence(new, lens, T_full)
    ref, env = do.gqa_rope_oracle(full, cos, sin, H, Hkv)
    rows = torch.stack([torch.arange(Tn) + int(n) for n in lens])  # [B, Tn] positions
    pick = lambda x: torch.stack([x[b, rows[b]] for b in range(3)])  # noqa: E731
    good = do.emulate_append(new, cos, sin, H, Hkv, lens)
    oe.assert_within(good, pick(ref), pick(env), do.ROPE_C, name="append rotation")
    bad = do.emulate_append(new, cos, sin, H, Hkv, lens, at_t=True)
    assert torch.equal(bad[0], good[0])  # lens 0: t is the position
    with pytest.raises(AssertionError):
        oe.assert_within(bad, pick(ref), pick(env), do.ROPE_C, name="rotation at t")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_append_reference_op(dtype):
    """``rope_append_`` on the CPU (its PyTorch reference): the rotated Q and K in qkv and the K/V rows in the
    caches against the fp64 oracle at positions lens[b] + t (the cache holds qkv's rotated K), rows past the capacity
    (sequence 2: positions 22, 23 fit, 24 .. 26 do not) written nowhere, every other cache row untouched."""
    from pytorch_distributed_training_example_amd.ops.rope import rope_append_, rope_table
    H, Hkv, Tn, cap, B = 4, 2, 5, 24, 3
    R = (H + Hkv) * 64
    cos, sin = rope_table(32)
    lens = torch.tensor([0, 7, 22], dtype=torch.int32)
    g = torch.Generator().manual_seed(4)
    new = torch.randn(B, Tn, (H + 2 * Hkv) * 64, generator=g).to(dtype)
    k = torch.full((B, Hkv, cap, 64), 3.0, dtype=dtype)
    v = torch.full((B, Hkv, cap, 64), 3.0, dtype=dtype)
    qkv = new.clone()
    assert rope_append_(qkv, cos, sin, H, Hkv, k, v, lens) is qkv
    ref, env = do.gqa_rope_oracle(do.full_sequence(new, lens, 32), cos, sin, H, Hkv)
    written = torch.zeros(B, cap, dtype=torch.bool)
    for b in range(B):
        for t in range(Tn):
            p = int(lens[b]) + t
            if p >= cap:
                assert torch.equal(qkv[b, t], new[b, t]), (b, t, "a row past the capacity was changed")
                continue
            written[b, p] = True
            assert torch.equal(qkv[b, t, R:], new[b, t, R:]), (b, t, "the V columns of qkv changed")
            oe.assert_within(qkv[b, t], ref[b, p], env[b, p], do.ROPE_C, oe.FLOOR, name=f"row ({b}, {t})")
            assert torch.equal(k[b, :, p].reshape(-1), qkv[b, t, H * 64:R]), (b, t, "K row in the cache")
            assert torch.equal(v[b, :, p].reshape(-1), new[b, t, R:]), (b, t, "V row in the cache")
    untouched = ~written[:, None, :, None].expand(B, Hkv, cap, 64)
    assert bool((k[untouched] == 3.0).all()) and bool((v[untouched] == 3.0).all())
    with pytest.raises(RuntimeError, match="inference only"):
        rope_append_(new.clone().requires_grad_(), cos, sin, H, Hkv, k, v, lens)
    with pytest.raises(ValueError, match="caches"):
        rope_append_(new.clone(), cos, sin, H, Hkv, k[:, :1], v[:, :1], lens)


def test_reference_ops_agree_with_the_oracle():
    """``attention_decode`` on the CPU (its PyTorch reference) against the oracle, NaN behind the last key
    included."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode
    q, k, v, lens_t = do.decode_inputs(3, 4, 2, 96, (0, 40, 95), 1.0, seed=5, stale="nan")
    ref, env = do.decode_oracle(q, k, v, lens_t)
    out, lse = attention_decode(do.pack_q(q, 2), k, v, lens_t, 4, 2, return_lse=True)
    oe.assert_within(out.view(3, 4, 64), ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="reference O")
    oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_SMOOTH, name="reference LSE")
