"""The e4m3 paged KV cache without a GPU: its pools, the reference append and decode that the kernels of
csrc/kernels/attn_paged_fp8.hip are held to, the command line and the refusals."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe

FP8 = torch.float8_e4m3fn


def _cache(**kw):
    from pytorch_distributed_training_example_amd.ops.kv_cache import PagedKVCache
    return PagedKVCache(2, 3, 2, 7, 4, "cpu", **kw)


def quantised(c):
    """(bytes [..., 64] e4m3, scales [...], dequantised fp32) of the bf16 rows ``c`` [..., 64]."""
    from pytorch_distributed_training_example_amd.ops.linear import quantize_rows_e4m3
    q, s = quantize_rows_e4m3(c.reshape(-1, 64))
    q, s = q.view(c.shape), s.view(c.shape[:-1])
    return q, s, q.float() * s[..., None]


def test_pools_scales_and_an_unchanged_allocator():
    c, ref = _cache(dtype=FP8), _cache()
    assert c.fp8 and not ref.fp8 and ref.k_scale is None
    for l in range(2):
        assert c.k[l].shape == c.v[l].shape == (7, 2, 64, 64) and c.k[l].dtype == c.v[l].dtype == FP8
        assert c.k_scale[l].shape == c.v_scale[l].shape == (7, 2, 64) and c.k_scale[l].dtype == torch.float32
    for x in (c, ref):
        x.admit(0), x.admit(2)
        x.reserve(70)
        x.advance(70)
        x.free(0)
        x.admit(1)
        x.reserve(130, slots=[1])
    assert c.pages_of(1) == ref.pages_of(1) and c.pages_of(2) == ref.pages_of(2) and c.free_pages == ref.free_pages
    assert torch.equal(c.block_table, ref.block_table) and torch.equal(c.lens, ref.lens) and c.bounds == ref.bounds


@pytest.mark.parametrize("Tn,lens", [(1, (0, 62)), (3, (62, 0)), (70, (62, 0))])
def test_reference_append_stores_quantize_rows_of_the_bf16_rows(Tn, lens):
    from pytorch_distributed_training_example_amd.ops.rope import rope_append_paged_, rope_append_paged_fp8_, rope_table
    H, Hkv, NP, MP = 4, 2, 7, 3
    qkv = torch.randn(2, Tn, (H + 2 * Hkv) * 64, generator=torch.Generator().manual_seed(Tn)).to(torch.bfloat16)
    cos, sin = rope_table(192)
    table = torch.tensor([[5, 2, 6], [0, 3, -1]], dtype=torch.int32)  # slot 1 has no third page
    lens = torch.tensor(lens, dtype=torch.int32)
    kb, vb = (torch.full((NP, Hkv, 64, 64), 7.0, dtype=torch.bfloat16) for _ in range(2))
    want = rope_append_paged_(qkv.clone(), cos, sin, H, Hkv, kb, vb, table, lens)
    kq, vq = (torch.full((NP, Hkv, 64, 64), 0x7F, dtype=torch.uint8).view(FP8) for _ in range(2))
    ks, vs = (torch.full((NP, Hkv, 64), float("nan")) for _ in range(2))
    got = rope_append_paged_fp8_(qkv.clone(), cos, sin, H, Hkv, kq, vq, ks, vs, table, lens)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    for pb, pq, ps in ((kb, kq, ks), (vb, vq, vs)):
        written = ~(pb == 7.0).all(-1)  # [NP, Hkv, 64]: the rows the bf16 reference stored
        assert int(written.sum()) == Hkv * sum(min(Tn, 64 * (3 if b == 0 else 2) - int(lens[b])) for b in range(2))
        q, s, _ = quantised(pb[written])
        assert torch.equal(pq.view(torch.uint8)[written], q.view(torch.uint8)) and torch.equal(ps[written], s)
        assert bool((pq.view(torch.uint8)[~written] == 0x7F).all()) and bool(ps[~written].isnan().all())


def test_reference_decode_is_inside_the_envelope_on_the_gpu_tests_smallest_inputs():
    """If the reference alone left ATTN_C * E_O of the oracle on K^, V^, the inputs would be wrong, not the constant."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_paged_fp8
    B, H, Hkv, MP = 3, 2, 2, 4
    q, k, v, lens = do.decode_inputs(B, H, Hkv, 64 * MP, (0, 63, 255), 4.0, seed=3, stale="zero")
    (kq, ks, kh), (vq, vs, vh) = quantised(k), quantised(v)
    ref, env = do.decode_oracle(q, kh, vh, lens)
    paged = lambda c: c.view(B, Hkv, MP, 64, *c.shape[3:]).transpose(1, 2).reshape(B * MP, Hkv, 64, *c.shape[3:])
    table = torch.arange(B * MP, dtype=torch.int32).view(B, MP)
    O, lse = attention_decode_paged_fp8(do.pack_q(q, Hkv), paged(kq), paged(vq), paged(ks), paged(vs), table, lens, H,
                                        Hkv, return_lse=True)
    worst = oe.assert_within(O.view(B, H, 64), ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="reference decode")
    oe.assert_abs(lse, ref["LSE"], oe.LSE_TOL_PEAKED, name="reference LSE")
    print(f"reference decode on dequantised rows: worst O ratio {worst:.3f} of {oe.ATTN_C}")


def test_command_line_accepts_paged_fp8():
    from pytorch_distributed_training_example_amd.cli import build_parser
    assert build_parser().parse_args(["--sample-cache", "paged-fp8"]).sample_cache == "paged-fp8"


def test_refusals():
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache
    with pytest.raises(NotImplementedError, match="contiguous"):
        KVCache(1, 1, 1, 64, "cpu", dtype=FP8)
    model = get_model("llama_tiny", block_size=128).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (1, 8), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="kv_dtype"):
        model.new_paged_cache(1, 2, kv_dtype="int8")
    with pytest.raises(NotImplementedError, match="prefill_chunk"):
        model.generate(idx, 2, paged=True, kv_dtype="fp8", prefill_chunk=4)
    with pytest.raises(NotImplementedError, match="paged=True"):
        model.generate(idx, 2, kv_dtype="fp8")
    with torch.no_grad():
        cache = model.new_paged_cache(1, 2, kv_dtype="fp8")
        cache.admit(0)
        cache.reserve(8)
        model.prefill(idx, cache)
        cache.reserve(3)
        before = [t.clone() for t in cache.k_scale]
        with pytest.raises(NotImplementedError, match="out of scope"):
            model.extend(idx[:, :3], cache, slots=[0])
        assert all(torch.equal(a, b) for a, b in zip(before, cache.k_scale)) and cache.lens.tolist() == [8]
        assert model.generate(idx, 3, paged=True, kv_dtype="fp8").shape == (1, 3)
