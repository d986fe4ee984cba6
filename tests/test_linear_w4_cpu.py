"""The CPU side of weight-only int4 decoding: the torch formulas of ops/linear.py (quantise, pack / unpack,
dequantise, the fallback of linear_skinny_w4) and the CLI's choice."""
import pytest
import torch


def test_pack_places_every_value_where_the_layout_says_and_unpack_inverts_it():
    from pytorch_distributed_training_example_amd.ops import linear as L
    N, K = 3, 512
    q = torch.randint(-8, 8, (N, K), generator=torch.Generator().manual_seed(0)).to(torch.int8)
    wq = L.pack_int4(q)
    assert wq.shape == (N, K // 2) and wq.dtype == torch.uint8 and torch.equal(L.unpack_int4(wq), q)
    words = wq.view(torch.int32).view(N, K // 256, 4, 8)  # [n, line s, lane group g, word i]
    for n, s, g, i, j in [(0, 0, 0, 0, 0), (1, 1, 3, 7, 7), (2, 0, 2, 5, 3), (1, 0, 1, 4, 6)]:
        nib = (int(words[n, s, g, i]) >> (4 * (j // 2) + 16 * (j % 2))) & 15
        assert (nib - 16 if nib > 7 else nib) == int(q[n, 256 * s + 32 * i + 8 * g + j])


def test_quantize_groups_and_linear_w4_follow_the_formulas_on_the_cpu():
    from pytorch_distributed_training_example_amd.ops import linear as L
    from pytorch_distributed_training_example_amd.ops.swiglu import swiglu
    w = torch.randn(32, 512, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    w[3, 128:256] = 0
    wq, scale = L.quantize_groups_int4(w)
    assert wq.shape == (32, 256) and wq.dtype == torch.uint8 and scale.shape == (4, 32) and scale.dtype == torch.float32
    amax = w.float().view(32, 4, 128).abs().amax(2)
    q = L.unpack_int4(wq).view(32, 4, 128)
    assert scale[1, 3] == 1 and not q[3, 1].any()
    keep = amax > 0
    assert torch.equal(scale.t()[keep], amax[keep] * torch.tensor(1 / 7, dtype=torch.float32))
    assert q.abs().amax(2)[keep].eq(7).all() and q.abs().max() == 7  # every group's amax lands on 7; -8 never
    deq = L.dequantize_groups_int4(wq, scale)
    assert torch.equal(deq.view(32, 4, 128), q.float() * scale.t()[:, :, None])
    # half a step is amax / 14; scale and 7 / amax carry three fp32 roundings on a grid point of at most amax
    err = (deq.double() - w.double()).abs().view(32, 4, 128)
    assert (err <= amax.double()[:, :, None] * (1 / 14 + 2.0 ** -20)).all()
    x = torch.randn(2, 3, 512).to(torch.bfloat16)
    n0 = L.SKINNY_STATS["w4_calls"]
    want = torch.nn.functional.linear(x, deq.to(torch.bfloat16))
    assert torch.equal(L.linear_skinny_w4(x, wq, scale), want)
    assert torch.equal(L.linear_skinny_w4(x, wq, scale, swiglu=True), swiglu(want))
    assert L.SKINNY_STATS["w4_calls"] == n0 and not L.skinny_w4_ok(x, wq, scale)
    with pytest.raises(ValueError, match="NaN or Inf"):
        L.quantize_groups_int4(torch.full((16, 256), float("nan"), dtype=torch.bfloat16))


def test_cli_takes_int4_sample_weights_for_llama_and_refuses_them_elsewhere():
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit, match="--sample-weights int4"):
        cli.main(["--model", "mlp", "--sample-weights", "int4"])
    args = cli.build_parser().parse_args(["--model", "llama_tiny", "--sample-tokens", "2", "--sample-weights", "int4"])
    assert cli.sample_args_error(args) is None and args.sample_weights == "int4"
