"""The CPU side of weight-only e4m3 decoding: the torch formulas of ops/linear.py and the CLI's refusal."""
import pytest
import torch


def test_quantize_rows_and_linear_w8_follow_the_formulas_on_the_cpu():
    from pytorch_distributed_training_example_amd.ops import linear as L
    w = torch.randn(32, 128, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    w[3] = 0
    wq, scale = L.quantize_rows_e4m3(w)
    amax = w.float().abs().amax(1)
    assert wq.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert scale[3] == 1 and not wq.float()[3].any()
    keep = amax > 0
    assert torch.equal(scale[keep], amax[keep] * torch.tensor(1 / 448, dtype=torch.float32))
    assert torch.equal(wq.float()[keep], (w.float()[keep] * torch.full_like(amax[keep], 448).div(amax[keep])[:, None]).to(torch.float8_e4m3fn).float())
    assert wq.float().abs().amax(1)[keep].eq(448).all()  # every row's amax lands on the largest e4m3 number
    # half an e4m3 ulp in the top binade is 16 / 448 of amax; scale and 448 / amax carry three fp32 roundings
    err = (wq.double() * scale.double()[:, None] - w.double()).abs()
    assert (err <= amax.double()[:, None] * (1 / 28 + 2.0 ** -20)).all()
    x = torch.randn(2, 3, 128).to(torch.bfloat16)
    deq = (wq.float() * scale[:, None]).to(torch.bfloat16)
    n0 = L.SKINNY_STATS["w8_calls"]
    assert torch.equal(L.linear_skinny_w8(x, wq, scale), torch.nn.functional.linear(x, deq))
    from pytorch_distributed_training_example_amd.ops.swiglu import swiglu
    assert torch.equal(L.linear_skinny_w8(x, wq, scale, swiglu=True), swiglu(torch.nn.functional.linear(x, deq)))
    assert L.SKINNY_STATS["w8_calls"] == n0 and not L.skinny_w8_ok(x, wq, scale)
    with pytest.raises(ValueError, match="NaN or Inf"):
        L.quantize_rows_e4m3(torch.full((16, 128), float("nan"), dtype=torch.bfloat16))


def test_cli_refuses_fp8_sample_weights_for_a_model_without_generation():
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit, match="--sample-weights fp8"):
        cli.main(["--model", "mlp", "--sample-weights", "fp8"])
    args = cli.build_parser().parse_args(["--model", "llama_tiny", "--sample-tokens", "2", "--sample-weights", "fp8"])
    assert cli.sample_args_error(args) is None and cli.build_parser().parse_args([]).sample_weights == "bf16"
