"""The CPU side of int4 weights at every row count: linear_w4's torch fallback, the model flag and the CLI's choice."""
import pytest
import torch


@pytest.mark.parametrize("rows", [3, 70])
def test_linear_w4_is_the_dequantised_matmul_on_the_cpu(rows):
    from pytorch_distributed_training_example_amd.ops import linear as L
    from pytorch_distributed_training_example_amd.ops.swiglu import swiglu
    g = torch.Generator().manual_seed(rows)
    wq, scale = L.quantize_groups_int4(torch.randn(32, 512, generator=g).to(torch.bfloat16))
    x = torch.randn(rows, 512, generator=g).to(torch.bfloat16)
    n0 = L.SKINNY_STATS["w4_tall_calls"]
    want = x @ L.dequantize_groups_int4(wq, scale).to(torch.bfloat16).t()
    assert torch.equal(L.linear_w4(x, wq, scale), want) and torch.equal(L.linear_w4(x, wq, scale, swiglu=True), swiglu(want))
    assert L.SKINNY_STATS["w4_tall_calls"] == n0 and not L.w4_ok(x, wq, scale)


def test_all_rows_flag_round_trips_on_the_cpu():
    from pytorch_distributed_training_example_amd.models import get_model
    model = get_model("llama_tiny").to(torch.bfloat16).eval()
    idx = torch.randint(0, 512, (2, 40), generator=torch.Generator().manual_seed(0))  # 80 rows
    with torch.no_grad():
        plain = model(idx)
        assert torch.equal(model.quantize_decode_weights("int4")(idx), plain)  # the default: bf16 weights
        model.quantize_decode_weights("int4", all_rows=True)
        assert all(m._w4[3] is True and len(m._w4) == 4 for m in model._decode_linears())
        assert not torch.equal(model(idx), plain)
        assert torch.equal(model.drop_decode_weights()(idx), plain)
    with pytest.raises(NotImplementedError, match="W8A16"):
        model.quantize_decode_weights("fp8", all_rows=True)


def test_cli_takes_int4_all_for_llama_and_refuses_it_elsewhere():
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit, match="--sample-weights int4-all"):
        cli.main(["--model", "mlp", "--sample-weights", "int4-all"])
    args = cli.build_parser().parse_args(["--model", "llama_tiny", "--sample-tokens", "2", "--sample-weights", "int4-all"])
    assert cli.sample_args_error(args) is None and args.sample_weights == "int4-all"
