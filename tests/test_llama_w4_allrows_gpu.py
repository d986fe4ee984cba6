"""Llama.quantize_decode_weights("int4", all_rows=True) on the MI355X: calls on more than 64 rows really run the
any-row W4A16 GEMM, the default still leaves them on the bf16 weights bit for bit, and prefill + decode on the int4
weights is as close to the fp32 forward of the dequantised weights as the bf16 cached path is to its own."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["llama_tiny", "llama_tiny_gqa"]
B, T0, TN, STEPS = 4, 40, 20, 8  # a 160-row prefill, an 80-row extend


def _model(name):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model(name)).to(DEV).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, T0 + TN), generator=torch.Generator().manual_seed(1)).to(DEV)
    return model, idx[:, :T0].contiguous(), idx[:, T0:].contiguous()


def _cached_error(model, idx, ref):
    """max |cached logits - ``ref``'s fp32 full forward|, last prompt position and STEPS greedy steps."""
    with torch.no_grad():
        cache = model.new_cache(B, T0 + STEPS + 1)
        out, seq = [model.prefill(idx, cache)], idx
        for _ in range(STEPS):
            tok = out[-1].argmax(-1)
            seq = torch.cat([seq, tok[:, None]], 1)
            out.append(model.decode_step(tok, cache))
        want = ref(seq.cpu())[:, T0 - 1:]
    return (torch.stack(out, 1).float().cpu() - want).abs().max().item()


@pytest.mark.parametrize("name", NAMES)
def test_the_default_leaves_tall_calls_on_the_bf16_weights(name):
    # an extend of an empty cache with all logits: the LM head sees 160 rows too (a prefill's runs on B = 4)
    from pytorch_distributed_training_example_amd.ops.linear import SKINNY_STATS as st
    model, idx, _ = _model(name)
    with torch.no_grad():
        plain, t0 = model.extend(idx, model.new_cache(B)), st.get("w4_tall_calls", 0)
        model.quantize_decode_weights("int4")
        assert torch.equal(model.extend(idx, model.new_cache(B)), plain) and st.get("w4_tall_calls", 0) == t0


@pytest.mark.parametrize("name", NAMES)
def test_all_rows_routes_tall_calls_to_the_w4_gemm(name):
    from pytorch_distributed_training_example_amd.ops.linear import SKINNY_STATS as st
    model, idx, more = _model(name)
    nl = model.cfg.n_layer
    with torch.no_grad():
        plain = model.prefill(idx, model.new_cache(B))
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        t0 = st["w4_tall_calls"]
        model.quantize_decode_weights("int4", all_rows=True)
        assert list(model.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
        cache, s0 = model.new_cache(B), st["w4_calls"]
        logits = model.prefill(idx, cache)  # lm_head sees B rows: the skinny kernel
        assert (st["w4_tall_calls"] - t0, st["w4_calls"] - s0) == (4 * nl, 1) and not torch.equal(logits, plain)
        assert model.extend(more, cache).shape == (B, TN, model.cfg.vocab_size) and st["w4_tall_calls"] - t0 == 8 * nl + 1
        model.decode_step(more[:, 0].contiguous(), cache)
        assert st["w4_tall_calls"] - t0 == 8 * nl + 1
        model.transformer.h[0].mlp.c_fc.weight.mul_(1.0)  # an in-place update: the int4 copy is stale
        with pytest.raises(RuntimeError, match="quantize_decode_weights"):
            model.prefill(idx, model.new_cache(B))
    with pytest.raises(NotImplementedError, match="W8A16"):
        model.quantize_decode_weights("fp8", all_rows=True)


@pytest.mark.parametrize("name", NAMES)
def test_all_rows_logits_are_as_close_to_their_fp32_forward_as_bf16_is(name):
    # bound: twice the unquantised bf16 cached path's own error, measured here: fp32 accumulation + one rounding
    from pytorch_distributed_training_example_amd.ops.linear import dequantize_groups_int4
    model, idx, _ = _model(name)
    original = copy.deepcopy(model).float().cpu()
    e_bf16 = _cached_error(model, idx, original)
    model.quantize_decode_weights("int4", all_rows=True)
    ref = copy.deepcopy(original)
    for mod, src in zip(ref._decode_linears(), model._decode_linears()):
        mod.weight.data.copy_(dequantize_groups_int4(src._w4[0], src._w4[1]))
    e_w4 = _cached_error(model, idx, ref)
    print(f"{name}: e_w4 = {e_w4:.4g} against the dequantised weights, e_bf16 = {e_bf16:.4g}, ratio {e_w4 / e_bf16:.3f}")
    assert e_w4 <= 2 * e_bf16, (e_w4, e_bf16)
