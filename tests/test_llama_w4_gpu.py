"""Weight-only int4 decoding of the Llama decoder (Llama.quantize_decode_weights("int4"), MI355X): the decode-time
Linears really run the W4A16 skinny GEMM, the call leaves state_dict() alone, stale bytes are refused, dropping
the quantised weights restores the earlier bits, and the logits are as close to the fp32 forward of the
dequantised weights as the bf16 cached path is to the fp32 forward of its own. Nothing here judges int4 against
the original weights: that is the format's property (profiles/r26/skinny_w4_gemm.txt reports it)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["llama_tiny", "llama_tiny_gqa"]
B, T0, STEPS = 4, 12, 8
# Worst |logit error| of the bf16 cached path (prefill + 8 greedy decode steps, these prompts and seeds) against the
# fp32 forward of its own weights: tests/test_llama_w8_gpu.py's PARENT_ERR, measured on that path
PARENT_ERR = {"llama_tiny": 0.00745, "llama_tiny_gqa": 0.008933}


def _model(name):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model(name)).to(DEV).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, T0), generator=torch.Generator().manual_seed(1)).to(DEV)
    return model, idx


def _cached_error(model, idx, ref):
    """max |cached logits - ``ref``'s fp32 full forward| over the last prompt position and STEPS greedy steps."""
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
def test_int4_decode_routes_to_the_w4_kernel_and_back(name):
    from pytorch_distributed_training_example_amd.ops import linear as L
    model, idx = _model(name)
    tok = idx[:, 0].contiguous()
    with torch.no_grad():
        cache = model.new_cache(B, T0 + 4)
        model.prefill(idx, cache)
        before = model.decode_step(tok, cache)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.quantize_decode_weights()
        model.quantize_decode_weights("int4")  # replaces the e4m3 copies
        assert all(hasattr(m, "_w4") and not hasattr(m, "_w8") for m in model._decode_linears())
        after_sd = model.state_dict()
        assert list(after_sd) == list(sd) and all(torch.equal(after_sd[k], sd[k]) for k in sd)
        n4, n8 = L.SKINNY_STATS["w4_calls"], L.SKINNY_STATS["w8_calls"]
        cache.set_lens([T0] * B)
        quant = model.decode_step(tok, cache)
        assert L.SKINNY_STATS["w4_calls"] - n4 == 4 * model.cfg.n_layer + 1 and L.SKINNY_STATS["w8_calls"] == n8
        assert quant.shape == before.shape and not torch.equal(quant, before)
        model.transformer.h[0].attn.c_proj.weight.mul_(1.0)  # an in-place update: the int4 copy is stale
        cache.set_lens([T0] * B)
        with pytest.raises(RuntimeError, match="quantize_decode_weights"):
            model.decode_step(tok, cache)
        model.quantize_decode_weights()  # back to the default: no int4 copy stays behind
        assert all(hasattr(m, "_w8") and not hasattr(m, "_w4") for m in model._decode_linears())
        model.drop_decode_weights()
        cache.set_lens([T0] * B)
        n4 = L.SKINNY_STATS["w4_calls"]
        assert torch.equal(model.decode_step(tok, cache), before) and L.SKINNY_STATS["w4_calls"] == n4


@pytest.mark.parametrize("name", NAMES)
def test_w4_logits_are_as_close_to_their_fp32_forward_as_bf16_is(name):
    """Bound: twice the bf16 cached path's recorded figure; the kernel adds fp32 accumulation and one bf16 rounding,
    as the W8 kernel does."""
    from pytorch_distributed_training_example_amd.ops.linear import dequantize_groups_int4
    model, idx = _model(name)
    original = copy.deepcopy(model).float().cpu()
    model.quantize_decode_weights("int4")
    ref = copy.deepcopy(original)
    for mod, src in zip(ref._decode_linears(), model._decode_linears()):
        mod.weight.data.copy_(dequantize_groups_int4(src._w4[0], src._w4[1]))
    e_w4, e_fmt = _cached_error(model, idx, ref), _cached_error(model, idx, original)
    print(f"{name}: e_w4 = {e_w4:.4g} against the dequantised weights, ratio to the recorded bf16 figure "
          f"{e_w4 / PARENT_ERR[name]:.3f}; against the original weights (the format, not asserted) {e_fmt:.4g}")
    assert e_w4 <= 2 * PARENT_ERR[name], (e_w4, PARENT_ERR[name])
