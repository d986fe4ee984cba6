"""Weight-only e4m3 decoding of the Llama decoder (Llama.quantize_decode_weights, MI355X): the decode-time Linears
really run the W8A16 skinny GEMM, the call leaves state_dict() alone, stale bytes are refused, dropping the
quantised weights restores today's bits, and the logits are as close to the fp32 forward of the dequantised
weights as the bf16 cached path is to the fp32 forward of its own."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["llama_tiny", "llama_tiny_gqa"]
B, T0, STEPS = 4, 12, 8
# Worst |logit error| of the bf16 cached path (prefill + 8 greedy decode steps, these prompts and seeds) against the
# fp32 forward of its own weights, measured on the parent commit's code path (profiles/r22/llama_w8_numerics.txt)
PARENT_ERR = {"llama_tiny": 0.00745, "llama_tiny_gqa": 0.008933}


def _model(name):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model(name)).to(DEV).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (B, T0), generator=torch.Generator().manual_seed(1)).to(DEV)
    return model, idx


def _greedy(model, idx):
    """prefill + STEPS greedy decode steps: (logits [B, 1 + STEPS, V], the sequences [B, T0 + STEPS])."""
    cache = model.new_cache(B, T0 + STEPS + 1)
    out, seq = [model.prefill(idx, cache)], idx
    for _ in range(STEPS):
        tok = out[-1].argmax(-1)
        seq = torch.cat([seq, tok[:, None]], 1)
        out.append(model.decode_step(tok, cache))
    return torch.stack(out, 1), seq


def _cached_error(model, idx, dequantised):
    """max |cached logits - fp32 full forward| over the last prompt position and the STEPS decoded ones; the fp32
    model holds the dequantised e4m3 weights when ``dequantised``."""
    ref = copy.deepcopy(model).drop_decode_weights().float().cpu()  # the reference path on the CPU
    if dequantised:
        for mod, src in zip(ref._decode_linears(), model._decode_linears()):
            mod.weight.data.copy_(src._w8[0].float() * src._w8[1][:, None])
    with torch.no_grad():
        got, seq = _greedy(model, idx)
        want = ref(seq.cpu())[:, T0 - 1:]
    return (got.float().cpu() - want).abs().max().item()


@pytest.mark.parametrize("name", NAMES)
def test_quantised_decode_routes_to_the_w8_kernel_and_back(name):
    from pytorch_distributed_training_example_amd.ops import linear as L
    model, idx = _model(name)
    tok = idx[:, 0].contiguous()
    with torch.no_grad():
        cache = model.new_cache(B, T0 + 4)
        model.prefill(idx, cache)
        n0 = L.SKINNY_STATS["w8_calls"]
        before = model.decode_step(tok, cache)
        assert L.SKINNY_STATS["w8_calls"] == n0  # no call, no w8 kernel
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.quantize_decode_weights()
        after_sd = model.state_dict()
        assert list(after_sd) == list(sd) and all(torch.equal(after_sd[k], sd[k]) for k in sd)
        cache.set_lens([T0] * B)
        quant = model.decode_step(tok, cache)
        assert L.SKINNY_STATS["w8_calls"] - n0 == 4 * model.cfg.n_layer + 1
        assert quant.shape == before.shape and not torch.equal(quant, before)
        model.transformer.h[0].attn.c_proj.weight.mul_(1.0)  # an in-place update: the e4m3 copy is stale
        cache.set_lens([T0] * B)
        with pytest.raises(RuntimeError, match="quantize_decode_weights"):
            model.decode_step(tok, cache)
        model.drop_decode_weights()
        cache.set_lens([T0] * B)
        n1 = L.SKINNY_STATS["w8_calls"]
        assert torch.equal(model.decode_step(tok, cache), before) and L.SKINNY_STATS["w8_calls"] == n1


@pytest.mark.parametrize("name", NAMES)
def test_w8_logits_are_as_close_to_their_fp32_forward_as_bf16_is(name):
    """Measured on the MI355X: the bf16 cached path 0.00745 (llama_tiny) / 0.008933 (llama_tiny_gqa) from its own
    fp32 forward; the quantised path 0.007399 / 0.007877 from the fp32 forward of the dequantised weights, 0.99x /
    0.88x of the bf16 figure. Bound: twice the bf16 path's figure."""
    model, idx = _model(name)
    e_bf16 = _cached_error(model, idx, False)
    model.quantize_decode_weights()
    e_w8 = _cached_error(model, idx, True)
    print(f"{name}: e_bf16 = {e_bf16:.4g} (recorded {PARENT_ERR[name]:.4g}), e_w8 = {e_w8:.4g}, "
          f"ratio to the recorded {e_w8 / PARENT_ERR[name]:.3f}")
    assert e_w8 <= 2 * PARENT_ERR[name], (e_w8, PARENT_ERR[name])
