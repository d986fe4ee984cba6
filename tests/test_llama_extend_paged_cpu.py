"""``Llama.extend(..., slots=)`` on a paged cache, reference path (CPU, fp32): appends onto non-empty slots across
key 64 give the full forward's logits, a ragged append moves the named slots only, and a paged chunked prefill
generates what the contiguous one generates."""
import pytest
import torch

from pytorch_distributed_training_example_amd.models import get_model
from test_llama_generate_cpu import NAMES, _close

_FULL = {}


def _setup(name):
    """The model at block_size 192, 100 tokens for 3 sequences and the full forward's logits, once per preset."""
    if name not in _FULL:
        torch.manual_seed(0)
        model = get_model(name, block_size=192).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (3, 100), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            _FULL[name] = (model, idx, model(idx))
    return _FULL[name]


@pytest.mark.parametrize("name", NAMES)
def test_extend_on_named_slots_matches_the_full_forward(name):
    model, idx, full = _setup(name)
    with torch.no_grad():
        cache = model.new_paged_cache(3, 9)
        for s in range(3):
            cache.admit(s)
        cache.reserve(58)
        model.prefill(idx[:, :58], cache)
        cache.reserve(17, slots=[2, 0])  # 58 .. 74 crosses key 64: both slots take their second page
        got = model.extend(idx[[2, 0], 58:75], cache, slots=[2, 0])
        _close(got, full[[2, 0], 58:75], "17 tokens onto 58 in slots 2 and 0")
        assert cache.lens.tolist() == [75, 58, 75] and cache.bounds == [75, 58, 75] and len(cache.pages_of(1)) == 1
        # ragged: slots 0 and 2 keep 2 and 5 of 5 drafted rows; slot 1 is not named and does not move
        cache.reserve(5, slots=[0, 2])
        got = model.extend(idx[[0, 2], 75:80], cache, new_lens=(2, 5), last_only=True, slots=[0, 2])
        _close(got, torch.stack([full[0, 76], full[2, 79]]), "last valid rows of a ragged append")
        assert cache.lens.tolist() == [77, 58, 80] and cache.bounds == [80, 58, 80]
        cache.reserve(1)
        got = model.decode_step(torch.stack([idx[0, 77], idx[1, 58], idx[2, 80]]), cache)
        _close(got, torch.stack([full[0, 77], full[1, 58], full[2, 80]]), "the decode step after the appends")
        with pytest.raises(ValueError, match="chunked prefill"):  # Tn > 1 outside extend onto slots that hold something
            model.prefill(idx[:1, :4], cache, slots=[1])


@pytest.mark.parametrize("name", NAMES)
def test_paged_chunked_prefill_generates_the_contiguous_tokens(name):
    model, idx, _ = _setup(name)
    lens = (5, 60, 70)
    toks, want = model.generate(idx[:, :70], 6, prompt_lens=lens, return_logits=True, prefill_chunk=16)
    paged, got = model.generate(idx[:, :70], 6, prompt_lens=lens, return_logits=True, prefill_chunk=16, paged=True)
    _close(got, want, "ragged prompts in slices of 16 on a paged cache")
    assert torch.equal(paged, toks)


def test_slots_on_a_contiguous_cache_raises():
    model, idx, _ = _setup("llama_tiny")
    with torch.no_grad(), pytest.raises(ValueError, match="PagedKVCache"):
        model.extend(idx[:, :3], model.new_cache(3, 8), slots=[0, 1, 2])
