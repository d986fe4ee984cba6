"""``Llama.extend`` on the reference path (CPU, fp32): multi-token appends onto a non-empty cache give the
full forward's logits, a chunked prefill generates what the whole prefill generates, and the refusals."""
import pytest
import torch

# the models, their full forward (computed once for both files) and the tolerance of cached logits
from test_llama_generate_cpu import NAMES, _close, _setup


@pytest.mark.parametrize("name", NAMES)
def test_extend_matches_the_full_forward(name):
    model, idx, full = _setup(name)
    with torch.no_grad():
        cache = model.new_cache(3, 40)
        _close(model.extend(idx[:, :5], cache), full[:, :5], "extend onto an empty cache")
        _close(model.extend(idx[:, 5:22], cache), full[:, 5:22], "17 tokens onto 5")
        _close(model.extend(idx[:, 22:23], cache), full[:, 22:23], "one token through the decode path")
        assert cache.bound == 23 and cache.lens.tolist() == [23, 23, 23]
        # ragged: sequences take 3, 6 and 0 of the 6 rows; the next append overwrites the padding
        _close(model.extend(idx[:, 23:29], cache, new_lens=(3, 6, 0), last_only=True)[:2],
               torch.stack([full[0, 25], full[1, 28]]), "last valid rows of a ragged append")
        assert cache.lens.tolist() == [26, 29, 23] and cache.bound == 29
        nxt = torch.stack([idx[0, 26:30], idx[1, 29:33], idx[2, 23:27]])
        got = model.extend(nxt, cache)
        for b, p in enumerate((26, 29, 23)):
            _close(got[b], full[b, p:p + 4], f"sequence {b} after the ragged append")


@pytest.mark.parametrize("name", NAMES)
def test_chunked_prefill_generates_what_the_whole_prefill_generates(name):
    model, idx, _ = _setup(name)
    lens = (5, 17, 1)
    toks, want = model.generate(idx[:, :17], 6, prompt_lens=lens, return_logits=True)
    chunked, got = model.generate(idx[:, :17], 6, prompt_lens=lens, return_logits=True, prefill_chunk=4)
    _close(got, want, "ragged prompts in chunks of 4")
    assert torch.equal(chunked, toks)


def test_refusals():
    model, idx, _ = _setup("llama_tiny")
    with torch.no_grad():
        cache = model.new_cache(3, 8)
        model.extend(idx[:, :5], cache)
        with pytest.raises(ValueError, match="capacity"):
            model.extend(idx[:, 5:9], cache)
        long = model.new_cache(3, 80)
        model.extend(idx[:, :37], long)
        with pytest.raises(ValueError, match="rotary"):
            model.extend(idx[:, :28], long)  # 65 positions against the table's 64
        with pytest.raises(ValueError, match="new_lens"):
            model.extend(idx[:, :3], model.new_cache(3, 8), new_lens=(1, 4, 0))
