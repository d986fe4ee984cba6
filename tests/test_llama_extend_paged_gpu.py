"""``Llama.extend(..., slots=)`` on the paged KV cache (bf16, MI355X): a long prompt joins a running batch in
slices without moving a bit of the other slots, and a ragged verification step lands where the fp32 forward is."""
import pytest
import torch

from test_llama_paged_gpu import LENS, NAMES, _errors, _setup, _start

pytestmark = pytest.mark.gpu
PROMPT, SLICE = 70, 16  # sequence 3 joins in slot 1: slices of 16, the last of 6, across key 64


def _step(model, idx, cache, i, pos1, row1=3):
    """Decode step i of slots 0 and 2 (sequences 0 and 2 from LENS); slot 1 feeds sequence row1's token at pos1."""
    cache.reserve(1)
    return model.decode_step(torch.stack([idx[0, LENS[0] + i], idx[row1, pos1], idx[2, LENS[2] + i]]), cache)


@pytest.mark.parametrize("name", NAMES)
def test_a_prompt_joins_in_slices_and_drafts_are_verified(name):
    from pytorch_distributed_training_example_amd.ops import attention as A
    model, idx, want, full = _setup(name)
    n_slices = -(-PROMPT // SLICE)
    with torch.no_grad():
        plain, _ = _start(model, idx)  # the run without the joiner: slot 1 goes on decoding sequence 1
        ref = [_step(model, idx, plain, i, LENS[1] + i, row1=1) for i in range(2 + n_slices + 6)]

        cache, _ = _start(model, idx)
        got = [_step(model, idx, cache, i, LENS[1] + i, row1=1) for i in range(2)]
        cache.free(1)
        cache.admit(1)
        p0, e0 = A.EXTEND_PAGED_STATS["native_calls"], A.EXTEND_STATS["native_calls"]
        for s in range(0, PROMPT, SLICE):
            end = min(s + SLICE, PROMPT)
            cache.reserve(end - s, slots=[1])  # the slice's pages only
            joined = [model.extend(idx[3:4, s:end], cache, last_only=True, slots=[1])[0]]
            assert cache.lens.tolist()[1] == end and cache.bounds[1] == end
            # every slot decodes between the slices; the joiner's row is rolled back and the next slice overwrites it
            got.append(_step(model, idx, cache, len(got), end))
            cache.set_lens([end], slots=[1])
        assert A.EXTEND_PAGED_STATS["native_calls"] - p0 == model.cfg.n_layer * n_slices
        for i in range(6):  # the joiner decodes on: the step above stored its token at PROMPT, rolled back
            got.append(_step(model, idx, cache, len(got), PROMPT + i))
            joined.append(got[-1][1])
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a[[0, 2]], b[[0, 2]]), f"step {i}: an untouched slot's logits changed"
    e_new, e_full = _errors(torch.stack(joined), want, full, 3, torch.arange(PROMPT - 1, PROMPT + 6))
    print(f"{name}: joined in slices e_paged = {e_new:.4g}, e_full = {e_full:.4g}, ratio {e_new / e_full:.3f}")
    assert e_new <= 2 * e_full, (e_new, e_full)

    # a ragged verification step: 5 drafted (here: the true) tokens on slots 0 and 2, of which 2 and 5 are kept
    pos = [LENS[0] + len(got), PROMPT + 6, LENS[2] + len(got)]
    assert cache.lens.tolist() == pos
    bounds = cache.bounds
    with torch.no_grad():
        cache.reserve(5, slots=[0, 2])
        ver = model.extend(torch.stack([idx[0, pos[0]:pos[0] + 5], idx[2, pos[2]:pos[2] + 5]]), cache,
                           new_lens=(2, 5), slots=[0, 2])
        pos = [pos[0] + 2, pos[1], pos[2] + 5]
        assert cache.lens.tolist() == pos and cache.bounds == [bounds[0] + 5, bounds[1], bounds[2] + 5]
        cache.reserve(1)
        nxt = model.decode_step(torch.stack([idx[r, p] for r, p in zip((0, 3, 2), pos)]), cache)
    assert A.EXTEND_PAGED_STATS["native_calls"] - p0 == model.cfg.n_layer * (n_slices + 1)
    assert A.EXTEND_STATS["native_calls"] == e0
    e_new = e_full = 0.0
    for b, r in ((0, 0), (1, 2)):  # the verified rows, then the step after the rollback, for sequences 0 and 2
        kept = (2, 5)[b]
        for e in (_errors(ver[b, :kept], want, full, r, torch.arange(pos[r] - kept, pos[r])),
                  _errors(nxt[r], want, full, r, pos[r])):
            e_new, e_full = max(e_new, e[0]), max(e_full, e[1])
    print(f"{name}: ragged verification e_paged = {e_new:.4g}, e_full = {e_full:.4g}, ratio {e_new / e_full:.3f}")
    assert e_new <= 2 * e_full, (e_new, e_full)
