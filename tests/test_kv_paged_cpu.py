"""PagedKVCache's host-side allocator, and the CPU reference path of the paged ops and of generate(paged=True)
against the contiguous cache."""
import pytest
import torch

from pytorch_distributed_training_example_amd.models import get_model
from pytorch_distributed_training_example_amd.ops.kv_cache import PagedKVCache


def _cache(n_pages=6, max_pages=3):
    cache = PagedKVCache(1, 3, 2, n_pages, max_pages, "cpu", torch.float32)
    for s in range(3):
        cache.admit(s)
    return cache


def test_allocator_reserve_free_and_bounds():
    cache = _cache()
    cache.reserve(70)  # two pages per slot: the pool is exhausted
    assert cache.free_pages == 0 and sorted(sum((cache.pages_of(s) for s in range(3)), [])) == list(range(6))
    assert torch.equal(cache.block_table[:, :2].sort(1).values, cache.block_table[:, :2]) and (cache.block_table[:, 2] == -1).all()
    cache.set_lens([5, 60, 70])
    assert cache.bounds == [5, 60, 70]
    cache.reserve(1)  # nobody crosses a page: nothing to do
    cache.advance(4)
    assert cache.bounds == [9, 64, 74] and cache.lens.tolist() == [9, 64, 74]
    cache.set_lens([9, 64, 127])
    before = (cache.block_table.clone(), cache.free_pages, cache.bounds)
    with pytest.raises(ValueError, match="0 free"):  # slot 2 needs a third page and the pool has none
        cache.reserve(2)
    assert torch.equal(cache.block_table, before[0]) and (cache.free_pages, cache.bounds) == before[1:]
    gone = cache.pages_of(1)
    cache.free(1)
    assert cache.free_pages == 2 and (cache.block_table[1] == -1).all() and not cache.is_active(1)
    assert cache.lens.tolist() == [9, 0, 127] and cache.active.tolist() == [1, 0, 1] and cache.bounds == [9, 0, 127]
    cache.reserve(2)  # now slot 2 gets one of the freed, uncleared pages
    assert cache.pages_of(2)[2] in gone and cache.free_pages == 1
    cache.advance(2)
    assert cache.lens.tolist() == [11, 0, 129]  # the freed slot does not move
    with pytest.raises(ValueError, match="max_pages_per_seq"):
        cache.reserve(64)
    cache.table_len = 130
    with pytest.raises(ValueError, match="rotary"):
        cache.reserve(2)
    with pytest.raises(ValueError, match="reserve"):  # a step whose pages were not reserved is refused before it runs
        cache.require(64)


@pytest.mark.parametrize("name", ["llama_tiny", "llama_tiny_gqa"])
def test_reference_path_generates_the_contiguous_tokens(name):
    torch.manual_seed(0)
    model = get_model(name, block_size=192).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (3, 70), generator=torch.Generator().manual_seed(1))
    want = model.generate(idx, 8, prompt_lens=(5, 60, 70))  # greedy; sequence 1 crosses key 64
    got = model.generate(idx, 8, prompt_lens=(5, 60, 70), paged=True)
    assert torch.equal(got, want)


def test_extend_on_a_paged_cache_raises():
    model = get_model("llama_tiny", block_size=192).eval()
    cache = model.new_paged_cache(2, 8)
    assert cache.max_pages == 3 and cache.table_len == 192
    idx = torch.randint(0, model.cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        cache.admit(0)
        with pytest.raises(ValueError, match="not admitted"):  # before the forward: nothing is written
            model.prefill(idx, cache)
        cache.admit(1)
        cache.reserve(6)
        model.prefill(idx, cache)
        cache.reserve(3)
        with pytest.raises(NotImplementedError, match="paged"):
            model.extend(idx[:, :3], cache)
