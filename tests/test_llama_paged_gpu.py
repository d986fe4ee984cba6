"""Llama generation on the paged KV cache (bf16, MI355X): as close to the fp32 forward as the bf16 full forward
is across a page boundary, a sequence joining on freed, uncleared pages without moving a bit of the others, and
a captured decode step replaying bit for bit with pages reserved between the replays."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["llama_tiny_gqa", "llama_tiny"]
LENS = (5, 60, 70)  # sequence 1 crosses key 64 while decoding
STEPS = 12

_SETUP = {}


def _setup(name):
    """bf16 model on the GPU, tokens, and the fp32 forward of the same (bf16-valued) weights: once per preset."""
    if name not in _SETUP:
        from pytorch_distributed_training_example_amd.models import get_model
        from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
        torch.manual_seed(0)
        model = to_bf16_mixed(get_model(name, block_size=192)).to(DEV).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (4, 96), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            want = copy.deepcopy(model).float().cpu()(idx)  # [4, 96, V] fp32, the reference path on the CPU
            full = model(idx.to(DEV)).float().cpu()
        _SETUP[name] = (model, idx.to(DEV), want, full)
    return _SETUP[name]


def _start(model, idx, n_pages=9):
    """Three admitted slots prefilled with sequences 0..2 at LENS (right-padded to 70). Returns (cache, logits)."""
    cache = model.new_paged_cache(3, n_pages)
    for s in range(3):
        cache.admit(s)
    cache.reserve(70)
    return cache, model.prefill(idx[:3, :70], cache, prompt_lens=LENS)


def _steps(model, idx, cache, rows, start, first, n):
    """n teacher-forced decode steps: slot s feeds sequence rows[s] from position start[s], step numbers from first."""
    out = []
    for i in range(first, first + n):
        cache.reserve(1)
        tok = torch.stack([idx[rows[s], start[s] + i] for s in range(3)])
        out.append(model.decode_step(tok, cache))
    return out


def _errors(got, want, full, b, pos):
    return (got.float().cpu() - want[b, pos]).abs().max().item(), (full[b, pos] - want[b, pos]).abs().max().item()


@pytest.mark.parametrize("name", NAMES)
def test_paged_path_is_as_accurate_as_the_full_forward(name):
    from pytorch_distributed_training_example_amd.ops import attention as A
    from pytorch_distributed_training_example_amd.ops import rope as R
    model, idx, want, full = _setup(name)
    a0, r0, d0 = A.PAGED_STATS["native_calls"], R.APPEND_PAGED_STATS["native_calls"], A.DECODE_STATS["native_calls"]
    with torch.no_grad():
        cache, first = _start(model, idx)
        got = torch.stack([first] + _steps(model, idx, cache, (0, 1, 2), LENS, 0, STEPS), 1)
    n_layer = model.cfg.n_layer
    assert R.APPEND_PAGED_STATS["native_calls"] - r0 == n_layer * (1 + STEPS)
    assert A.PAGED_STATS["native_calls"] - a0 == n_layer * STEPS and A.DECODE_STATS["native_calls"] == d0
    assert cache.lens.tolist() == [n + STEPS for n in LENS] and cache.bounds == [70 + STEPS] * 3
    e_paged = e_full = 0.0
    for b in range(3):
        e = _errors(got[b], want, full, b, torch.arange(LENS[b] - 1, LENS[b] + STEPS))
        e_paged, e_full = max(e_paged, e[0]), max(e_full, e[1])
    print(f"{name}: max_t e_paged = {e_paged:.4g}, max_t e_full = {e_full:.4g}, ratio {e_paged / e_full:.3f}")
    assert e_paged <= 2 * e_full, (e_paged, e_full)


@pytest.mark.parametrize("name", NAMES)
def test_a_sequence_joins_on_freed_pages_and_the_others_do_not_move(name):
    model, idx, want, full = _setup(name)
    with torch.no_grad():
        plain, _ = _start(model, idx)
        ref = _steps(model, idx, plain, (0, 1, 2), LENS, 0, 8)

        cache, _ = _start(model, idx, n_pages=6)  # two pages per slot: the newcomer can only land on freed ones
        got = _steps(model, idx, cache, (0, 1, 2), LENS, 0, 3)
        freed = cache.pages_of(1)
        cache.free(1)
        assert cache.free_pages == 2 and cache.lens.tolist()[1] == 0
        cache.admit(1)
        cache.reserve(62, slots=[1])  # sequence 3's prompt of 62 tokens joins in slot 1
        assert cache.pages_of(1) == freed[:1] and cache.free_pages == 1
        joined = [model.prefill(idx[3:4, :62], cache, slots=[1])[0]]
        # slot 1 now feeds sequence 3 from position 62 (its step counter goes on at 3) and takes the other
        # freed page when it crosses key 64
        more = _steps(model, idx, cache, (0, 3, 2), (LENS[0], 62 - 3, LENS[2]), 3, 5)
    for i, (a, b) in enumerate(zip(got + more, ref)):
        assert torch.equal(a[[0, 2]], b[[0, 2]]), f"step {i}: an untouched sequence's logits changed"
    joined = torch.stack(joined + [m[1] for m in more])
    e_new, e_full = _errors(joined, want, full, 3, torch.arange(61, 61 + 6))
    print(f"{name}: joined sequence e_paged = {e_new:.4g}, e_full = {e_full:.4g}")
    assert e_new <= 2 * e_full, (e_new, e_full)
    assert sorted(cache.pages_of(1)) == sorted(freed) and cache.free_pages == 0  # pages are conserved
    assert cache.lens.tolist() == [LENS[0] + 8, 67, LENS[2] + 8]


def _start_joined(model, idx):
    """_start, then slot 1 is freed and sequence 3 joins there with a 62-token prompt: one page, so its decode
    steps reach a new page at key 64. Slots feed sequences JROWS from positions JSTART."""
    cache, _ = _start(model, idx)
    cache.free(1)
    cache.admit(1)
    cache.reserve(62, slots=[1])
    model.prefill(idx[3:4, :62], cache, slots=[1])
    return cache


JROWS, JSTART = (0, 3, 2), (LENS[0], 62, LENS[2])


@pytest.mark.parametrize("name", NAMES)
def test_captured_paged_step_replays_bit_for_bit(name):
    model, idx, _, _ = _setup(name)
    toks = [torch.stack([idx[JROWS[s], JSTART[s] + i] for s in range(3)]) for i in range(STEPS)]
    bounds = (70, 62, 70)
    with torch.no_grad():
        want = _steps(model, idx, _start_joined(model, idx), JROWS, JSTART, 0, STEPS)

        cache = _start_joined(model, idx)
        start = cache.lens.clone()
        static_tok = toks[0].clone()
        cache.reserve(1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up: allocates the split scratch outside the capture
            model.decode_step(static_tok, cache)
        torch.cuda.current_stream().wait_stream(side)
        cache.set_lens(start, bound=bounds)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model.decode_step(static_tok, cache)
        cache.set_lens(start, bound=bounds)  # the capture moved the host bounds only: nothing ran
        table0 = cache.block_table.clone()
        assert len(cache.pages_of(1)) == 1
        for i, t in enumerate(toks):
            cache.reserve(1)  # between the replays: slot 1 gets its second page, and the table is uploaded, before step 2
            static_tok.copy_(t)
            graph.replay()
            cache.set_lens(cache.lens, bound=[b + i + 1 for b in bounds])  # a replay advances lens on the device only
            assert torch.equal(static_logits, want[i]), f"replay {i} differs from the eager step"
        torch.cuda.synchronize()
    assert len(cache.pages_of(1)) == 2 and not torch.equal(cache.block_table, table0)  # the replays saw a new table
    assert cache.lens.tolist() == [n + STEPS for n in JSTART]
