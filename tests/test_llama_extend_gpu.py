"""``Llama.extend`` on the native path (bf16, MI355X): multi-token appends onto a non-empty cache are as close
to the fp32 forward as the bf16 full forward is and run the append kernel, rejected drafts leave no trace
after a rollback, and a captured extend replays bit for bit."""
import pytest
import torch

# the bf16 models, their tokens and the fp32 reference logits, computed once for both files
from test_llama_generate_gpu import DEV, LENS, NAMES, _setup

pytestmark = pytest.mark.gpu


def _next(idx, start, n):
    """Each sequence's own n tokens from its position start[b] on: [3, n]."""
    return torch.stack([idx[b, start[b]:start[b] + n] for b in range(3)])


@pytest.mark.parametrize("name", NAMES)
def test_extend_is_as_accurate_as_the_full_forward(name):
    from pytorch_distributed_training_example_amd.ops import attention as A
    model, idx, want = _setup(name)
    n_layer, nl = model.cfg.n_layer, (3, 6, 1)
    e0, d0 = A.EXTEND_STATS["native_calls"], A.DECODE_STATS["native_calls"]
    with torch.no_grad():
        full = model(idx).float().cpu()
        cache = model.new_cache(3, 40)
        got = [(model.prefill(idx[:, :17], cache, prompt_lens=LENS)[:, None], [n - 1 for n in LENS], (1, 1, 1))]
        p1 = list(LENS)
        got.append((model.extend(_next(idx, p1, 6), cache), p1, (6, 6, 6)))
        assert A.EXTEND_STATS["native_calls"] - e0 == n_layer
        p2 = [p + 6 for p in p1]
        got.append((model.extend(_next(idx, p2, 6), cache, new_lens=nl), p2, nl))
        p3 = [p + n for p, n in zip(p2, nl)]
        got.append((model.decode_step(_next(idx, p3, 1)[:, 0], cache)[:, None], p3, (1, 1, 1)))
    assert A.EXTEND_STATS["native_calls"] - e0 == 2 * n_layer and A.DECODE_STATS["native_calls"] - d0 == n_layer
    assert len(A.EXTEND_STATS["geo"]) == 4 and cache.lens.tolist() == [p + 1 for p in p3]
    e_full = e_cached = 0.0
    for logits, pos, valid in got:
        logits = logits.float().cpu()
        for b in range(3):
            rows = slice(pos[b], pos[b] + valid[b])
            e_full = max(e_full, (full[b, rows] - want[b, rows]).abs().max().item())
            e_cached = max(e_cached, (logits[b, :valid[b]] - want[b, rows]).abs().max().item())
    print(f"{name}: max e_cached = {e_cached:.4g}, max e_full = {e_full:.4g}, ratio {e_cached / e_full:.3f}")
    assert e_cached <= 2 * e_full, (e_cached, e_full)


@pytest.mark.parametrize("name", NAMES)
def test_rollback_leaves_no_trace_of_the_rejected_drafts(name):
    """Six drafted tokens of which two are accepted, then the next four, against a cache that never saw the
    rejected four (the same calls with other tokens in their place and new_lens = 2)."""
    model, idx, _ = _setup(name)
    accepted, nxt = _next(idx, LENS, 2), _next(idx, [n + 2 for n in LENS], 4)
    with torch.no_grad():
        a = model.new_cache(3, 40)
        model.prefill(idx[:, :17], a, prompt_lens=LENS)
        start = a.lens.clone()
        drafted = model.extend(torch.cat([accepted, idx[:, 30:34]], 1), a)
        a.set_lens(start + 2)  # the present bound, 23, holds
        got = model.extend(nxt, a)
        b = model.new_cache(3, 40)
        model.prefill(idx[:, :17], b, prompt_lens=LENS)
        first = model.extend(torch.cat([accepted, idx[:, 34:38]], 1), b, new_lens=torch.full((3,), 2, device=DEV))
        want = model.extend(nxt, b)
    assert torch.equal(drafted[:, :2], first[:, :2]) and torch.equal(got, want)
    assert torch.equal(a.lens, b.lens) and a.lens.tolist() == [n + 6 for n in LENS]


@pytest.mark.parametrize("name", NAMES)
def test_captured_extend_replays_bit_for_bit(name):
    model, idx, _ = _setup(name)
    chunks = [_next(idx, [n + 4 * i for n in LENS], 4) for i in range(2)]
    with torch.no_grad():
        eager = model.new_cache(3, 40)
        model.prefill(idx[:, :17], eager, prompt_lens=LENS)
        want = [model.extend(c, eager).clone() for c in chunks]

        cache = model.new_cache(3, 40)
        model.prefill(idx[:, :17], cache, prompt_lens=LENS)
        start = cache.lens.clone()
        static_tok = chunks[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up outside the capture
            model.extend(static_tok, cache)
        torch.cuda.current_stream().wait_stream(side)
        cache.set_lens(start, bound=17)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model.extend(static_tok, cache)
        cache.set_lens(cache.lens, bound=17 + 8)  # replays advance lens on the device only
        for i, c in enumerate(chunks):
            static_tok.copy_(c)
            graph.replay()
            assert torch.equal(static_logits, want[i]), f"replay {i} differs from the eager call"
        torch.cuda.synchronize()
    assert torch.equal(cache.lens, eager.lens) and cache.lens.tolist() == [n + 8 for n in LENS]
