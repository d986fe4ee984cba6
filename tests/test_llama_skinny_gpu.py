"""The Llama decoder's decode-time Linears on the skinny GEMM (``PDT_DECODE_GEMM=1``; bf16, MI355X): the cached
path stays as close to the fp32 forward as the bf16 full forward is, every Linear of a step really runs the
kernel, a captured step replays bit for bit, and with the switch at its default nothing launches it."""
import pytest
import torch

from test_llama_generate_gpu import LENS, NAMES, STEPS, _setup, _teacher_forced

pytestmark = pytest.mark.gpu


def _errors(got, full, want, first, count):
    e_full = e_cached = 0.0
    for b in range(3):
        pos = torch.arange(first[b], first[b] + count)
        e_full = max(e_full, (full[b, pos] - want[b, pos]).abs().max().item())
        e_cached = max(e_cached, (got[b] - want[b, pos]).abs().max().item())
    return e_cached, e_full


@pytest.mark.parametrize("name", NAMES)
def test_decode_and_extend_on_the_skinny_gemm(name, switch):
    from pytorch_distributed_training_example_amd.ops import linear as L
    model, idx, want = _setup(name)
    per_call = 4 * model.cfg.n_layer + 1
    with torch.no_grad():
        full = model(idx).float().cpu()  # 120 rows: not the skinny path
        n0 = L.SKINNY_STATS["native_calls"]
        _teacher_forced(model, idx)
        assert L.SKINNY_STATS["native_calls"] == n0  # the default: off
        switch("PDT_DECODE_GEMM", "1")
        got, cache = _teacher_forced(model, idx)
        # the prefill runs 51 rows through the blocks and its 3 last rows through the head; every step 3 rows
        assert L.SKINNY_STATS["native_calls"] - n0 == per_call * (1 + STEPS)
        e_cached, e_full = _errors(got.float().cpu(), full, want, [n - 1 for n in LENS], 1 + STEPS)
        print(f"{name}: decode e_cached = {e_cached:.4g}, e_full = {e_full:.4g}")
        assert e_cached <= 2 * e_full, (e_cached, e_full)

        cache = model.new_cache(3, 40)
        model.prefill(idx[:, :17], cache, prompt_lens=LENS)
        n1 = L.SKINNY_STATS["native_calls"]
        ext = model.extend(torch.stack([idx[b, LENS[b]:LENS[b] + 6] for b in range(3)]), cache)  # 18 rows
        assert L.SKINNY_STATS["native_calls"] - n1 == per_call and L.SKINNY_STATS["geo"][2] == 2
        e_cached, e_full = _errors(ext.float().cpu(), full, want, list(LENS), 6)
        print(f"{name}: extend e_cached = {e_cached:.4g}, e_full = {e_full:.4g}")
        assert e_cached <= 2 * e_full, (e_cached, e_full)


@pytest.mark.parametrize("name", NAMES)
def test_captured_decode_step_on_the_skinny_gemm_replays_bit_for_bit(name, switch):
    switch("PDT_DECODE_GEMM", "1")
    model, idx, _ = _setup(name)
    toks = [torch.stack([idx[b, LENS[b] + i] for b in range(3)]) for i in range(4)]
    with torch.no_grad():
        eager = model.new_cache(3, 40)
        model.prefill(idx[:, :17], eager, prompt_lens=LENS)
        want = [model.decode_step(t, eager).clone() for t in toks]
        cache = model.new_cache(3, 40)
        model.prefill(idx[:, :17], cache, prompt_lens=LENS)
        start = cache.lens.clone()
        static_tok = toks[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.decode_step(static_tok, cache)
        torch.cuda.current_stream().wait_stream(side)
        cache.set_lens(start, bound=17)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model.decode_step(static_tok, cache)
        cache.set_lens(cache.lens, bound=17 + 4)
        for i, t in enumerate(toks):
            static_tok.copy_(t)
            graph.replay()
            assert torch.equal(static_logits, want[i]), f"replay {i} differs from the eager step"
        torch.cuda.synchronize()
