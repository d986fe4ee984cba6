"""KV-cache generation of the Llama decoder on the native path (bf16, MI355X): the cached path is as close
to the fp32 forward as today's bf16 full forward is, it really runs the new kernels, it is reproducible,
a captured decode step replays bit for bit, and PDT_DISABLE_NATIVE=1 goes through the reference."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["llama_tiny", "llama_tiny_gqa"]
LENS = (5, 17, 1)
STEPS = 20

_SETUP = {}


def _setup(name):
    """bf16 model on the GPU, tokens, and the fp32 forward of the same (bf16-valued) weights: once per preset."""
    if name not in _SETUP:
        from pytorch_distributed_training_example_amd.models import get_model
        from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
        torch.manual_seed(0)
        model = to_bf16_mixed(get_model(name)).to(DEV).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (3, 40), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            want = copy.deepcopy(model).float().cpu()(idx)  # [3, 40, V] fp32, the reference path on the CPU
        _SETUP[name] = (model, idx.to(DEV), want)
    return _SETUP[name]


def _teacher_forced(model, idx, cache=None):
    """Prefill the ragged prompts (right-padded to 17), then STEPS decode steps fed each sequence's true next
    token. Returns the logits [3, 1 + STEPS, V] (sequence b's entry i is position LENS[b] - 1 + i) and the cache."""
    cache = cache or model.new_cache(3, 40)
    out = [model.prefill(idx[:, :17], cache, prompt_lens=LENS)]
    for i in range(STEPS):
        tok = torch.stack([idx[b, LENS[b] + i] for b in range(3)])
        out.append(model.decode_step(tok, cache))
    return torch.stack(out, 1), cache


@pytest.mark.parametrize("name", NAMES)
def test_cached_path_is_as_accurate_as_the_full_forward(name):
    from pytorch_distributed_training_example_amd.ops import attention as A
    from pytorch_distributed_training_example_amd.ops import rope as R
    model, idx, want = _setup(name)
    n_layer = model.cfg.n_layer
    a0, r0 = A.DECODE_STATS["native_calls"], R.APPEND_STATS["native_calls"]
    with torch.no_grad():
        full = model(idx).float().cpu()
        got, cache = _teacher_forced(model, idx)
    got = got.float().cpu()
    # the decode path really launched the new kernels: one append per layer and call, one decode per layer and step
    assert R.APPEND_STATS["native_calls"] - r0 == n_layer * (1 + STEPS)
    assert A.DECODE_STATS["native_calls"] - a0 == n_layer * STEPS
    S, C = A.attention_decode_geo(3, model.cfg.kv_heads, 40, None, model.cfg.n_head // model.cfg.kv_heads)
    assert A.DECODE_STATS["geo"] == (S, C) and C % 64 == 0 and S * C >= 40
    assert cache.lens.tolist() == [n + STEPS for n in LENS]
    e_full = e_cached = 0.0
    for b in range(3):
        pos = torch.arange(LENS[b] - 1, LENS[b] + STEPS)
        e_full = max(e_full, (full[b, pos] - want[b, pos]).abs().max().item())
        e_cached = max(e_cached, (got[b] - want[b, pos]).abs().max().item())
    print(f"{name}: max_t e_cached = {e_cached:.4g}, max_t e_full = {e_full:.4g}, ratio {e_cached / e_full:.3f}")
    assert e_cached <= 2 * e_full, (e_cached, e_full)


@pytest.mark.parametrize("name", NAMES)
def test_generate_is_reproducible(name):
    model, idx, _ = _setup(name)

    def run(seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        return model.generate(idx[:, :17], 12, temperature=0.8, top_k=50, generator=g, prompt_lens=LENS,
                              return_logits=True)

    (a, la), (b, lb) = run(5), run(5)
    assert torch.equal(a, b) and torch.equal(la, lb)
    greedy, lg = model.generate(idx[:, :17], 12, prompt_lens=LENS, return_logits=True)
    assert torch.equal(greedy, lg.argmax(-1)) and greedy.is_cuda


@pytest.mark.parametrize("name", NAMES)
def test_captured_decode_step_replays_bit_for_bit(name):
    model, idx, _ = _setup(name)
    toks = [torch.stack([idx[b, LENS[b] + i] for b in range(3)]) for i in range(12)]
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
        with torch.cuda.stream(side):  # warm-up: allocates the split scratch outside the capture
            model.decode_step(static_tok, cache)
        torch.cuda.current_stream().wait_stream(side)
        cache.set_lens(start, bound=17)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_logits = model.decode_step(static_tok, cache)
        # a replay advances lens on the device only; the host bound is the replaying caller's to keep
        cache.set_lens(cache.lens, bound=17 + 12)
        for i, t in enumerate(toks):
            static_tok.copy_(t)
            graph.replay()
            assert torch.equal(static_logits, want[i]), f"replay {i} differs from the eager step"
        torch.cuda.synchronize()
    assert torch.equal(cache.lens, eager.lens) and cache.lens.tolist() == [n + 12 for n in LENS]


def test_disable_native_generates_through_the_reference(switch):
    from pytorch_distributed_training_example_amd.ops import attention as A
    from pytorch_distributed_training_example_amd.ops import rope as R
    model, idx, _ = _setup("llama_tiny_gqa")
    native_toks, native_logits = model.generate(idx[:, :17], 6, prompt_lens=LENS, return_logits=True)
    switch("PDT_DISABLE_NATIVE", "1")
    a0, r0 = A.DECODE_STATS["native_calls"], R.APPEND_STATS["native_calls"]
    toks, logits = model.generate(idx[:, :17], 6, prompt_lens=LENS, return_logits=True)
    assert (A.DECODE_STATS["native_calls"], R.APPEND_STATS["native_calls"]) == (a0, r0)
    assert torch.equal(toks, logits.argmax(-1))
    # the same model on the other path: bf16 roundings apart (first step: no divergence of the sequences yet).
    # Each path rounds to bf16 (2^-8 = 0.4 % of a value) at about six points per layer of this two-layer model,
    # so either is within ~2.5 % of the largest logit from the exact result and the two within 5 % of each other.
    err = (logits[:, 0].float() - native_logits[:, 0].float()).abs().max().item()
    assert err <= 0.05 * native_logits[:, 0].float().abs().max().item(), err
