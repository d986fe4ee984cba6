"""KV-cache generation of the Llama decoder on the reference path (CPU, fp32): prefill + decode steps give
the full forward's logits, ragged prompts, greedy / seeded sampling, EOS masking, the refusals and the
``--sample-tokens`` command line."""
import os
import subprocess
import sys

import pytest
import torch

from pytorch_distributed_training_example_amd.models import get_model
from pytorch_distributed_training_example_amd.ops.kv_cache import KVCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["llama_tiny", "llama_tiny_gqa"]
TOL = 1e-5  # of max|want|: the bound tests/test_llama_cpu.py holds fp32 logits to

_FULL = {}


def _setup(name):
    """The model, 37 tokens for 3 sequences and the full forward's logits, once per preset."""
    if name not in _FULL:
        torch.manual_seed(0)
        model = get_model(name).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (3, 37), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            _FULL[name] = (model, idx, model(idx))
    return _FULL[name]


def _close(got, want, what):
    err, ref = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= TOL * ref, f"{what}: max error {err:.3g} > {TOL} x {ref:.3g}"


@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_steps_match_the_full_forward(name):
    model, idx, full = _setup(name)
    with torch.no_grad():
        cache = model.new_cache(3, 40)
        _close(model.prefill(idx[:, :17], cache), full[:, 16], "prefill")
        assert cache.bound == 17 and cache.lens.tolist() == [17, 17, 17]
        for t in range(17, 37):  # 20 steps fed the true next token
            _close(model.decode_step(idx[:, t], cache), full[:, t], f"decode step at position {t}")
        assert cache.bound == 37 and cache.lens.tolist() == [37, 37, 37]


@pytest.mark.parametrize("name", NAMES)
def test_ragged_batch_equals_each_sequence_alone(name):
    model, idx, _ = _setup(name)
    lens = (5, 17, 1)
    with torch.no_grad():
        cache = model.new_cache(3, 30)
        batch = [model.prefill(idx[:, :17], cache, prompt_lens=lens)]
        assert cache.lens.tolist() == list(lens) and cache.bound == 17
        nxt = torch.stack([idx[b, lens[b]:lens[b] + 6] for b in range(3)])  # each sequence's own continuation
        for t in range(6):
            batch.append(model.decode_step(nxt[:, t], cache))
        for b in range(3):
            alone = model.new_cache(1, 30)
            _close(batch[0][b:b + 1], model.prefill(idx[b:b + 1, :lens[b]], alone), f"sequence {b} prefill")
            for t in range(6):
                _close(batch[t + 1][b:b + 1], model.decode_step(nxt[b:b + 1, t], alone), f"sequence {b} step {t}")


@pytest.mark.parametrize("name", NAMES)
def test_generate_greedy_seeded_and_eos(name):
    model, idx, full = _setup(name)
    model.train()
    toks, logits = model.generate(idx[:, :9], 8, return_logits=True)
    assert model.training  # the mode is restored
    model.eval()
    assert toks.shape == (3, 8) and logits.shape == (3, 8, model.cfg.vocab_size)
    assert torch.equal(toks, logits.argmax(-1))
    _close(logits[:, 0], full[:, 8], "first generated position")
    with torch.no_grad():  # greedy generation is the full forward's argmax on the grown sequence
        grown = torch.cat([idx[:, :9], toks], 1)
        _close(logits, model(grown)[:, 8:-1], "generated positions")

    def sample(seed):
        g = torch.Generator().manual_seed(seed)
        return model.generate(idx[:, :9], 8, temperature=0.9, top_k=20, generator=g, return_logits=True)

    (a, la), (b, lb), (c, _) = sample(3), sample(3), sample(4)
    assert torch.equal(a, b) and torch.equal(la, lb) and not torch.equal(a, c)
    top20 = la.topk(20, dim=-1).indices
    assert bool((top20 == a[..., None]).any(-1).all())  # every draw is among the 20 likeliest

    eos = int(toks[1, 2])  # a token the greedy run emits: sequence 1 must be EOS from its first one on
    masked = model.generate(idx[:, :9], 8, eos_token=eos)
    for b in range(3):
        row, want = masked[b].tolist(), toks[b].tolist()
        first = want.index(eos) if eos in want else len(want)
        assert row[:first + 1] == want[:first + 1] and all(t == eos for t in row[first:])
    assert masked[1].tolist()[2:] == [eos] * 6


def test_refusals():
    model, idx, _ = _setup("llama_tiny")
    with pytest.raises(ValueError, match="block_size"):
        model.generate(idx[:, :37], 64 - 37 + 1)
    with torch.no_grad():
        cache = model.new_cache(3, 40)
        model.prefill(idx[:, :5], cache)
        with pytest.raises(ValueError, match="chunked prefill"):
            model.prefill(idx[:, 5:9], cache)
        full = model.new_cache(3, 6)
        model.prefill(idx[:, :6], full)
        with pytest.raises(ValueError, match="capacity"):
            model.decode_step(idx[:, 6], full)
        with pytest.raises(ValueError, match="does not fit"):
            model.decode_step(idx[:1, 6], cache)
        with pytest.raises(ValueError, match="prompt_lens"):
            model.prefill(idx[:, :5], model.new_cache(3, 8), prompt_lens=(1, 6, 2))
    with pytest.raises(RuntimeError, match="inference only"):
        model.prefill(idx[:, :5], model.new_cache(3, 40))  # gradients enabled, parameters require them


def test_cache_bound_is_kept_on_the_host():
    c = KVCache(2, 3, 2, 16, "cpu", torch.float32)
    assert c.k[0].shape == (3, 2, 16, 64) and c.k[0].is_contiguous() and c.lens.dtype == torch.int32
    c.advance(5)
    assert c.bound == 5 and c.lens.tolist() == [5, 5, 5]
    c.set_lens([1, 9, 4])
    assert c.bound == 9 and c.lens.tolist() == [1, 9, 4]
    c.require(7, table_len=16)
    with pytest.raises(ValueError, match="capacity"):
        c.require(8)
    with pytest.raises(ValueError, match="rotary"):
        c.require(7, table_len=15)
    with pytest.raises(ValueError):
        c.set_lens([1, 17, 4])
    c.reset()
    assert c.bound == 0 and c.lens.tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------- command line
def _train(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--no-cuda", "--world-size", "1"] + args,
                          capture_output=True, text=True, timeout=300, cwd=str(cwd),
                          env=dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1"))


def _sample_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("Sample: [")]
    assert len(lines) == 1, stdout[-2000:]
    ids = [int(t) for t in lines[0][len("Sample: ["):-1].split(",")]
    return ids


def test_cli_samples_after_training_and_from_a_resumed_checkpoint(tmp_path):
    base = ["--model", "llama_tiny", "--steps-per-epoch", "2", "--epochs", "1", "--batch-size", "4", "--seq-len", "32",
            "--checkpoint", "ck.pt", "--sample-tokens", "6", "--sample-prompt", "1,2,3"]
    r = _train(base, tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    ids = _sample_line(r.stdout)
    assert len(ids) == 6 and all(0 <= t < 512 for t in ids)
    # the finished checkpoint, resumed: no epoch left to train, the same weights give the same greedy sample
    r2 = _train(base + ["--resume"], tmp_path)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "resumed from ck.pt" in r2.stdout and "Train Epoch" not in r2.stdout
    assert _sample_line(r2.stdout) == ids


@pytest.mark.parametrize("model", ["gpt2_tiny", "resnet18"])
def test_cli_refuses_sampling_for_other_models(model):
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["--model", model, "--sample-tokens", "4", "--no-cuda"])
    assert "--sample-tokens" in str(ei.value) and model in str(ei.value)


def test_cli_refuses_a_sample_that_does_not_fit():
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit, match="block_size"):
        cli.main(["--model", "llama_tiny", "--sample-tokens", "64", "--no-cuda"])
    with pytest.raises(SystemExit, match="sample-prompt"):
        cli.main(["--model", "llama_tiny", "--sample-tokens", "4", "--sample-prompt", "a,b", "--no-cuda"])
