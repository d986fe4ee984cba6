"""Grouped-query attention in the Llama-style decoder off the GPU: ``llama_tiny_gqa`` against a reference written
here from the published formulas with ``repeat_kv`` under Hugging Face's key names (k_proj / v_proj of
``num_key_value_heads * 64`` rows), loaded through ``from_hf_state_dict(sd, n_kv_head=2)``; the configuration
and its state-dict shapes; and the ``--kv-heads`` flag."""
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_state_dict(L, H, Hkv, D, Fh, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * 0.05  # noqa: E731
    sd = {"model.embed_tokens.weight": r(V, D), "model.norm.weight": 1 + r(D), "lm_head.weight": r(V, D)}
    for i in range(L):
        p = f"model.layers.{i}."
        sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.o_proj.weight"] = r(D, D), r(D, D)
        sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"] = r(Hkv * 64, D), r(Hkv * 64, D)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = r(Fh, D), r(Fh, D)
        sd[p + "mlp.down_proj.weight"] = r(D, Fh)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = 1 + r(D), 1 + r(D)
    return sd


def _repeat_kv(x, n_rep):
    """HF's repeat_kv: [B, Hkv, T, dh] -> [B, Hkv * n_rep, T, dh], head h of the result is head h // n_rep."""
    B, Hkv, T, dh = x.shape
    return x[:, :, None].expand(B, Hkv, n_rep, T, dh).reshape(B, Hkv * n_rep, T, dh)


def _reference_logits(sd, idx, L, H, Hkv, eps=1e-5, base=10000.0):
    """Llama with grouped-query attention as published (RMSNorm, RoPE with rotate_half, repeat_kv, causal
    softmax attention, SwiGLU), in fp32."""
    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w

    def rotate_half(x):
        return torch.cat([-x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]], -1)

    B, T = idx.shape
    x = sd["model.embed_tokens.weight"][idx]
    D = x.shape[-1]
    dh = D // H
    inv_freq = 1.0 / (base ** (torch.arange(0, dh, 2, dtype=torch.float64) / dh))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv_freq[None, :]
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().float()[None, None], emb.sin().float()[None, None]  # [1, 1, T, dh]
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    for i in range(L):
        p = f"model.layers.{i}."
        hn = rms(x, sd[p + "input_layernorm.weight"])
        q = (hn @ sd[p + "self_attn.q_proj.weight"].t()).view(B, T, H, dh).transpose(1, 2)
        k, v = [(hn @ sd[p + f"self_attn.{n}_proj.weight"].t()).view(B, T, Hkv, dh).transpose(1, 2) for n in "kv"]
        q, k = q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin
        k, v = _repeat_kv(k, H // Hkv), _repeat_kv(v, H // Hkv)
        att = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        att = torch.softmax(att.masked_fill(~causal, float("-inf")), -1)
        x = x + (att @ v).transpose(1, 2).reshape(B, T, D) @ sd[p + "self_attn.o_proj.weight"].t()
        hn = rms(x, sd[p + "post_attention_layernorm.weight"])
        gate, up = hn @ sd[p + "mlp.gate_proj.weight"].t(), hn @ sd[p + "mlp.up_proj.weight"].t()
        x = x + (torch.nn.functional.silu(gate) * up) @ sd[p + "mlp.down_proj.weight"].t()
    return rms(x, sd["model.norm.weight"]) @ sd["lm_head.weight"].t()


def _sd_of(cfg, seed=0):
    return _hf_state_dict(cfg.n_layer, cfg.n_head, cfg.n_kv_head, cfg.n_embd, cfg.ffn, cfg.vocab_size, seed)


# ----------------------------------------------------------------------------- the model against a reference
@pytest.mark.parametrize("fused_addln", ["1", "0"])
def test_llama_tiny_gqa_matches_hf_style_reference(fused_addln, switch):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.llama import from_hf_state_dict
    switch("PDT_FUSED_ADDLN", fused_addln)
    model = get_model("llama_tiny_gqa").eval()
    cfg = model.cfg
    assert (cfg.n_head, cfg.n_kv_head, cfg.kv_heads) == (4, 2, 2)
    sd = _sd_of(cfg)
    ours = from_hf_state_dict(sd, n_kv_head=2)
    assert set(ours) == set(model.state_dict())
    model.load_state_dict(ours)
    idx = torch.randint(0, cfg.vocab_size, (2, 37), generator=torch.Generator().manual_seed(1))
    want = _reference_logits(sd, idx, cfg.n_layer, cfg.n_head, cfg.n_kv_head, cfg.eps, cfg.rope_base)
    with torch.no_grad():
        got = model(idx)
    assert got.shape == want.shape == (2, 37, cfg.vocab_size)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    model.train()
    got_t = model(idx)
    assert torch.equal(got_t.detach(), got)
    got_t.square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_llama_gqa_gradients_match_reference_autograd():
    """The hand-written backwards on the grouped layout (the conjugate rotation of H + Hkv heads of the packed
    gradient, the group sum of dK / dV) against autograd through the reference, fp32 on the CPU."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.llama import from_hf_state_dict
    model = get_model("llama_tiny_gqa")
    cfg = model.cfg
    sd = {k: v.requires_grad_() for k, v in _sd_of(cfg).items()}
    model.load_state_dict(from_hf_state_dict({k: v.detach() for k, v in sd.items()}, n_kv_head=2))
    idx = torch.randint(0, cfg.vocab_size, (2, 19), generator=torch.Generator().manual_seed(2))
    tgt = torch.randint(0, cfg.vocab_size, (2, 19), generator=torch.Generator().manual_seed(3))
    loss = model(idx, tgt)
    loss.backward()
    ref = torch.nn.functional.cross_entropy(
        _reference_logits(sd, idx, cfg.n_layer, cfg.n_head, cfg.n_kv_head).view(-1, cfg.vocab_size), tgt.view(-1))
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    want = from_hf_state_dict({k: v.grad for k, v in sd.items()}, n_kv_head=2)
    for name, p in model.named_parameters():
        assert float((p.grad - want[name]).abs().max()) <= 1e-4 * float(want[name].abs().max()) + 1e-9, name


# ----------------------------------------------------------------------------- configuration, state dict
def test_state_dict_shapes_and_default_is_multi_head():
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.llama import LlamaConfig
    gqa, mha = get_model("llama_tiny_gqa"), get_model("llama_tiny")
    assert LlamaConfig().n_kv_head is None and mha.cfg.n_kv_head is None and mha.cfg.kv_heads == 4
    assert list(gqa.state_dict()) == list(mha.state_dict())  # same keys
    for name, t in gqa.state_dict().items():
        want = ((4 + 2 * 2) * 64, 256) if name.endswith("attn.c_attn.weight") else tuple(mha.state_dict()[name].shape)
        assert tuple(t.shape) == want, name
    assert tuple(mha.state_dict()["transformer.h.0.attn.c_attn.weight"].shape) == (3 * 256, 256)
    # n_kv_head = n_head spelled out: the same shapes and the same init draws as the default
    torch.manual_seed(7)
    a = get_model("llama_tiny")
    torch.manual_seed(7)
    b = get_model("llama_tiny", n_kv_head=4)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert get_model("llama_tiny", n_kv_head=1).transformer.h[0].attn.c_attn.weight.shape == ((4 + 2) * 64, 256)


def test_n_kv_head_must_divide_n_head():
    from pytorch_distributed_training_example_amd.models import get_model
    for bad in (3, 0, 8):
        with pytest.raises(ValueError, match="n_kv_head"):
            get_model("llama_tiny", n_kv_head=bad)


def test_from_hf_state_dict_checks_the_kv_rows():
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.llama import from_hf_state_dict
    sd = _sd_of(get_model("llama_tiny_gqa").cfg)
    with pytest.raises(ValueError, match="grouped-query"):  # the default still refuses, and says what to pass
        from_hf_state_dict(sd)
    with pytest.raises(ValueError, match="n_kv_head"):
        from_hf_state_dict(sd)
    with pytest.raises(ValueError, match="n_kv_head"):
        from_hf_state_dict(sd, n_kv_head=1)
    with pytest.raises(ValueError, match="n_kv_head"):
        from_hf_state_dict(sd, n_kv_head=4)
    out = from_hf_state_dict(sd, n_kv_head=2)
    w = out["transformer.h.1.attn.c_attn.weight"]
    p = "model.layers.1.self_attn."
    assert torch.equal(w, torch.cat([sd[p + "q_proj.weight"], sd[p + "k_proj.weight"], sd[p + "v_proj.weight"]], 0))
    assert w.shape == (512, 256)


# ----------------------------------------------------------------------------- command line
def test_kv_heads_flag_parses_and_registered_name_has_defaults():
    from pytorch_distributed_training_example_amd import cli
    args = cli.build_parser().parse_args(["--model", "llama_medium", "--kv-heads", "4"])
    assert args.kv_heads == 4 and cli.build_parser().parse_args([]).kv_heads is None
    assert cli.is_token_model("llama_tiny_gqa") and cli.MODEL_DEFAULTS["llama_tiny_gqa"]["loss"] == "cross_entropy"
    assert cli.kv_heads_ok("llama_medium", 4) and cli.kv_heads_ok("llama_small", 4) and cli.kv_heads_ok("llama_tiny", 1)


@pytest.mark.parametrize("model,n", [("gpt2_tiny", 2), ("resnet50", 1), ("lenet", 4), ("llama_tiny", 3), ("llama_medium", 5),
                                     ("llama_small", 8), ("llama_tiny", 0), ("llama_tiny", -2), ("llama_tiny", 8)])
def test_kv_heads_is_refused_up_front(model, n):
    from pytorch_distributed_training_example_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["--model", model, "--kv-heads", str(n), "--no-cuda"])
    assert str(ei.value) == cli.kv_heads_msg(model, n) and "--kv-heads" in str(ei.value)


def test_train_cli_llama_tiny_kv_heads_two_steps_cpu(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--model", "llama_tiny", "--kv-heads", "1",
                        "--steps-per-epoch", "2", "--epochs", "1", "--batch-size", "4", "--seq-len", "32", "--no-cuda",
                        "--world-size", "1"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Train Epoch: 1" in r.stdout, r.stdout[-2000:]
