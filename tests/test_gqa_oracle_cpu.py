"""The grouped-query oracle (tests/gqa_oracle.py) on the CPU, before any GPU runs:
  * an emulation of the GQA kernels' rounding points (P and dS rounded to bf16 per query head, dK / dV
    accumulated in fp32 over the group's heads and rounded once) stays inside the group-summed envelopes
    with ratio < 2, the analytic ceiling (the GPU tests allow ATTN_C = 3);
  * planted bugs (a wrong head map, a query head left out of a group's sum, dK of the first head only, a
    RoPE launch that skips the last K head or touches V) are rejected on inputs where the clean emulation passes;
  * the CPU path of ``attention_qkv(..., kv_heads=)`` and ``rope_qkv_(..., kv_heads=)`` equals the explicit
    expand-then-multi-head computation, and ``kv_heads=heads`` is the call without the argument, bit for bit."""
import functools

import pytest
import torch

import gqa_oracle as go
import oracle_envelope as oe

SCALE = 0.125


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


@functools.lru_cache(maxsize=None)
def _inputs(H, Hkv, T, amp, seed=1):
    g = torch.Generator().manual_seed(seed + 100 * H + 10 * Hkv)
    r = lambda h, a: _bf(torch.randn(2, h, T, 64, generator=g, dtype=torch.float64) * a).float()  # noqa: E731
    return r(H, amp), r(Hkv, amp), r(Hkv, 1.0), r(H, 1.0)


def emulate_gqa(q, k, v, do, causal, scale=SCALE, mut=None):
    """fp32 grouped-query attention rounding where the kernels round: per query head P -> bf16 before P V
    and P^T dO, dS -> bf16 before dS K and dS^T Q; O and dQ -> bf16 per head; dK and dV summed in fp32 over
    the group's heads and rounded to bf16 once. ``mut`` plants one bug."""
    H, Hkv, T = q.shape[1], k.shape[1], q.shape[2]
    G = H // Hkv
    kv_of = (lambda h: h % Hkv) if mut == "head_map_mod" else (lambda h: h // G)
    allowed = torch.ones(T, T, dtype=torch.bool)
    if causal:
        allowed = allowed.tril()
    O, LSE, dQ = [], [], []
    dK, dV = torch.zeros_like(k), torch.zeros_like(v)
    for h in range(H):
        j = kv_of(h)
        qh, kh, vh, doh = q[:, h], k[:, j], v[:, j], do[:, h]
        S = ((qh @ kh.transpose(-1, -2)) * scale).masked_fill(~allowed, float("-inf"))
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        Oh = _bf(_bf(P) @ vh)
        dS = P * (doh @ vh.transpose(-1, -2) - (doh * Oh).sum(-1, keepdim=True))
        O.append(Oh), LSE.append(lse), dQ.append(_bf(_bf(dS) @ kh * scale))
        last, first = h % G == G - 1, h % G == 0
        if not (mut == "dk_skip_last_head" and last):
            if not (mut == "dk_first_head_only" and not first):
                dK[:, j] += _bf(dS).transpose(-1, -2) @ qh * scale
        dV[:, j] += _bf(P).transpose(-1, -2) @ doh
    return {"O": torch.stack(O, 1), "LSE": torch.stack(LSE, 1), "dQ": torch.stack(dQ, 1), "dK": _bf(dK), "dV": _bf(dV)}


def _failed(got, ref, env, c=2.0):
    bad = set()
    for name in ("O", "dQ", "dK", "dV"):
        try:
            oe.assert_within(got[name], ref[name], env[name], c, name=name)
        except AssertionError:
            bad.add(name)
    try:
        oe.assert_abs(got["LSE"], ref["LSE"], oe.LSE_TOL_PEAKED, name="LSE")
    except AssertionError:
        bad.add("LSE")
    return bad


# ----------------------------------------------------------------------------- (a) the emulation fits
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (6, 2)])
@pytest.mark.parametrize("T,amp", [(65, 0.5), (129, 0.5), (129, 4.0)])
def test_emulation_within_group_summed_envelopes(H, Hkv, T, amp, causal):
    q, k, v, do = _inputs(H, Hkv, T, amp)
    ref, env = go.gqa_attention_oracle(q, k, v, do, causal=causal, scale=SCALE)
    assert ref["dK"].shape == ref["dV"].shape == env["dK"].shape == k.shape and ref["dQ"].shape == q.shape
    assert not _failed(emulate_gqa(q, k, v, do, causal), ref, env, c=2.0)


def test_oracle_matches_float64_autograd_through_repeat_interleave():
    q, k, v, do = (t.double() for t in _inputs(6, 2, 37, 1.0))
    q, k, v = q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    S = (q @ k.repeat_interleave(3, 1).transpose(-1, -2)) * 0.2
    S = S.masked_fill(~torch.ones(37, 37, dtype=torch.bool).tril(), float("-inf"))
    O = torch.softmax(S, -1) @ v.repeat_interleave(3, 1)
    dq, dk, dv = torch.autograd.grad(O, (q, k, v), do)
    ref, _ = go.gqa_attention_oracle(q.detach(), k.detach(), v.detach(), do, causal=True, scale=0.2)
    for a, b in ((ref["O"], O.detach()), (ref["dQ"], dq), (ref["dK"], dk), (ref["dV"], dv)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------- (b) planted bugs
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("mut,must_fail", [("head_map_mod", {"O", "dQ", "dK", "dV"}), ("dk_skip_last_head", {"dK"}),
                                           ("dk_first_head_only", {"dK"})])
def test_planted_attention_bugs_are_rejected(mut, must_fail, causal):
    q, k, v, do = _inputs(4, 2, 65, 0.5)
    ref, env = go.gqa_attention_oracle(q, k, v, do, causal=causal, scale=SCALE)
    assert not _failed(emulate_gqa(q, k, v, do, causal), ref, env)
    bad = _failed(emulate_gqa(q, k, v, do, causal, mut=mut), ref, env, c=oe.ATTN_C)
    assert must_fail <= bad, (mut, bad)
    if mut != "head_map_mod":  # dV is still summed over the whole group: only dK may fail
        assert bad == {"dK"}, bad


def emulate_rope(qkv, cos, sin, H, Hkv, conj=False, mut=None):
    """fp32 rotation of the H + Hkv leading heads, one rounding to bf16. ``mut``: skip_last_k (the last K head
    is left alone), rotate_v0 (V head 0 is rotated too)."""
    B, T, C = qkv.shape
    X = qkv.float().view(B, T, H + 2 * Hkv, 64).clone()
    R = H + Hkv + {"skip_last_k": -1, "rotate_v0": 1}.get(mut, 0)
    c, s = cos[:T].view(1, T, 1, 32), sin[:T].view(1, T, 1, 32) * (-1.0 if conj else 1.0)
    a, b = X[:, :, :R, :32].clone(), X[:, :, :R, 32:].clone()
    X[:, :, :R, :32], X[:, :, :R, 32:] = a * c - b * s, b * c + a * s
    return X.view(B, T, C).to(torch.bfloat16)


@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (12, 4)])
def test_rope_emulation_within_bounds_and_planted_bugs_rejected(H, Hkv):
    from pytorch_distributed_training_example_amd.ops.rope import rope_table
    T = 65
    qkv = go.gqa_rope_inputs(2, T, H, Hkv)
    cos, sin = rope_table(T + 3)
    for conj in (False, True):
        ref, env = go.gqa_rope_oracle(qkv, cos, sin, H, Hkv, conj)
        got = emulate_rope(qkv, cos, sin, H, Hkv, conj)
        oe.assert_within(got, ref, env, go.ROPE_C, go.FLOOR, name=f"rope conj={conj}")
        for mut in ("skip_last_k", "rotate_v0"):
            with pytest.raises(AssertionError):
                oe.assert_within(emulate_rope(qkv, cos, sin, H, Hkv, conj, mut=mut), ref, env, go.ROPE_C, go.FLOOR)
    back = emulate_rope(emulate_rope(qkv, cos, sin, H, Hkv), cos, sin, H, Hkv, conj=True)
    oe.assert_within(back, qkv.double(), go.gqa_rope_roundtrip_envelope(qkv, cos, sin, H, Hkv), 1.0, go.FLOOR, name="roundtrip")


def test_gqa_rope_oracle_is_rope_oracle_at_equal_head_counts():
    import llama_oracle as lo
    from pytorch_distributed_training_example_amd.ops.rope import rope_table
    qkv = lo.rope_inputs(2, 9, 4)
    cos, sin = rope_table(16)
    for conj in (False, True):
        a, b = lo.rope_oracle(qkv, cos, sin, 4, conj), go.gqa_rope_oracle(qkv, cos, sin, 4, 4, conj)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(lo.rope_roundtrip_envelope(qkv, cos, sin, 4), go.gqa_rope_roundtrip_envelope(qkv, cos, sin, 4, 4))


# ----------------------------------------------------------------------------- (c) the CPU path of the ops
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (6, 2)])
def test_attention_qkv_cpu_path_equals_expand_then_mha(H, Hkv, causal):
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv, attention_reference
    T, G = 37, H // Hkv
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(2, T, (H + 2 * Hkv) * 64, generator=g).requires_grad_()
    dy = torch.randn(2, T, H * 64, generator=g)
    y = attention_qkv(qkv, H, causal=causal, kv_heads=Hkv)
    (got_g,) = torch.autograd.grad(y, qkv, dy)
    x = qkv.detach().clone().requires_grad_()
    q, k, v = go.split_packed(x, H, Hkv)
    want = attention_reference(q, go.expand_kv(k, G), go.expand_kv(v, G), causal).transpose(1, 2).reshape(2, T, H * 64)
    (want_g,) = torch.autograd.grad(want, x, dy)
    torch.testing.assert_close(y.detach(), want.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(got_g, want_g, rtol=1e-5, atol=1e-6)


def test_kv_heads_equal_to_heads_is_the_call_without_it_on_cpu():
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    from pytorch_distributed_training_example_amd.ops.rope import rope_qkv_, rope_table
    g = torch.Generator().manual_seed(4)
    H, T = 3, 21
    base = torch.randn(2, T, 3 * H * 64, generator=g)
    cos, sin = rope_table(T)
    outs = []
    for kw in ({}, {"kv_heads": H}, {"kv_heads": None}):
        x = base.clone().requires_grad_()
        y = attention_qkv(rope_qkv_(x * 1.0, cos, sin, H, **kw), H, causal=True, **kw)
        y.square().sum().backward()
        outs.append((y.detach(), x.grad))
    for y, gx in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(gx, outs[0][1])


@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (12, 4)])
def test_rope_qkv_cpu_path_with_kv_heads(H, Hkv):
    from pytorch_distributed_training_example_amd.ops.rope import rope_qkv_, rope_table
    T = 9
    cos, sin = rope_table(T + 1)
    qkv = go.gqa_rope_inputs(2, T, H, Hkv).float()
    ref, _ = go.gqa_rope_oracle(qkv, cos, sin, H, Hkv)
    x = qkv.clone().requires_grad_()
    y = rope_qkv_(x * 1.0, cos, sin, H, kv_heads=Hkv)
    assert type(y.grad_fn).__name__.startswith("_RopeQKVFn")
    torch.testing.assert_close(y.detach().double(), ref, rtol=1e-6, atol=1e-6)
    assert torch.equal(y.detach()[..., (H + Hkv) * 64:], qkv[..., (H + Hkv) * 64:])
    dy = torch.randn(2, T, (H + 2 * Hkv) * 64, generator=torch.Generator().manual_seed(5))
    (gx,) = torch.autograd.grad(y, x, dy.clone())
    want, _ = go.gqa_rope_oracle(dy, cos, sin, H, Hkv, conj=True)
    torch.testing.assert_close(gx.double(), want, rtol=1e-6, atol=1e-6)


def test_refusals_on_cpu():
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    from pytorch_distributed_training_example_amd.ops.rope import rope_qkv_, rope_table
    cos, sin = rope_table(4)
    with pytest.raises(ValueError, match="dropout"):
        attention_qkv(torch.randn(1, 4, 8 * 64), 4, kv_heads=2, dropout_p=0.1)
    with pytest.raises(ValueError, match="multiple"):
        attention_qkv(torch.randn(1, 4, 10 * 64), 4, kv_heads=3)
    with pytest.raises(ValueError, match="multiple"):
        rope_qkv_(torch.randn(1, 4, 10 * 64), cos, sin, 4, kv_heads=3)
    with pytest.raises(ValueError, match="heads"):
        rope_qkv_(torch.randn(1, 4, 7 * 64 + 1), cos, sin, 4, kv_heads=2)
