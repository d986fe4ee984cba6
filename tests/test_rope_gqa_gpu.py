"""The grouped-query launch of the rotary kernel (csrc/kernels/rope.hip, ``rope_qkv_gqa``) on the packed
[B, T, (H + 2 Hkv) 64] tensor against the fp64 oracle of tests/gqa_oracle.py: forward and conjugate rotation
inside the envelope on the H + Hkv rotated heads, the Hkv value heads and a guard band behind the tensor
bit-identical to before, forward + conj restoring Q and K to two bf16 roundings, the binding's refusals (each
with inputs that would stay in bounds even if the check were missing), and autograd through
linear -> rope_qkv_ -> attention_qkv with ``kv_heads``."""
import pytest
import torch

import gqa_oracle as go
import oracle_envelope as oe

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _ops():
    from pytorch_distributed_training_example_amd.ops import rope
    from pytorch_distributed_training_example_amd.ops._native import native
    return rope, native()


def _table(T_max):
    rope, _ = _ops()
    cos, sin = rope.rope_table(T_max)
    return cos.to(DEV), sin.to(DEV)


def _guarded(qkv_cpu):
    """qkv at the front of a buffer with GUARD more elements (filled with 7) behind it."""
    n = qkv_cpu.numel()
    buf = torch.full((n + GUARD,), 7.0, dtype=qkv_cpu.dtype, device=DEV)
    buf[:n] = qkv_cpu.reshape(-1).to(DEV)
    return buf[:n].view(qkv_cpu.shape), buf[n:]


@pytest.mark.parametrize("T", [1, 5, 130])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (12, 4)])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_conj_and_roundtrip(B, H, Hkv, T):
    rope, nat = _ops()
    src = go.gqa_rope_inputs(B, T, H, Hkv)
    cos, sin = _table(T + 3)  # T_max > T
    x0 = src.to(DEV)
    R = (H + Hkv) * 64
    v_before = x0[..., R:].clone()
    tag = f"B={B} H={H} Hkv={Hkv} T={T}"
    errors = []
    for conj in (False, True):
        q, guard = _guarded(src)
        nat.rope_qkv_gqa(q, cos, sin, H, Hkv, conj)
        ref, env = go.gqa_rope_oracle(x0, cos, sin, H, Hkv, conj)
        try:
            r = oe.assert_within(q, ref, env, go.ROPE_C, go.FLOOR, name=f"rope gqa {tag} conj={int(conj)}")
            print(f"ratio rope gqa {tag} conj={int(conj)} {r:.4g}")
        except AssertionError as e:
            errors.append(str(e))
        if not torch.equal(q[..., R:], v_before):
            errors.append(f"conj={conj}: the V heads changed")
        if not bool((guard == 7.0).all()):
            errors.append(f"conj={conj}: the guard band behind qkv was written")
    # the op (no autograd) is the same kernel and returns its argument; then the conj kernel restores Q and K
    q, guard = _guarded(src)
    assert rope.rope_qkv_(q, cos, sin, H, kv_heads=Hkv) is q
    ref, env = go.gqa_rope_oracle(x0, cos, sin, H, Hkv)
    oe.assert_within(q, ref, env, go.ROPE_C, go.FLOOR, name="rope_qkv_")
    nat.rope_qkv_gqa(q, cos, sin, H, Hkv, True)
    try:
        r = oe.assert_within(q, x0.double(), go.gqa_rope_roundtrip_envelope(x0, cos, sin, H, Hkv), 1.0, go.FLOOR,
                             name=f"roundtrip {tag}")
        print(f"ratio roundtrip gqa {tag} {r:.4g}")
    except AssertionError as e:
        errors.append(str(e))
    if not (torch.equal(q[..., R:], v_before) and bool((guard == 7.0).all())):
        errors.append("roundtrip: V or the guard band changed")
    assert not errors, "\n".join(errors)


def test_equal_head_counts_give_the_multi_head_launch_bits():
    _, nat = _ops()
    B, T, H = 3, 130, 4
    src = go.gqa_rope_inputs(B, T, H, H).to(DEV)
    cos, sin = _table(T)
    for conj in (False, True):
        a, b = src.clone(), src.clone()
        nat.rope_qkv(a, cos, sin, H, conj)
        nat.rope_qkv_gqa(b, cos, sin, H, H, conj)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_binding_refusals_launch_nothing():
    """A last dim that is not (H + 2 Hkv) 64, heads that do not divide, T > T_max: each raises before any launch.
    Every bad input is (the front of) a buffer at least as large as what the kernel would touch if the check
    were missing."""
    _, nat = _ops()
    B, T, H, Hkv = 2, 6, 4, 2
    cos, sin = _table(8)
    big = torch.randn(B * T * 3 * H * 64, device=DEV).to(torch.bfloat16)  # the multi-head size: the largest claimed
    keep = big.clone()
    n = B * T * (H + 2 * Hkv) * 64
    good = big[:n].view(B, T, (H + 2 * Hkv) * 64)
    # the multi-head width with Hkv = 2, and the grouped width with the wrong head counts
    with pytest.raises(RuntimeError, match="head dim must be 64"):
        nat.rope_qkv_gqa(big.view(B, T, 3 * H * 64), cos, sin, H, Hkv, False)
    with pytest.raises(RuntimeError, match="head dim must be 64"):
        nat.rope_qkv_gqa(good, cos, sin, H, 1, False)
    with pytest.raises(RuntimeError, match="head dim must be 64"):
        nat.rope_qkv(good, cos, sin, H, False)
    # head dim 32 at the grouped layout
    with pytest.raises(RuntimeError, match="head dim must be 64"):
        nat.rope_qkv_gqa(big[:n // 2].view(B, T, (H + 2 * Hkv) * 32), cos, sin, H, Hkv, False)
    # 3 K/V heads for 4 query heads: [B, T, 10 * 64] fits in big
    with pytest.raises(RuntimeError, match="multiple"):
        nat.rope_qkv_gqa(big[:B * T * 10 * 64].view(B, T, 10 * 64), cos, sin, H, 3, False)
    with pytest.raises(RuntimeError, match="exceeds the table"):
        nat.rope_qkv_gqa(good, cos[:4], sin[:4], H, Hkv, False)
    with pytest.raises(RuntimeError, match="must be bf16"):
        nat.rope_qkv_gqa(torch.zeros(B, T, (H + 2 * Hkv) * 64, device=DEV), cos, sin, H, Hkv, False)
    torch.cuda.synchronize()
    assert torch.equal(big, keep)
    # the op refuses too, before reaching the binding
    rope, _ = _ops()
    with pytest.raises(ValueError, match="heads"):
        rope.rope_qkv_(big[:B * T * 7 * 64 + B * T].view(B, T, 7 * 64 + 1), cos, sin, H, kv_heads=Hkv)
    with pytest.raises(ValueError, match="exceeds the table"):
        rope.rope_qkv_(good, cos[:4], sin[:4], H, kv_heads=Hkv)
    assert torch.equal(big, keep)


@pytest.mark.parametrize("B,H,Hkv,T", [(3, 4, 2, 5), (1, 4, 1, 130), (2, 6, 2, 64)])
def test_autograd_through_linear_rope_attention(B, H, Hkv, T):
    """linear -> rope_qkv_(kv_heads) -> attention_qkv(kv_heads): the kernels' autograd Functions are the ones on
    the tape, the in-place rotation raises no in-place-modification error, the rotated tensor is inside the
    rotation's envelope and the gradients are finite."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    from pytorch_distributed_training_example_amd.ops.linear import linear
    rope, _ = _ops()
    Din, C = 64, (H + 2 * Hkv) * 64
    g = torch.Generator().manual_seed(100 * T + H)
    x = torch.randn(B, T, Din, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    w = (torch.randn(C, Din, generator=g) * (0.5 / Din ** 0.5)).to(torch.bfloat16).to(DEV).requires_grad_()
    do = torch.randn(B, T, H * 64, generator=g).to(torch.bfloat16).to(DEV)
    cos, sin = _table(T + 1)
    qkv = linear(x, w)
    qkv0 = qkv.detach().clone()
    rot = rope.rope_qkv_(qkv, cos, sin, H, kv_heads=Hkv)
    assert rot is qkv and type(rot.grad_fn).__name__.startswith("_RopeQKVFn")
    rot0 = rot.detach().clone()
    out = attention_qkv(rot, H, causal=True, kv_heads=Hkv)
    assert type(out.grad_fn).__name__.startswith("_FlashGQAFn"), out.grad_fn
    out.backward(do)
    ref, env = go.gqa_rope_oracle(qkv0, cos, sin, H, Hkv)
    oe.assert_within(rot0, ref, env, go.ROPE_C, go.FLOOR, name="rotated qkv")
    q, k, v = go.split_packed(rot0, H, Hkv)
    aref, aenv = go.gqa_attention_oracle(q, k, v, do.view(B, T, H, 64).permute(0, 2, 1, 3), causal=True)
    oe.assert_within(out.detach().view(B, T, H, 64).permute(0, 2, 1, 3), aref["O"], aenv["O"], go.ATTN_C, go.FLOOR, name="O")
    assert x.grad.shape == x.shape and w.grad.shape == w.shape
    assert bool(torch.isfinite(x.grad.float()).all()) and bool(torch.isfinite(w.grad.float()).all())
    assert float(w.grad.float().abs().max()) > 0 and float(x.grad.float().abs().max()) > 0
