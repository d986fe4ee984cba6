"""Rotary embedding in place on the packed QKV tensor (csrc/kernels/rope.hip) against the fp64 oracle of
tests/llama_oracle.py: the forward and the conjugate rotation inside the envelope, V and a guard band
behind the tensor bit-identical to before, forward + conj restoring Q and K to two bf16 roundings, autograd
through linear -> rope_qkv_ -> attention_qkv, and the binding's refusals (each with inputs that would stay
in bounds even if the check were missing)."""
import pytest
import torch

import llama_oracle as lo
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


@pytest.mark.parametrize("T", [1, 5, 64, 130])
@pytest.mark.parametrize("H", [1, 4, 12])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_conj_and_roundtrip(B, H, T):
    rope, nat = _ops()
    src = lo.rope_inputs(B, T, H)
    cos, sin = _table(T + 3)  # T_max > T
    x0 = src.to(DEV)
    v_before = x0.view(B, T, 3, H, 64)[:, :, 2].clone()
    errors = []
    for conj in (False, True):
        q, guard = _guarded(src)
        nat.rope_qkv(q, cos, sin, H, conj)
        ref, env = lo.rope_oracle(x0, cos, sin, H, conj)
        try:
            r = lo.assert_within(q, ref, env, lo.ROPE_C, lo.FLOOR, name=f"rope B={B} H={H} T={T} conj={int(conj)}")
            print(f"ratio rope B={B} H={H} T={T} conj={int(conj)} {r:.4g}")
        except AssertionError as e:
            errors.append(str(e))
        if not torch.equal(q.view(B, T, 3, H, 64)[:, :, 2], v_before):
            errors.append(f"conj={conj}: the V third changed")
        if not bool((guard == 7.0).all()):
            errors.append(f"conj={conj}: the guard band behind qkv was written")
    # the op (no autograd) is the same kernel and returns its argument; then the conj kernel restores Q and K
    q, guard = _guarded(src)
    assert rope.rope_qkv_(q, cos, sin, H) is q
    ref, env = lo.rope_oracle(x0, cos, sin, H)
    lo.assert_within(q, ref, env, lo.ROPE_C, lo.FLOOR, name="rope_qkv_")
    nat.rope_qkv(q, cos, sin, H, True)
    try:
        r = lo.assert_within(q, x0.double(), lo.rope_roundtrip_envelope(x0, cos, sin, H), 1.0, lo.FLOOR,
                             name=f"roundtrip B={B} H={H} T={T}")
        print(f"ratio roundtrip B={B} H={H} T={T} {r:.4g}")
    except AssertionError as e:
        errors.append(str(e))
    if not (torch.equal(q.view(B, T, 3, H, 64)[:, :, 2], v_before) and bool((guard == 7.0).all())):
        errors.append("roundtrip: V or the guard band changed")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("epilogue", ["auto", "1"], ids=["gemm_lib", "gemm_ours"])
@pytest.mark.parametrize("B,H,T", [(3, 4, 5), (1, 4, 130), (3, 2, 64)])
def test_autograd_through_linear_rope_attention(B, H, T, epilogue, switch):
    """linear -> rope_qkv_ -> attention_qkv -> <., dO>: the in-place rotation of c_attn's output raises no
    in-place-modification error (with the forward GEMM on the library and on our kernel), and the weight and
    input gradients are inside an envelope assembled stage by stage from the kernels' own stored values:
    attention's envelope (x ATTN_C) on the rotated qkv, carried through the float64 conjugate rotation (its
    absolute value), plus the rotation's own envelope (x ROPE_C), carried through the two gradient GEMMs
    (their absolute values) plus (K + 16) u sum|terms| + u_out |result| for a K-term fp32 accumulation."""
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    from pytorch_distributed_training_example_amd.ops.linear import linear
    rope, _ = _ops()
    switch("PDT_LINEAR_EPILOGUE", epilogue)
    Din, C3 = 64, 3 * H * 64
    g = torch.Generator().manual_seed(100 * T + H)
    x = torch.randn(B, T, Din, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
    w = (torch.randn(C3, Din, generator=g) * (0.5 / Din ** 0.5)).to(torch.bfloat16).to(DEV).requires_grad_()
    do = torch.randn(B, T, H * 64, generator=g).to(torch.bfloat16).to(DEV)
    cos, sin = _table(T + 1)

    qkv = linear(x, w)
    qkv0 = qkv.detach().clone()
    rot = rope.rope_qkv_(qkv, cos, sin, H)
    assert rot is qkv and type(rot.grad_fn).__name__.startswith("_RopeQKVFn")
    rot0 = rot.detach().clone()
    out = attention_qkv(rot, H, causal=True)
    assert type(out.grad_fn).__name__.startswith("_FlashQKVFn"), out.grad_fn
    out.backward(do)

    # forward: the rotation of the GEMM's own output
    ref, env = lo.rope_oracle(qkv0, cos, sin, H)
    lo.assert_within(rot0, ref, env, lo.ROPE_C, lo.FLOOR, name="rotated qkv")
    # attention's gradients on the rotated qkv the kernels read
    bhtd = lambda t5, i: t5[:, :, i].permute(0, 2, 1, 3)  # noqa: E731
    r5 = rot0.view(B, T, 3, H, 64)
    aref, aenv = oe.attention_oracle(bhtd(r5, 0), bhtd(r5, 1), bhtd(r5, 2),
                                     do.view(B, T, H, 64).permute(0, 2, 1, 3), causal=True)
    pack = lambda d: torch.stack([d[n].permute(0, 2, 1, 3) for n in ("dQ", "dK", "dV")], 2)  # noqa: E731
    G, E = pack(aref), oe.ATTN_C * pack(aenv)  # [B, T, 3, H, 64]
    # ... through the conjugate rotation (float64), with its own rounding
    c = cos[:T].double().view(1, T, 1, 1, 32)
    s = sin[:T].double().view(1, T, 1, 1, 32)
    G0, E0 = G.clone(), E.clone()
    glo, ghi, elo, ehi = G[:, :, :2, :, :32], G[:, :, :2, :, 32:], E[:, :, :2, :, :32], E[:, :, :2, :, 32:]
    G0[:, :, :2, :, :32], G0[:, :, :2, :, 32:] = glo * c + ghi * s, ghi * c - glo * s
    E0[:, :, :2, :, :32] = elo * c.abs() + ehi * s.abs() + lo.ROPE_C * 2 * lo.U_FP32 * ((glo * c).abs() + (ghi * s).abs())
    E0[:, :, :2, :, 32:] = ehi * c.abs() + elo * s.abs() + lo.ROPE_C * 2 * lo.U_FP32 * ((ghi * c).abs() + (glo * s).abs())
    E0[:, :, :2] += lo.ROPE_C * oe.U_BF16 * G0[:, :, :2].abs()
    # ... through dW = g0^T x and dx = g0 W
    M = B * T
    G0, E0 = G0.reshape(M, C3), E0.reshape(M, C3)
    X, W = x.detach().double().view(M, Din), w.detach().double()
    dw_ref, dx_ref = G0.t() @ X, G0 @ W
    dw_env = E0.t() @ X.abs() + (M + 16) * lo.U_FP32 * (G0.abs().t() @ X.abs()) + oe.U_BF16 * dw_ref.abs()
    dx_env = E0 @ W.abs() + (C3 + 16) * lo.U_FP32 * (G0.abs() @ W.abs()) + oe.U_BF16 * dx_ref.abs()
    r1 = lo.assert_within(w.grad, dw_ref, dw_env, 1.0, lo.FLOOR, name="dW")
    r2 = lo.assert_within(x.grad.view(M, Din), dx_ref, dx_env, 1.0, lo.FLOOR, name="dx")
    print(f"ratio chain B={B} H={H} T={T} {epilogue} dW {r1:.4g} dx {r2:.4g}")


def test_binding_refusals_launch_nothing():
    """Head dim 32, T > T_max and fp32 input each raise before any launch. Every bad input is the front of a
    buffer large enough for what the kernel would touch if the check were missing."""
    _, nat = _ops()
    B, T, H = 2, 6, 2
    cos, sin = _table(8)
    src = lo.rope_inputs(B, T, H)
    good = src.to(DEV)
    nat.rope_qkv(good, cos, sin, H, False)
    ref, env = lo.rope_oracle(src.to(DEV), cos, sin, H)
    lo.assert_within(good, ref, env, lo.ROPE_C, lo.FLOOR, name="valid call")

    # head dim 32: [B, T, 3 * H * 32] at the front of a buffer of B * T * 3 * H * 64 elements
    big = torch.randn(B * T * 3 * H * 64, device=DEV).to(torch.bfloat16)
    keep = big.clone()
    with pytest.raises(RuntimeError, match="head dim must be 64"):
        nat.rope_qkv(big[:B * T * 3 * H * 32].view(B, T, 3 * H * 32), cos, sin, H, False)
    # T > T_max: the [4, 32] tables are the front of the [8, 32] ones
    with pytest.raises(RuntimeError, match="exceeds the table"):
        nat.rope_qkv(big.view(B, T, 3 * H * 64), cos[:4], sin[:4], H, False)
    # fp32 input: twice the bytes of the bf16 tensor the kernel would address
    f32 = torch.randn(B, T, 3 * H * 64, device=DEV)
    keep32 = f32.clone()
    with pytest.raises(RuntimeError, match="must be bf16"):
        nat.rope_qkv(f32, cos, sin, H, False)
    # a strided last dim and a non-contiguous batch stride
    wide = torch.randn(B, T, 2 * 3 * H * 64, device=DEV).to(torch.bfloat16)
    for bad in (wide[:, :, ::2], wide[:, :, :3 * H * 64]):
        with pytest.raises(RuntimeError, match="contiguous"):
            nat.rope_qkv(bad, cos, sin, H, False)
    # a table of the wrong dtype (float64: more bytes than the fp32 one)
    with pytest.raises(RuntimeError, match=r"\bcos\b"):
        nat.rope_qkv(big.view(B, T, 3 * H * 64), cos.double(), sin, H, False)
    torch.cuda.synchronize()
    assert torch.equal(big, keep) and torch.equal(f32, keep32)
    # the op itself refuses too, before reaching the binding
    from pytorch_distributed_training_example_amd.ops.rope import rope_qkv_
    with pytest.raises(ValueError, match="exceeds the table"):
        rope_qkv_(big.view(B, T, 3 * H * 64), cos[:4], sin[:4], H)
    with pytest.raises(ValueError, match="contiguous"):
        rope_qkv_(wide[:, :, :3 * H * 64], cos, sin, H)
