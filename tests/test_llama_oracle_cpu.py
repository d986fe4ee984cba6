"""The envelopes of tests/llama_oracle.py are sharp, shown on the CPU before any GPU run, in the manner
of test_oracle_envelope_cpu.py:
  * the fp64 oracles agree with torch's own float64 autograd;
  * an fp32 emulation of each kernel's roundings stays inside every bound, on the very inputs the GPU
    tests use (llama_oracle.rms_inputs / rope_inputs / swiglu_inputs);
  * each planted bug is rejected on inputs at which the clean emulation passes: one RMSNorm row left out
    of dw, mean(x^2) over D - 1, RoPE on the pairs (2j, 2j+1), RoPE at position t + 1, the backward
    rotated by +theta, SwiGLU with gate and up swapped, dg without the g (1 - sigma) term."""
import pytest
import torch
import torch.nn.functional as F

import llama_oracle as lo
from pytorch_distributed_training_example_amd.ops.rope import rope_table


def _failed(got, ref, env, consts):
    bad = set()
    for name, c in consts.items():
        try:
            lo.assert_within(got[name], ref[name], env[name], c, lo.FLOOR, name=name)
        except AssertionError:
            bad.add(name)
    return bad


# ----------------------------------------------------------------------------- oracles against autograd
@pytest.mark.parametrize("fused", [False, True])
def test_rmsnorm_oracle_matches_float64_autograd(fused):
    x, dy, h, ds, w = lo.rms_inputs(9, 256, torch.float32, fused=True)
    xs = ((x + h) if fused else x).double().requires_grad_()
    wd = w.double().requires_grad_()
    y = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + lo.EPS) * wd
    outs, grads = ([xs, y], [ds.double(), dy.double()]) if fused else ([y], [dy.double()])
    dx, dw = torch.autograd.grad(outs, (xs, wd), grads)
    ref, env = lo.rmsnorm_oracle(x, w, lo.EPS, dy, h if fused else None, ds if fused else None)
    for a, r in ((ref["y"], y.detach()), (ref["dx"], dx), (ref["dw"], dw)):
        torch.testing.assert_close(a, r, rtol=1e-11, atol=1e-11)
    assert all(bool((e > 0).all()) for e in env.values())
    if hasattr(F, "rms_norm"):
        torch.testing.assert_close(ref["y"], F.rms_norm(xs.detach(), (256,), w.double(), lo.EPS), rtol=1e-11, atol=1e-11)


def test_rope_oracle_is_hf_rotate_half_and_orthogonal():
    qkv = lo.rope_inputs(2, 7, 3)
    cos, sin = rope_table(16)
    ref, _ = lo.rope_oracle(qkv, cos, sin, 3)
    X = qkv.double().view(2, 7, 3, 3, 64)
    c = torch.cat([cos[:7], cos[:7]], -1).double().view(1, 7, 1, 64)
    s = torch.cat([sin[:7], sin[:7]], -1).double().view(1, 7, 1, 64)
    rot_half = lambda t: torch.cat([-t[..., 32:], t[..., :32]], -1)  # noqa: E731  (HF modeling_llama)
    R = ref.view(2, 7, 3, 3, 64)
    for i in range(2):
        torch.testing.assert_close(R[:, :, i], X[:, :, i] * c + rot_half(X[:, :, i]) * s, rtol=1e-13, atol=1e-13)
    assert torch.equal(R[:, :, 2], X[:, :, 2])
    # the conjugate rotation is the transpose: <R x, g> = <x, R^T g>
    g = torch.randn(2, 7, 3 * 3 * 64, dtype=torch.float64).to(torch.bfloat16)
    back, _ = lo.rope_oracle(g, cos, sin, 3, conj=True)
    torch.testing.assert_close((ref * g.double()).sum(), (qkv.double() * back).sum(), rtol=1e-12, atol=1e-9)


def test_swiglu_oracle_matches_float64_autograd():
    gu, dy = lo.swiglu_inputs(7, 24, torch.float32)
    gd = gu.double().requires_grad_()
    y = F.silu(gd[:, :24]) * gd[:, 24:]
    (dgu,) = torch.autograd.grad(y, gd, dy.double())
    ref, env = lo.swiglu_oracle(gu, dy)
    torch.testing.assert_close(ref["y"], y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(torch.cat([ref["dg"], ref["du"]], -1), dgu, rtol=1e-11, atol=1e-12)
    assert all(bool((e >= 0).all()) for e in env.values())


# ----------------------------------------------------------------------------- RMSNorm
RMS_CONSTS = {"y": lo.RMS_C, "dx": lo.RMS_C, "dw": lo.RMS_C_SUM}


def emulate_rmsnorm(x, dy, w, eps, h=None, ds=None, skip_row=None, d_minus_1=False):
    """fp32 RMSNorm forward / backward the way the kernel forms it, outputs rounded to x's dtype."""
    s = (x.float() + h.float()).to(x.dtype) if h is not None else x
    X, G = s.float(), dy.float()
    D = X.shape[-1]
    rstd = torch.rsqrt((X * X).sum(-1, keepdim=True) / (D - 1 if d_minus_1 else D) + eps)
    xh = X * rstd
    y = (xh * w).to(x.dtype)
    gw = G * w
    dx = rstd * (gw - xh * (gw * xh).mean(-1, keepdim=True))
    if ds is not None:
        dx = dx + ds.float()
    rows = torch.ones(X.shape[0])
    if skip_row is not None:
        rows[skip_row] = 0
    return {"s": s, "y": y, "dx": dx.to(x.dtype), "dw": (G * xh * rows[:, None]).sum(0)}


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,D,regime", [(1, 256, "smooth"), (33, 768, "smooth"), (33, 1024, "probe"),
                                        (129, 2048, "smooth"), (33, 1024, "largemean"), (65, 768, "probe")])
def test_rmsnorm_emulation_within_bounds(N, D, regime, dtype, fused):
    x, dy, h, ds, w = lo.rms_inputs(N, D, dtype, fused, regime)
    ref, env = lo.rmsnorm_oracle(x, w, lo.EPS, dy, h, ds)
    got = emulate_rmsnorm(x, dy, w, lo.EPS, h, ds)
    assert not _failed(got, ref, env, RMS_CONSTS)
    if fused:
        assert torch.equal(got["s"], ref["s"])


@pytest.mark.parametrize("N", [33, 65, 5])
def test_rmsnorm_row_left_out_of_dw_is_rejected(N):
    x, dy, _, _, w = lo.rms_inputs(N, 768, torch.float32, False, "probe")
    ref, env = lo.rmsnorm_oracle(x, w, lo.EPS, dy)
    assert not _failed(emulate_rmsnorm(x, dy, w, lo.EPS), ref, env, RMS_CONSTS)
    for row in lo.rms_probe_rows(N):
        assert "dw" in _failed(emulate_rmsnorm(x, dy, w, lo.EPS, skip_row=row), ref, env, RMS_CONSTS), row


@pytest.mark.parametrize("D", [256, 2048])
def test_rmsnorm_mean_over_d_minus_1_is_rejected(D):
    x, dy, _, _, w = lo.rms_inputs(33, D, torch.float32)
    ref, env = lo.rmsnorm_oracle(x, w, lo.EPS, dy)
    assert not _failed(emulate_rmsnorm(x, dy, w, lo.EPS), ref, env, RMS_CONSTS)
    assert {"y", "dx"} <= _failed(emulate_rmsnorm(x, dy, w, lo.EPS, d_minus_1=True), ref, env, RMS_CONSTS)


# ----------------------------------------------------------------------------- RoPE
def emulate_rope(qkv, cos, sin, heads, conj=False, mut=None):
    """fp32 rotation of the Q and K thirds, one rounding to bf16. ``mut``: interleaved (pairs (2j, 2j+1)),
    t_plus_1 (the next position's angles), no_conj (the sine not negated when ``conj``)."""
    B, T, C3 = qkv.shape
    X = qkv.float().view(B, T, 3, heads, 64).clone()
    t0 = 1 if mut == "t_plus_1" else 0
    c = cos[t0:t0 + T].view(1, T, 1, 1, 32)
    s = sin[t0:t0 + T].view(1, T, 1, 1, 32)
    if conj and mut != "no_conj":
        s = -s
    qk = X[:, :, :2]
    if mut == "interleaved":
        a, b = qk[..., 0::2].clone(), qk[..., 1::2].clone()
        qk[..., 0::2], qk[..., 1::2] = a * c - b * s, b * c + a * s
    else:
        a, b = qk[..., :32].clone(), qk[..., 32:].clone()
        qk[..., :32], qk[..., 32:] = a * c - b * s, b * c + a * s
    return X.view(B, T, C3).to(torch.bfloat16)


ROPE_CASES = [(1, 1, 1), (3, 5, 4), (1, 64, 12), (3, 130, 4)]


@pytest.mark.parametrize("B,T,H", ROPE_CASES)
def test_rope_emulation_within_bounds(B, T, H):
    qkv = lo.rope_inputs(B, T, H)
    cos, sin = rope_table(T + 3)
    for conj in (False, True):
        ref, env = lo.rope_oracle(qkv, cos, sin, H, conj)
        lo.assert_within(emulate_rope(qkv, cos, sin, H, conj), ref, env, lo.ROPE_C, lo.FLOOR, name=f"rope conj={conj}")
    back = emulate_rope(emulate_rope(qkv, cos, sin, H), cos, sin, H, conj=True)
    lo.assert_within(back, qkv.double(), lo.rope_roundtrip_envelope(qkv, cos, sin, H), 1.0, lo.FLOOR, name="roundtrip")


@pytest.mark.parametrize("mut", ["interleaved", "t_plus_1"])
def test_rope_wrong_pairing_or_position_is_rejected(mut):
    qkv = lo.rope_inputs(3, 5, 4)
    cos, sin = rope_table(8)
    ref, env = lo.rope_oracle(qkv, cos, sin, 4)
    with pytest.raises(AssertionError):
        lo.assert_within(emulate_rope(qkv, cos, sin, 4, mut=mut), ref, env, lo.ROPE_C, lo.FLOOR)


def test_rope_backward_rotated_by_plus_theta_is_rejected():
    qkv = lo.rope_inputs(3, 5, 4)
    cos, sin = rope_table(8)
    ref, env = lo.rope_oracle(qkv, cos, sin, 4, conj=True)
    with pytest.raises(AssertionError):
        lo.assert_within(emulate_rope(qkv, cos, sin, 4, conj=True, mut="no_conj"), ref, env, lo.ROPE_C, lo.FLOOR)
    back = emulate_rope(emulate_rope(qkv, cos, sin, 4), cos, sin, 4, conj=True, mut="no_conj")
    with pytest.raises(AssertionError):
        lo.assert_within(back, qkv.double(), lo.rope_roundtrip_envelope(qkv, cos, sin, 4), 1.0, lo.FLOOR)


# ----------------------------------------------------------------------------- SwiGLU
SWIGLU_CONSTS = {"y": lo.SWIGLU_C, "dg": lo.SWIGLU_C, "du": lo.SWIGLU_C}


def emulate_swiglu(gu, dy, mut=None):
    """fp32 SwiGLU the way the kernel forms it (sigma from e^-g and a reciprocal, 1 - sigma as e^-g sigma
    for g > 0), outputs rounded to gu's dtype. ``mut``: swapped (gate and up), no_g_term (dg = dy u sigma)."""
    Fh = gu.shape[-1] // 2
    g, u = gu[..., :Fh].float(), gu[..., Fh:].float()
    if mut == "swapped":
        g, u = u, g
    d = dy.float()
    e = torch.exp(-g)
    sg = 1.0 / (1.0 + e)
    oms = torch.where(g > 0, e * sg, 1.0 - sg)
    dg = d * u * sg * (1.0 if mut == "no_g_term" else (1.0 + g * oms))
    return {"y": (g * sg * u).to(gu.dtype), "dg": dg.to(gu.dtype), "du": (d * g * sg).to(gu.dtype)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,Fh", [(1, 8), (7, 264), (257, 264), (7, 2816)])
def test_swiglu_emulation_within_bounds(N, Fh, dtype):
    gu, dy = lo.swiglu_inputs(N, Fh, dtype)
    assert float(gu[:, :Fh].float().min()) < -11 and float(gu[:, :Fh].float().max()) > 11 or N * Fh < 64
    ref, env = lo.swiglu_oracle(gu, dy)
    assert not _failed(emulate_swiglu(gu, dy), ref, env, SWIGLU_CONSTS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_swiglu_planted_bugs_are_rejected(dtype):
    gu, dy = lo.swiglu_inputs(7, 264, dtype)
    ref, env = lo.swiglu_oracle(gu, dy)
    assert not _failed(emulate_swiglu(gu, dy), ref, env, SWIGLU_CONSTS)
    assert {"y", "dg", "du"} <= _failed(emulate_swiglu(gu, dy, mut="swapped"), ref, env, SWIGLU_CONSTS)
    assert _failed(emulate_swiglu(gu, dy, mut="no_g_term"), ref, env, SWIGLU_CONSTS) == {"dg"}
