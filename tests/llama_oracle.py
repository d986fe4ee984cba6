"""fp64 oracles and a-priori envelopes for the Llama-decoder kernels (rmsnorm.hip, rope.hip, swiglu.hip),
in the manner of oracle_envelope.py, whose comparator they use; plus the seeded inputs shared by the GPU
tests and by tests/test_llama_oracle_cpu.py, which proves on the CPU that the bounds hold for an fp32
emulation of each kernel and reject planted bugs. A helper module imported by plain name.

The oracle is the operation in float64 on the kernel's own (bf16 / fp32) inputs; the envelope bounds
what a correct kernel's roundings can do to each element; ``assert_within`` asks
``|actual - ref| <= c * (env + FLOOR)`` elementwise. The constants come from the analysis and are never
fitted to what the kernels return. u = 2^-24, u_out = the unit roundoff of the storage dtype.

RMSNorm (fp32 arithmetic on a row held in registers; n_s = D/64 + 7 roundings on the path of a row sum,
as for LayerNorm). All terms of mean(x^2) are positive, so the sum is perfectly conditioned and there is
no kappa term: rstd carries (n_s/2 + 5) u relative (the squares, the summation, the add of eps, rsqrt) and
    xh:  e_xh = u (n_s/2 + 8) |xh|
    y:   |w| e_xh + 2 u |y| + u_out |y|
    dx:  u (n_s + 8) rstd (|g w| + |xh| a2) + rstd (e_xh a2 + |xh| mean_j(|g w| e_xh)) + u_out |dx|
         with a2 = mean_j |g w xh|   (+ u |dx| for the + ds add)
    dw:  (N + 16) u sum_r |g xh| + sum_r |g| e_xh     (any summation order of N fp32 terms)
RMS_C = 2 for y and dx (rsqrt's own error and FMA contraction are not itemised), RMS_C_SUM = 1 for dw:
LN_C / LN_C_SUM and the same reasoning. The stored s = x + h is one correctly rounded add: bit for bit.

RoPE (x' = x_a cos -/+ x_b sin in fp32 from bf16 inputs and the kernel's own fp32 table, one rounding to
bf16): each product and the add round once, so
    2 u (|x[j] cos| + |x[j+32] sin|) + u_out |x'|,     ROPE_C = 2.
A forward followed by the conjugate rotation returns x up to the two bf16 roundings: the first, u_out |x'|
on each rotated value, passes through the inverse rotation, the second is that of the result:
    (u_out (1 + u_out) + 4 u) (|x'[j] cos| + |x'[j+32] sin|) + u_out |x|,   c = 1
(the u_out^2 term: the second rounding acts on the value that already carries the first one's error). Both
roundings are bounded rigorously and nothing else enters, so there is no constant to allow for.

SwiGLU (sg = 1 / (1 + e^-g) from the hardware exponential and reciprocal, each good to about one ulp; the
exponent's argument rounding costs u |g| relative):
    y:   u (8 + |g|) |y| + u_out |y|
    dg:  u (8 + |g|) |dy u| sg (1 + |g| (1 - sg)) + u_out |dg|   (absolute values: the cancellation of
         1 + g (1 - sg) near g = -1.28 is covered)
    du:  u (8 + |g|) |dy g sg| + u_out |du|
SWIGLU_C = 2.
"""
from __future__ import annotations

import torch

from oracle_envelope import FLOOR, U_FP32, assert_within, u_of  # noqa: F401  (re-exported to the tests)

RMS_C = 2.0
RMS_C_SUM = 1.0
ROPE_C = 2.0
SWIGLU_C = 2.0
EPS = 1e-5

# the backward's partition (rmsnorm.hip kBwdMinRows / kBwdMaxBlocks)
RMS_MIN_ROWS = 32
RMS_MAX_BLOCKS = 512


# ----------------------------------------------------------------------------- RMSNorm
def rmsnorm_oracle(x, w, eps, dy=None, h=None, ds=None):
    """x, dy (, h, ds): [N, D] in the storage dtype; w fp32 [D]. Returns (ref, env) with y (, s) and, with
    ``dy``, dx and dw. ``s`` is the sum as the storage dtype holds it; everything after is float64 on it."""
    u, u_out = U_FP32, u_of(x.dtype)
    s = (x.float() + h.float()).to(x.dtype) if h is not None else x
    X, W = s.double(), w.double()
    N, D = X.shape
    n_s = D / 64 + 7
    rstd = 1.0 / torch.sqrt((X * X).mean(-1, keepdim=True) + eps)
    xh = X * rstd
    y = xh * W
    e_xh = u * (n_s / 2 + 8) * xh.abs()
    ref = {"y": y, "rstd": rstd[:, 0]}
    env = {"y": W.abs() * e_xh + 2 * u * y.abs() + u_out * y.abs()}
    if h is not None:
        ref["s"] = s
    if dy is not None:
        G = dy.double()
        gw = G * W
        s2 = (gw * xh).mean(-1, keepdim=True)
        a2 = (gw * xh).abs().mean(-1, keepdim=True)
        dx = rstd * (gw - xh * s2)
        e_dx = u * (n_s + 8) * rstd * (gw.abs() + xh.abs() * a2) \
            + rstd * (e_xh * a2 + xh.abs() * (gw.abs() * e_xh).mean(-1, keepdim=True))
        if ds is not None:
            dx = dx + ds.double()
            e_dx = e_dx + u * dx.abs()
        ref.update(dx=dx, dw=(G * xh).sum(0))
        env.update(dx=e_dx + u_out * dx.abs(),
                   dw=(N + 16) * u * (G * xh).abs().sum(0) + (G.abs() * e_xh).sum(0))
    return ref, env


def rms_partition(N):
    """(rows per workgroup, workgroups) of the backward."""
    nblk = max(1, min(RMS_MAX_BLOCKS, -(-N // RMS_MIN_ROWS)))
    rpb = -(-N // nblk)
    return rpb, -(-N // rpb)


def rms_probe_rows(N):
    """The first and the last row of every workgroup's range (all of them up to 8 workgroups; else the
    first two, a middle one and the last two)."""
    rpb, nblk = rms_partition(N)
    blks = range(nblk) if nblk <= 8 else (0, 1, nblk // 2, nblk - 2, nblk - 1)
    rows = set()
    for b in blks:
        rows |= {b * rpb, min(N, (b + 1) * rpb) - 1}
    return sorted(rows)


def masked_rows(t, rows):
    z = torch.zeros_like(t)
    z[rows] = t[rows]
    return z


def rms_inputs(N, D, dtype, fused=False, regime="smooth", seed=None):
    """(x, dy, h, ds, w) on the CPU. Regimes: smooth (unit normal), largemean (x = 50 + 0.1 randn), probe
    (smooth, with dy and ds zero except on ``rms_probe_rows``)."""
    g = torch.Generator().manual_seed(1000 * D + N if seed is None else seed)
    r = lambda: torch.randn(N, D, generator=g)  # noqa: E731
    x = ((50.0 + 0.1 * r()) if regime == "largemean" else r()).to(dtype)
    dy = r().to(dtype)
    h, ds = ((0.1 * r() if regime == "largemean" else r()).to(dtype), r().to(dtype)) if fused else (None, None)
    w = torch.rand(D, generator=g) + 0.5
    if regime == "probe":
        rows = rms_probe_rows(N)
        dy = masked_rows(dy, rows)
        ds = masked_rows(ds, rows) if ds is not None else None
    return x, dy, h, ds, w


# ----------------------------------------------------------------------------- RoPE
def rope_oracle(qkv, cos, sin, heads, conj=False):
    """qkv [B, T, 3 * heads * 64] bf16, cos / sin fp32 [T_max, 32] (the kernel's own table). Returns
    (ref, env), float64 [B, T, 3 * heads * 64]; the V third of ref is qkv's and its envelope is 0."""
    B, T, C3 = qkv.shape
    X = qkv.double().view(B, T, 3, heads, 64)
    c = cos[:T].double().view(1, T, 1, 1, 32)
    s = sin[:T].double().view(1, T, 1, 1, 32) * (-1.0 if conj else 1.0)
    lo, hi = X[:, :, :2, :, :32], X[:, :, :2, :, 32:]
    ref, env = X.clone(), torch.zeros_like(X)
    ref[:, :, :2, :, :32] = lo * c - hi * s
    ref[:, :, :2, :, 32:] = hi * c + lo * s
    env[:, :, :2, :, :32] = 2 * U_FP32 * ((lo * c).abs() + (hi * s).abs())
    env[:, :, :2, :, 32:] = 2 * U_FP32 * ((hi * c).abs() + (lo * s).abs())
    env[:, :, :2] += u_of(qkv.dtype) * ref[:, :, :2].abs()
    return ref.view(B, T, C3), env.view(B, T, C3)


def rope_roundtrip_envelope(qkv, cos, sin, heads):
    """The bound on (forward, then conj) - qkv: two bf16 roundings of the rotation's terms (module docstring)."""
    B, T, C3 = qkv.shape
    u_out = u_of(qkv.dtype)
    rot, _ = rope_oracle(qkv, cos, sin, heads)
    R = rot.view(B, T, 3, heads, 64)
    c = cos[:T].double().view(1, T, 1, 1, 32).abs()
    s = sin[:T].double().view(1, T, 1, 1, 32).abs()
    lo, hi = R[:, :, :2, :, :32].abs(), R[:, :, :2, :, 32:].abs()
    env = torch.zeros_like(R)
    k = u_out * (1 + u_out) + 4 * U_FP32
    env[:, :, :2, :, :32] = k * (lo * c + hi * s)
    env[:, :, :2, :, 32:] = k * (hi * c + lo * s)
    env = env.view(B, T, C3)
    X = qkv.double().clone()
    X.view(B, T, 3, heads, 64)[:, :, 2] = 0
    return env + u_out * X.abs()


def rope_inputs(B, T, heads, seed=None):
    g = torch.Generator().manual_seed(10000 * B + 100 * heads + T if seed is None else seed)
    return torch.randn(B, T, 3 * heads * 64, generator=g).to(torch.bfloat16)


# ----------------------------------------------------------------------------- SwiGLU
def swiglu_oracle(gu, dy=None):
    """gu [N, 2F], dy [N, F] in the storage dtype. Returns (ref, env) with y and, with ``dy``, dg and du."""
    u, u_out = U_FP32, u_of(gu.dtype)
    F = gu.shape[-1] // 2
    g, up = gu[..., :F].double(), gu[..., F:].double()
    sg, oms = torch.sigmoid(g), torch.sigmoid(-g)  # 1 - sg without cancellation
    k = u * (8 + g.abs())
    y = g * sg * up
    ref, env = {"y": y}, {"y": k * y.abs() + u_out * y.abs()}
    if dy is not None:
        d = dy.double()
        dg = d * up * sg * (1 + g * oms)
        du = d * g * sg
        ref.update(dg=dg, du=du)
        env.update(dg=k * (d * up).abs() * sg * (1 + g.abs() * oms) + u_out * dg.abs(),
                   du=k * du.abs() + u_out * du.abs())
    return ref, env


def swiglu_inputs(N, F, dtype, seed=None):
    """(gu, dy) on the CPU: the gate spans [-12, 12] uniformly, with every 5th column clustered at
    -1.28 +- 0.02 (where 1 + g (1 - sg) cancels), the up projection and dy unit normal."""
    g = torch.Generator().manual_seed(100000 + 1000 * N + F if seed is None else seed)
    gate = torch.rand(N, F, generator=g) * 24 - 12
    gate[:, ::5] = -1.28 + 0.02 * torch.randn(N, (F + 4) // 5, generator=g)
    up = torch.randn(N, F, generator=g)
    dy = torch.randn(N, F, generator=g)
    return torch.cat([gate, up], -1).to(dtype), dy.to(dtype)
