"""fp64 oracle and condition envelopes for the BatchNorm kernels (csrc/kernels/batchnorm.hip). A helper
module imported by plain name, like oracle_envelope.py, whose comparator (``assert_within``,
``worst_ratio``, ``FLOOR``) it reuses; tests/test_bn_oracle_cpu.py proves on the CPU that it is sharp.

Method (that of oracle_envelope.py). The reference is the operation in float64 on the kernel's own bf16 /
fp32 inputs; the envelope of a result is an a-priori bound on what a correct kernel's roundings can do to
it, built from the same fp64 quantities. u = 2^-24 (fp32), u_out = 2^-8 (bf16). The constants are fixed
here from the analysis and never fitted to what the kernels return: BN_C_SUM = 1 for everything per
channel, BN_C = 2 for the elementwise outputs (as LN_C: FMA contraction order is not itemised).
Activations are [M, C] (channels last, flattened), all per-channel quantities [C].

Sums. The forward reduce adds S1 = sum_m d_m and S2 = sum_m d_m^2 with d = x - k, k = x[0, c] (the shift
of bn_reduce3_kernel); the backward adds sum dz and sum dz (x - mean), dz = dy * mask. A term passes
through at most n_path fp32 roundings, so
    e_S = n_path u sum|terms|                        (terms that are exactly 0 add nothing)
    n_path = ceil(rows_per_block / R)                sequential adds of one lane
           + R                                       the R-row LDS column sum
           + ceil(nrow / 8) + 8   (variant 5)        bn_fin_kernel: 8 strided subsets, then 8 adds
           | min(16, nrow) + ngroups   (variant 3)   group slabs, then the group sums
           + 8                                       the subtraction, the product / fma, gamma_n vs n u
with (rows_per_block, nrow, R) from ``reduce_geo3`` below, a replica of the launch geometry. Adding an exact
zero rounds nothing, so a sum with nnz non-zero terms rounds at most nnz - 1 times in all, whatever the tree:
n_path is replaced by min(n_path, nnz + 8) per channel (the probe inputs: a handful of non-zero rows).

Per-channel forward results (d1 = S1 / M; the kernel does this part in double, so only the sums' and the
casts' errors appear):
    mean = k + d1:        e_mean = e_S1 / M + u |mean|                      (the cast to fp32)
    var = S2 / M - d1^2:  e_var  = e_S2 / M + 2 |d1| e_d1 + e_d1^2,  e_d1 = e_S1 / M   (the cancelling step)
    invstd = (var + eps)^-1/2:  e_is = max over var +- e_var of |change|, + u invstd   (eps as fp32 holds it)
    a = gamma invstd:     e_a = |gamma| e_is + u |a|
    b = beta - (mean gamma) invstd:  e_b = |a| e_mean + |mean gamma| e_is + 2 u |mean a| + u |b|
    running_mean' = (1 - p) rm + p mean:  p e_mean + u (2 |(1 - p) rm| + |p mean| + |rm'|)
    running_var'  = (1 - p) rv + p unb, unb = var M / (M - 1) (M = 1: var, as the op keeps it):
                    p (e_var M / (M - 1) + u |unb|) + u (2 |(1 - p) rv| + |p unb| + |rv'|)
From double-accumulated partials (the tile finalizes) the sums carry u |partial| each and nothing else:
    e_S = u sum_t |s_t|,  e_Q = u sum_t (|q_t| + 2 s_t^2 / n_t).
Eval: invstd = rsqrtf(rv + eps): e_is = 3 u invstd (the add, and 2 u for rsqrtf), mean exact.

Forward elementwise, t = a x + b (+ r | + ra r + rb), y = bf16(relu?(t)):
    e_t = |x| e_a + e_b + u (|a x| + |a x + b|) (+ u |t| | + u (|ra r| + |ra r + rb| + |t|))
    e_y = e_t + u_out |y|
ReLU: where |t| > 2 e_t the decision is the reference's (mask bit and y > 0 compared exactly); the other
elements are *ambiguous* (``amb``): their y is held to the envelope only (relu is 1-Lipschitz), and their
share is capped at AMBIGUOUS_CAP (per tensor from 10^4 elements on, and per test case: AmbiguityPool). The backward oracle takes the mask actually used (``mask=``), so the
backward comparison needs no exclusions.

Backward, with S1 = sum dz, S2 = sum dz (x - mean_k), mean_k / invstd_k the fp32 statistics the kernel is
given (within e_mean / e_is of the reference, whether they come from the forward kernel or are the
rounded reference):
    dbeta = S1:            e_db = n_path u sum|dz|
    dgamma = S2 invstd:    e_dg = invstd (n_path u sum|dz (x - mean)| + |dbeta| e_mean) + |S2| e_is + u |dgamma|
    A = gamma invstd:      e_A = |gamma| e_is + u |A|
    B = -gamma invstd^2 dgamma / M:  e_B = |gamma| invstd^2 e_dg / M + 2 |B| e_is / invstd + 6 u |B|
    D = -gamma invstd dbeta / M:     e_D = |gamma| invstd e_db / M + |D| e_is / invstd + 5 u |D|
    dx = A dz + B (x - mean) + D:
        e_dx = |dz| e_A + |x - mean| e_B + |B| e_mean + e_D + u (2 |A dz| + 3 |B (x - mean)| + 2 |D|) + u_out |dx|
    dres = dz, bit for bit.

Rounding mode: ``rounding_bias`` is the mean of (|y| - |y_ref|) / |y_ref| over |y_ref| >= 2^-6; round to
nearest even (common.h) gives ~1e-5, truncation ~ -1.4e-3; the bound is +-2^-11.

Stem pool (bn_apply_pool_kernel / maxpool_bwd_kernel): z = fma(x, a, b) per window element, one rounding:
e_z = |x| e_a + e_b + u |z|; the pooled y is bf16(relu(max z)) with e_y = max over the window of e_z +
u_out |y|; the winner code is the first element in (kh, kw) scan order that attains the maximum, compared
exactly unless the best and second-best DISTINCT values lie within 2 e_z (ambiguous, same cap); code 15
exactly where the max is <= 0. The pool gradient sums at most four bf16 terms in fp32 and rounds to bf16:
e_dz = u_out |dz| + 4 u sum|terms|.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from oracle_envelope import FLOOR, U_BF16, U_FP32, assert_within, worst_ratio  # noqa: F401  (re-exported)

BN_C = 2.0
BN_C_SUM = 1.0
AMBIGUOUS_CAP = 1e-4
ROUNDING_BIAS_MAX = 2.0 ** -11
K_THREADS = 256  # batchnorm.hip kThreads
K_G = 16         # batchnorm.hip kG: blocks per level-1 group of the in-kernel finalize


# ----------------------------------------------------------------------------- launch geometry
class Path(NamedTuple):
    """The bn_tune setting a call ran under (defaults: BnTune's)."""
    variant: int = 5
    target_blocks: int = 512
    u_fwd: int = 8
    u_bwd: int = 4


class Geo(NamedTuple):
    cc: int               # channels per chunk
    R: int                # rows per pass
    nchunks: int
    nrow: int             # reduce blocks per chunk (= slabs)
    rows_per_block: int
    ngroups: int


def chunk3(C: int) -> int:
    """batchnorm.hip chunk3: for (cc = 512; cc > 64; cc >>= 1) if (C % cc == 0) return cc; return 64."""
    for cc in (512, 256, 128):
        if C % cc == 0:
            return cc
    return 64


def reduce_geo3(M: int, C: int, U: int, target_blocks: int = 512) -> Geo:
    """batchnorm.hip reduce_geo3, line by line."""
    cc = chunk3(C)
    nchunks = C // cc                                  # g.nchunks = C / cc
    R = K_THREADS // (cc // 8)                         # R = kThreads / (cc / 8)
    nrow = target_blocks // nchunks                    # nrow = g_tune.target_blocks / g.nchunks
    nrow = min(nrow, 1024)                             # if (nrow > 1024) nrow = 1024
    max_rows = (M + 2 * U * R - 1) // (2 * U * R)      # max_rows = ceil(M / (2 U R))
    nrow = min(nrow, max_rows)                         # if (nrow > max_rows) nrow = max_rows
    nrow = max(nrow, 1)                                # if (nrow < 1) nrow = 1
    rpb = (M + nrow - 1) // nrow                       # g.rows_per_block = ceil(M / nrow)
    nrow = (M + rpb - 1) // rpb                        # g.nrow = ceil(M / rows_per_block)
    return Geo(cc, R, nchunks, nrow, rpb, (nrow + K_G - 1) // K_G)


def n_path(M: int, C: int, U: int, path: Path = Path()) -> int:
    """fp32 roundings on the path of one term of a reduce sum (module docstring)."""
    g = reduce_geo3(M, C, U, path.target_blocks)
    slab = (math.ceil(g.nrow / 8) + 8) if path.variant == 5 else (min(K_G, g.nrow) + g.ngroups)
    return math.ceil(g.rows_per_block / g.R) + g.R + slab + 8


def n_eff(terms, n: int):
    """min(n_path, nnz + 8) per channel for the [M, C] terms of a sum."""
    return (terms != 0).sum(0).double().add(8).clamp_max(n)


# ----------------------------------------------------------------------------- per-channel propagation
def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def _opt(t, C, fill, like):
    return torch.full((C,), fill, dtype=torch.float64, device=like.device) if t is None else t.double()


def stats_envelopes(mean, var, e_mean_sum, e_var, M, w, b, running_mean, running_var, momentum, eps):
    """From the fp64 batch mean / biased variance and the envelopes of their sums (e_mean_sum: of the mean
    before its cast to fp32) to (ref, env) of mean, invstd, a, b, running_mean, running_var."""
    u = U_FP32
    C = mean.numel()
    eps, p = _f32(eps), _f32(momentum)
    gm, bt = _opt(w, C, 1.0, mean), _opt(b, C, 0.0, mean)
    e_mean = e_mean_sum + u * mean.abs()
    inv = (var + eps).rsqrt()
    inv_hi = ((var - e_var).clamp_min(0) + eps).rsqrt()
    inv_lo = (var + e_var + eps).rsqrt()
    e_is = torch.maximum(inv_hi - inv, inv - inv_lo) + u * inv
    a = gm * inv
    bb = bt - mean * a
    e_a = gm.abs() * e_is + u * a.abs()
    e_b = a.abs() * e_mean + (mean * gm).abs() * e_is + 2 * u * (mean * a).abs() + u * bb.abs()
    ref = {"mean": mean, "var": var, "invstd": inv, "a": a, "b": bb}
    env = {"mean": e_mean, "var": e_var, "invstd": e_is, "a": e_a, "b": e_b}
    if running_mean is not None:
        rm = running_mean.double()
        new = (1 - p) * rm + p * mean
        ref["running_mean"] = new
        env["running_mean"] = p * e_mean + u * (2 * ((1 - p) * rm).abs() + (p * mean).abs() + new.abs())
    if running_var is not None:
        rv = running_var.double()
        f = M / (M - 1) if M > 1 else 1.0
        unb = var * f
        new = (1 - p) * rv + p * unb
        ref["running_var"] = new
        env["running_var"] = p * (e_var * f + u * unb.abs()) + u * (2 * ((1 - p) * rv).abs() + (p * unb).abs() + new.abs())
    return ref, env


def unpack_mask(mask, M, C):
    """The kernels' 1-bit ReLU mask (bit j of byte k covers flat element 8 k + j) as bool [M, C]."""
    bits = (mask.view(-1, 1).to(torch.int32) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return bits.view(M, C).bool()


def forward_apply(X, R, ref, env, relu, res_ab=None):
    """t = a x + b (+ residual), y, the ReLU decision and the ambiguous set, from coefficient refs / envelopes
    (dicts with a, b). res_ab = (ra, rb): the residual term is ra r + rb (exact fp32 inputs)."""
    u = U_FP32
    a, b, e_a, e_b = ref["a"], ref["b"], env["a"], env["b"]
    t0 = X * a + b
    e_t = X.abs() * e_a + e_b + u * ((X * a).abs() + t0.abs())
    t = t0
    if R is not None:
        if res_ab is not None:
            ra, rb = res_ab[0].double(), res_ab[1].double()
            rr = R * ra + rb
            t = t0 + rr
            e_t = e_t + u * ((R * ra).abs() + rr.abs() + t.abs())
        else:
            t = t0 + R
            e_t = e_t + u * t.abs()
    y = t.clamp_min(0) if relu else t
    out_ref = {"t": t, "y": y}
    out_env = {"t": e_t, "y": e_t + U_BF16 * y.abs()}
    if relu:
        out_ref["pos"] = t > 0
        out_ref["amb"] = ~(t.abs() > 2 * e_t)
    return out_ref, out_env


def coef_oracle(S1, S2, e_S1, e_S2, inv, e_is, w, M):
    """dbeta = S1, dgamma = S2 invstd and the dx coefficients A, B, D with their envelopes, from the backward
    sums (fp64 [C]) and the envelopes of the sums and of invstd."""
    u = U_FP32
    gm = _opt(w, S1.numel(), 1.0, S1)
    dg = S2 * inv
    e_dg = inv * e_S2 + S2.abs() * e_is + u * dg.abs()
    A = gm * inv
    B = -gm * inv * inv * dg / M
    D = -gm * inv * S1 / M
    e_A = gm.abs() * e_is + u * A.abs()
    e_B = gm.abs() * inv * inv * e_dg / M + 2 * B.abs() * e_is / inv + 6 * u * B.abs()
    e_D = gm.abs() * inv * e_S1 / M + D.abs() * e_is / inv + 5 * u * D.abs()
    return ({"dbeta": S1, "dgamma": dg, "A": A, "B": B, "D": D},
            {"dbeta": e_S1, "dgamma": e_dg, "A": e_A, "B": e_B, "D": e_D})


def backward_oracle(X, DZ, ref, env, M, C, w, path):
    """dbeta, dgamma, the coefficients A, B, D and dx from dz (fp64 [M, C]) and the forward refs / envelopes."""
    u = U_FP32
    mean, e_mean = ref["mean"], env["mean"]
    xc = X - mean
    nb = n_eff(DZ, n_path(M, C, path.u_bwd, path))
    db = DZ.sum(0)
    e_db = nb * u * DZ.abs().sum(0)
    e_S2 = nb * u * (DZ * xc).abs().sum(0) + db.abs() * e_mean
    r, e = coef_oracle(db, (DZ * xc).sum(0), e_db, e_S2, ref["invstd"], env["invstd"], w, M)
    r["dx"], e["dx"] = dx_apply(X, DZ, mean, e_mean, r, e)
    return r, e


def dx_apply(X, DZ, mean, e_mean, coef, e_coef):
    """dx = A dz + B (x - mean) + D and its envelope from coefficient refs / envelopes."""
    u = U_FP32
    A, B, D = coef["A"], coef["B"], coef["D"]
    xc = X - mean
    dx = A * DZ + B * xc + D
    e_dx = DZ.abs() * e_coef["A"] + xc.abs() * e_coef["B"] + B.abs() * e_mean + e_coef["D"] \
        + u * (2 * (A * DZ).abs() + 3 * (B * xc).abs() + 2 * D.abs()) + U_BF16 * dx.abs()
    return dx, e_dx


# ----------------------------------------------------------------------------- the training oracle
def batchnorm_oracle(x, res, w, b, running_mean, running_var, momentum, eps, relu, dy=None, res_ab=None,
                     path: Path = Path(), mask=None):
    """x, res, dy: [M, C] (bf16 / any float, promoted to double); w, b, running_*: fp32 [C] or None (the
    running statistics BEFORE the call). ``res_ab`` [2, C]: the residual enters as ra r + rb. ``mask`` (bool
    [M, C]): the ReLU decisions the backward is to use (the kernel's own); default the reference's.
    Returns (ref, env): mean, var, invstd, a, b, running_mean, running_var, t, y (, pos, amb with relu) and,
    with ``dy``, dz (= dres), dbeta, dgamma, A, B, D, dx."""
    u = U_FP32
    X = x.double()
    M, C = X.shape
    k = X[0]
    d = X - k
    nf = n_eff(d, n_path(M, C, path.u_fwd, path))
    e_S1 = nf * u * d.abs().sum(0)
    e_S2 = nf * u * (d * d).sum(0)
    d1 = d.sum(0) / M
    mean = k + d1
    var = ((X - mean) ** 2).mean(0)
    e_d1 = e_S1 / M
    e_var = e_S2 / M + 2 * d1.abs() * e_d1 + e_d1 * e_d1
    ref, env = stats_envelopes(mean, var, e_d1, e_var, M, w, b, running_mean, running_var, momentum, eps)
    R = None if res is None else res.double()
    fr, fe = forward_apply(X, R, ref, env, relu, res_ab)
    ref.update(fr)
    env.update(fe)
    if dy is not None:
        DZ = dy.double()
        if relu:
            DZ = DZ * (ref["pos"] if mask is None else mask).double()
        br, be = backward_oracle(X, DZ, ref, env, M, C, w, path)
        ref["dz"] = DZ
        ref.update(br)
        env.update(be)
    return ref, env


def eval_oracle(x, res, w, b, running_mean, running_var, eps, relu):
    """bn_fwd_eval: a = gamma rsqrtf(rv + eps), b = beta - rm a; (ref, env) with a, b, t, y (, pos, amb)."""
    u = U_FP32
    X = x.double()
    C = X.shape[1]
    gm, bt = _opt(w, C, 1.0, X), _opt(b, C, 0.0, X)
    rm, rv = running_mean.double(), running_var.double()
    inv = (rv + _f32(eps)).rsqrt()
    e_is = 3 * u * inv
    a = gm * inv
    bb = bt - rm * a
    ref = {"a": a, "b": bb}
    env = {"a": gm.abs() * e_is + u * a.abs(),
           "b": (rm * gm).abs() * e_is + 2 * u * (rm * a).abs() + u * bb.abs()}
    fr, fe = forward_apply(X, None if res is None else res.double(), ref, env, relu)
    ref.update(fr)
    env.update(fe)
    return ref, env


def tiles_stats_oracle(S, Q, e_S, e_Q, M, w, b, running_mean, running_var, momentum, eps):
    """Statistics from double-accumulated sums S = sum x, Q = sum x^2 (fp64 [C]) whose only error is that of
    the fp32 partials they were added from (e_S, e_Q)."""
    mean = S / M
    var = (Q / M - mean * mean).clamp_min(0)
    e_m = e_S / M
    e_var = e_Q / M + 2 * mean.abs() * e_m + e_m * e_m + 2.0 ** -50 * (Q / M + mean * mean)
    return stats_envelopes(mean, var, e_m, e_var, M, w, b, running_mean, running_var, momentum, eps)


# ----------------------------------------------------------------------------- stem: BN apply + ReLU + 3x3 / s2 / p1 max-pool
def _windows(t, Ho, Wo, fill):
    """t [N, H, W, C] -> [9, N, Ho, Wo, C]: element k = kh * 3 + kw of every pooling window (``fill`` outside)."""
    N, H, W, C = t.shape
    tp = torch.full((N, 2 * Ho + 1, 2 * Wo + 1, C), fill, dtype=t.dtype, device=t.device)
    tp[:, 1:H + 1, 1:W + 1] = t
    return torch.stack([tp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)])


def pool_oracle(x, ref, env):
    """x [N, H, W, C] (NHWC), ref / env: dicts with the per-channel a, b. Returns (ref, env) with the pooled y
    [N, Ho, Wo, C], the winner ``code`` (first in scan order; 15 where the max is <= 0) and ``amb``: windows
    whose best two distinct values, or whose max and 0, lie within 2 e_z (module docstring)."""
    X = x.double()
    N, H, W, C = X.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z = X * ref["a"] + ref["b"]
    e_z = X.abs() * env["a"] + env["b"] + U_FP32 * z.abs()
    win = _windows(z, Ho, Wo, float("-inf"))
    e = _windows(e_z, Ho, Wo, 0.0).amax(0)
    m = win.amax(0)
    ks = torch.arange(9, device=X.device).view(9, 1, 1, 1, 1)
    first = torch.where(win == m, ks, torch.full_like(ks, 99)).amin(0)
    second = torch.where(win == m, torch.full_like(win, float("-inf")), win).amax(0)
    amb = ((m - second) <= 2 * e) | (m.abs() <= 2 * e)
    code = torch.where(m > 0, first, torch.full_like(first, 15))
    y = m.clamp_min(0)
    return {"y": y, "code": code, "amb": amb}, {"y": e + U_BF16 * y.abs()}


def pool_bwd_oracle(dy, code, H, W):
    """dy, code [N, Ho, Wo, C] -> (dz [N, H, W, C], its envelope): every input pixel is the sum of the (at most
    four) pooled gradients whose window chose it, added in fp32 and rounded to bf16."""
    G = dy.double()
    N, Ho, Wo, C = G.shape
    out = torch.zeros(2, N, 2 * Ho + 1, 2 * Wo + 1, C, dtype=torch.float64, device=G.device)
    for k in range(9):
        kh, kw = divmod(k, 3)
        g = torch.where(code == k, G, torch.zeros_like(G))
        out[0, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += g
        out[1, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += g.abs()
    dz, sabs = out[0, :, 1:H + 1, 1:W + 1], out[1, :, 1:H + 1, 1:W + 1]
    return dz, U_BF16 * dz.abs() + 4 * U_FP32 * sabs


# ----------------------------------------------------------------------------- checks shared by CPU and GPU tests
def rounding_bias(y, y_ref):
    """Mean of (|y| - |y_ref|) / |y_ref| over |y_ref| >= 2^-6, and the number of elements it covers."""
    yr = y_ref.double().reshape(-1)
    sel = yr.abs() >= 2.0 ** -6
    n = int(sel.sum())
    if n == 0:
        return 0.0, 0
    yy = y.double().reshape(-1)[sel]
    return float(((yy.abs() - yr[sel].abs()) / yr[sel].abs()).mean()), n


class AmbiguityPool:
    """Ambiguous ReLU decisions (or pool winners) of one test case, pooled over its tensors. A tensor of fewer
    than 1 / AMBIGUOUS_CAP = 10^4 elements cannot express a share of 1e-4 (one element is already more), so
    the cap is asserted per tensor from 10^4 elements on, and for every test case on the pool of all its
    tensors' elements (``check``)."""

    def __init__(self):
        self.amb = self.total = 0

    def add(self, amb, name=""):
        n, tot = int(amb.sum()), amb.numel()
        self.amb += n
        self.total += tot
        if tot * AMBIGUOUS_CAP >= 1:
            assert n <= AMBIGUOUS_CAP * tot, f"{name}: ambiguous share {n / tot:.3g} > {AMBIGUOUS_CAP}"

    def check(self, name=""):
        assert self.amb <= AMBIGUOUS_CAP * max(self.total, 1), \
            f"{name}: ambiguous share {self.amb} / {self.total} > {AMBIGUOUS_CAP}"
        return self.amb / max(self.total, 1)


def check_relu(y, mask_bits, ref, name="", pool=None):
    """The ReLU contract: off the ambiguous set, the kernel's (y > 0) and its mask bit equal the reference
    decision; everywhere, mask bit == (y > 0); the ambiguous elements go to ``pool`` (AmbiguityPool)."""
    pos, amb = ref["pos"], ref["amb"]
    if pool is not None:
        pool.add(amb, name)
    ypos = y.double() > 0
    bad = (ypos != pos) & ~amb
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} ReLU decisions differ from the reference off the ambiguous set"
    if mask_bits is not None:
        diff = mask_bits != ypos
        assert not bool(diff.any()), f"{name}: {int(diff.sum())} mask bits differ from (y > 0)"
    return int(amb.sum())


# ----------------------------------------------------------------------------- inputs (CPU generator: same data on both sides)
def probe_rows(M, C, U, path: Path = Path(), seed=0):
    """Row 0, row M - 1, the two rows on either side of the first, a middle and the last reduce-block
    boundary, and 8 seeded random rows."""
    g = reduce_geo3(M, C, U, path.target_blocks)
    rows = {0, M - 1}
    for m in {1, g.nrow // 2, g.nrow - 1}:
        rows |= {m * g.rows_per_block - 1, m * g.rows_per_block}
    gen = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, M, (8,), generator=gen).tolist())
    return sorted(r for r in rows if 0 <= r < M)


def make_inputs(regime, M, C, seed, res=False, U=8, path: Path = Path()):
    """The input regimes of the GPU tests, generated on the CPU from a CPU generator (the GPU tests move them
    over, so tests/test_bn_oracle_cpu.py speaks about the very same data). Returns a dict of CPU tensors:
    x, dy (, r) bf16 [M, C]; w, b, rm, rv fp32 [C].
      dense:      x = bf16(0.7 + 0.3 c / C + 1.5 randn), dy ~ N(0, 1)
      large_mean: x = bf16(40 + 0.5 randn)
      probe:      every row equals row 0 and dy = 0, except on ``probe_rows`` (forward geometry U; the
                  backward's boundaries are added when they differ)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    off = 0.3 * torch.arange(C, dtype=torch.float32) / C
    if regime == "large_mean":
        x = 40.0 + 0.5 * rn(M, C)
    else:
        x = 0.7 + off + 1.5 * rn(M, C)
    dy = rn(M, C)
    r = rn(M, C) if res else None
    w = torch.rand(C, generator=g) + 0.5
    b = rn(C)
    rm = 0.5 * rn(C)
    rv = torch.rand(C, generator=g) + 0.5
    if regime == "probe":
        rows = sorted(set(probe_rows(M, C, U, path, seed)) | set(probe_rows(M, C, path.u_bwd, path, seed)))
        keep = torch.zeros(M, dtype=torch.bool)
        keep[rows] = True
        x = torch.where(keep[:, None], x, x[0:1].expand(M, C))
        dy = torch.where(keep[:, None], dy, torch.zeros_like(dy))
    out = {"x": x.bfloat16(), "dy": dy.bfloat16(), "w": w, "b": b, "rm": rm, "rv": rv}
    if res:
        out["r"] = r.bfloat16()
    return out


# ----------------------------------------------------------------------------- the cases both test files run
class Case(NamedTuple):
    name: str
    regime: str
    M: int
    C: int
    relu: bool
    res: bool
    wb: bool          # weight and bias present
    momentum: float
    path: Path
    seed: int


WIDTHS = [64, 128, 192, 256, 320, 512, 1024, 4096]
COMBOS = [(False, False, True), (True, False, True), (False, True, True), (True, True, True), (True, True, False)]


def small_ms(C, U=8):
    """M in {1, 3, R - 1, R, R + 1, 2 U R + 1}: below / at / past one pass, and one row past two iterations."""
    R = reduce_geo3(1, C, U).R
    return sorted({1, 3, R - 1, R, R + 1, 2 * U * R + 1})


def width_cases(C):
    """Every (M, relu, res, weight/bias, regime) of one width; momentum 1 without ReLU, 0.1 with it."""
    out = []
    for M in small_ms(C):
        for relu, res, wb in COMBOS:
            for regime in ("dense", "probe"):
                out.append(Case(f"w C={C} M={M} relu={int(relu)} res={int(res)} wb={int(wb)} {regime}", regime, M, C,
                                relu, res, wb, 0.1 if relu else 1.0, Path(), 1000 * C + M))
    return out


def find_partition_m(C, U, nfull, target_blocks):
    """The smallest M whose reduce partition (U rows in flight) has >= 2 blocks, a ragged last block,
    rows_per_block no multiple of U R (nor of R) and exactly ``nfull`` full pipelined trips."""
    R = reduce_geo3(1, C, U).R
    for M in range(nfull * U * R, 64 * (nfull + 2) * U * R):
        g = reduce_geo3(M, C, U, target_blocks)
        if (g.nrow >= 2 and M % g.rows_per_block != 0 and g.rows_per_block % g.R != 0
                and g.rows_per_block // (U * g.R) == nfull):
            return M
    raise AssertionError((C, U, nfull, target_blocks))


def partition_cases():
    """Partition edges: C in {64, 512, 1024}; nfull in {1, 2, 3} for the forward (U = 8) and for the backward
    (U = 4); three blocks per chunk (target_blocks = 3 nchunks) so that rows_per_block can exceed 2 U R."""
    out = []
    for C in (64, 512, 1024):
        tb = 3 * (C // chunk3(C))
        path = Path(5, tb, 8, 4)
        for U in (8, 4):
            for nfull in (1, 2, 3):
                M = find_partition_m(C, U, nfull, tb)
                for regime in ("probe", "dense"):
                    out.append(Case(f"p C={C} U={U} nfull={nfull} M={M} {regime}", regime, M, C, True, True, True,
                                    0.1, path, 7 * C + M))
    return out


def slab_cases(variant=5):
    """More than 128 slabs (bn_tune(variant, 512, 2, 2)): C = 64, M = 16,520 -> nrow = 130; C = 512,
    M = 2,100 -> nrow = 132. The first dense case is also the >= 1e5-element rounding-mode tensor."""
    path = Path(variant, 512, 2, 2)
    out = []
    for C, M in ((64, 16520), (512, 2100)):
        for regime in ("probe", "dense"):
            out.append(Case(f"s v{variant} C={C} M={M} {regime}", regime, M, C, True, False, True, 0.1, path, C + M))
    return out


def variant3_cases():
    """The in-kernel finalize: nrow in {1, 2, 16, 17, 33, 130} (no ticket; level 1 only; exactly one group;
    a one-block last group; three groups with a ragged last one; 9 groups) on C = 64 and C = 512."""
    out = []
    for C in (64, 512):
        R = reduce_geo3(1, C, 2).R
        for nrow in (1, 2, 16, 17, 33, 130):
            M = 4 * R * nrow - (3 if nrow > 1 else 0)  # U = 2: max_rows = ceil(M / (4 R)) = nrow
            path = Path(3, 512, 2, 2)
            for regime in ("probe", "dense"):
                out.append(Case(f"v3 C={C} nrow={nrow} M={M} {regime}", regime, M, C, True, True, True, 0.1, path,
                                3 * C + M))
    return out


def large_mean_case():
    return Case("large_mean C=64 M=8192", "large_mean", 8192, 64, False, False, False, 1.0, Path(), 40)


def make_res_ab(C):
    """The (ra, rb) [2, C] of the deferred-residual cases."""
    g = torch.Generator().manual_seed(C)
    return torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)]).contiguous()


def apply_cases():
    """The cases of the apply-kernel tests, by test: the grid-stride second trip (more than 65,536 vectors on
    the fixed and the per-vector coefficient path), the deferred-residual form, the apply kernels fed the
    oracle's coefficients, eval, and the backward without dgamma."""
    combos = [(False, False), (True, False), (True, True), (False, True)]
    return {
        "wgs1": [Case(f"wgs1 C={C} M={M}", "dense", M, C, True, True, True, 0.1, Path(), C + M)
                 for C, M in ((64, 8200), (192, 2740))],
        "res_ab": [Case(f"res_ab C={C}", "dense", 777, C, True, True, True, 0.1, Path(), C) for C in (64, 320)],
        "coef": [Case(f"coef C={C} relu={int(relu)} res={int(res)}", "dense", 1031, C, relu, res, True, 0.1, Path(), C)
                 for C in (64, 192) for relu, res in combos],
        "eval": [Case(f"eval C={C} res={int(res)} wb={int(wb)}", "dense", 515, C, True, res, wb, 0.1, Path(), C)
                 for C in (64, 192) for res, wb in ((False, True), (True, True), (True, False), (False, False))],
        "nodgamma": [Case(f"nodgamma C={C}", "dense", 999, C, True, True, True, 0.1, Path(), C) for C in (64, 320)],
    }


STEM_SHAPES = [(2, 64, 7, 9), (3, 64, 16, 16), (1, 64, 1, 1), (2, 64, 2, 3)]  # (N, C, H, W)


def stem_inputs(shape):
    """make_inputs for a stem shape: x is [N H W, C], to be viewed as NHWC."""
    N, C, H, W = shape
    return make_inputs("dense", N * H * W, C, 17 * N * H * W + 1)


def all_cases():
    out = [c for C in WIDTHS for c in width_cases(C)]
    return out + partition_cases() + slab_cases(5) + slab_cases(3) + variant3_cases() + [large_mean_case()]
