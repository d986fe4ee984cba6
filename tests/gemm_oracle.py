"""Exact and envelope oracles for the Linear GEMM kernels (csrc/kernels/gemm.hip: ``gemm_nt`` on bf16 and
``gemm_nt_fp8`` on e4m3 operands). A helper module imported by plain name, like oracle_envelope.py, whose
comparator (``assert_within``) and constants (U_BF16 = 2^-8, U_FP32 = 2^-24, FLOOR = 2^-126) it reuses;
tests/test_gemm_oracle_cpu.py proves on the CPU that it is sharp, tests/test_gemm_oracle_gpu.py runs the kernels.

The kernel. C[M, N] = A[M, K] B[N, K]^T in 256 x BN tiles (BN = 128 or 256), one K-step of 64 bf16 (128 e4m3)
values at a time, fp32 accumulators in the MFMA unit. Epilogues: none; + bias (added in fp32, one rounding to
bf16); H = A B^T rounded to bf16 and G = gelu(bf16(H) + bias). fp8: the accumulators are multiplied by sa sb in
fp32 before the bias; without a bias K may be cut into ``ksplit`` runs of K-steps [s nkt / ksplit,
(s + 1) nkt / ksplit) whose fp32 partial tiles a second kernel adds in fixed order and rounds once.

(a) Exact operands: bit for bit. Every product and every partial sum of integer operands is an integer; while
all of them stay below 2^24 in magnitude they are exact fp32 numbers, so the accumulators hold the exact result
whatever the order of summation, inside the MFMA unit or across K-steps and splits. The one rounding left is the
round-to-nearest-even conversion to bf16 at the store, which ``ref.to(torch.bfloat16)`` of the exact float64
result performs too (the exact value is an fp32 number, so a conversion that passes through fp32 rounds once).
The kernel's output must therefore EQUAL the reference; there is no tolerance. Two fixtures:

  * Ternary operands, ``ternary``: entries in {-1, 0, +1}, nonzero with probability p = min(1, 32 / sqrt(K)),
    from a generator seeded with M + N + K. An output is a sum of K p^2 <= 1024 terms +-1: an integer of
    standard deviation <= 32. 256 is eight standard deviations, and the tests assert |ref| <= 256 on the
    REFERENCE (a precondition on the inputs, never on the kernel): such integers are bf16 numbers (8
    significant bits cover 0..256), so even the store is exact when there is no bias. One product dropped,
    counted twice or paired with the wrong partner moves an output by at least 1.
  * One-hot probes, ``onehot`` and ``position_coded``: one operand's rows are +-e_k, k = (row + pass R) mod K
    over ceil(K / R) passes, so that every k is selected in some pass (R = that operand's row count); the other
    is the position code ((31 row + 17 k) mod 251) - 125 (8 bits: bf16-exact), for e4m3 ((31 row + 17 k) mod 31)
    - 15 (4 bits: e4m3-exact). C[m, n] = +-code[., k]: the reference is a gather with no GEMM in it, exact under
    ANY accumulation arithmetic because one term of each sum is nonzero, and a mismatch names the tile, the
    row and the k (hence the K-step and the split) that went wrong. Both roles are run: B one-hot and A coded,
    A one-hot and B coded.

  Bias for the exact cases, ``exact_bias``: multiples of 1/4 in [-4, 4] (bf16-exact). acc * sc + bias is then
  a multiple of 1/4 below 2^10: exact in fp32, rounded once. fp8 scales: sa = 0.5, sb = 4, powers of two whose
  product 2 is not 1 (a forgotten or doubled scale shows), so scaled accumulators and split-K partials stay
  exact and the reduce kernel's sum is exact as well.

  One supposition: that v_mfma_scale_f32_16x16x128_f8f6f4 adds 128 products of small integers (|product| <= 225,
  sums below 2^15) without loss. The fp8 exact test measures it; profiles/r14/gemm_oracle_ratios.txt says what
  it found.

(b) Real-valued operands: an envelope. ref = (sa sb) A B^T + bias in float64 on the stored operand values, and
    env_C = U_BF16 |ref| + 2 (K + ksplit + 2) U_FP32 ((sa sb) |A| |B|^T + |bias|),        c = 1, floor = FLOOR.
  First term: the single rounding of the output to bf16 (|fl(x) - x| <= 2^-8 |x|, reached only just above a
  power of two; that x is the fp32 result and not ref changes it at second order). Second term: a sum of K
  products in fp32, in ANY order, errs by at most (K - 1) U_FP32 sum |a_k b_k| to first order (the products of
  bf16 or e4m3 numbers are exact in fp32); the scale multiply, the ksplit - 1 adds of the reduce kernel and
  the bias add are K + ksplit + 2 roundings at most, each relative to a quantity bounded by the bracket. The
  factor 2 allows for accumulation inside the MFMA unit that need not be IEEE sequential summation (wider or
  truncated internal alignment). The bound uses absolute values, so it stays meaningful where ref cancels:
  the ``cancel`` operands have ref ~ 2^-7 of |A| |B|^T, where a relative tolerance would pass anything. The
  constants come from this analysis; none is fitted to what the kernel returns.

(c) The GELU epilogue. H is verified by (a) or (b). G is then judged from the kernel's OWN H: with
  v = H_kernel + bias in float64 and G_ref = gelu64(v) = v Phi(v) (erf form) or v / (1 + e^(-2u)),
  u = sqrt(2/pi) (v + 0.044715 v^3) (tanh form),
    env_G = U_BF16 |G_ref| + 2^-21 |v|,                                                    c = 1.
  The first term is the rounding of G to bf16. The second is absolute in the CDF factor F (G = v F / 2, F in
  [0, 2]), and it is needed: the kernel forms F = 1 + erf_AS(v / sqrt 2) or F = 1 + (1 - 2 / (1 + e^(2u))), and
  both cancel in the negative tail, so F carries an absolute error of a few 2^-24 however small G is. An
  error dF in F moves G by |v| dF / 2, so 2^-21 |v| admits dF <= 2^-20 = 16 units of 2^-24. What uses them:
    erf form:  Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 = 2.5 units; the fp32 rounding of x = |v| / sqrt 2
               (1.5 U relative) through x erf'(x) <= 0.48: 0.7 units; the rounding of t = 1 / (1 + 0.3275911 x)
               and of the Horner steps, scaled by e^(-x^2) <= 1 and zero at x = 0: a few units at |v| ~ 1 and
               none in the tails; __expf's argument rounding, relative x^2 2^-23 on e^(-x^2), with
               x^2 e^(-x^2) <= 0.37: 0.7 units; the roundings of 1 - p e^(-x^2) and of 1 +- e: 0.5 + 1 units.
    tanh form: u is four fp32 operations (~4 U relative) and __expf rounds its argument (relative
               |2u| 2^-24 on E = e^(2u), |2u| <= 17 before E saturates F): together <= 6 |2u| 2^-24 on E, through
               dF / (dE / E) = 2 E / (1 + E)^2 <= 1/2, and |2u| 2 E / (1 + E)^2 <= 0.45: 2.7 units; the roundings of
               1 + E and of the reciprocal (2 / (1 + E) <= 2): 2 + 2 units; of 1 - 2 r and 1 + t: 1 + 2 units.
  Both stay below 16 units. The fp32 add bf16(H) + bias is one more rounding, relative 2^-24 on v through
  G' <= 1.13: 2^-23.8 |v|, a fifth of the term. Where F is not small the first term dominates by 2^12 and
  none of this matters; the absolute term decides only for v < -3.5, where everything scaled by e^(-x^2) or
  E has vanished and one or two units remain. ``bias_bands`` puts columns at v in [-9, -3] and [3, 9] (bias
  -+6 on H ~ N(0, 1.5^2)) as well as near zero and at randn.

What the GPU found is recorded in profiles/r14/gemm_oracle_ratios.txt.
"""
from __future__ import annotations

import math

import torch

from oracle_envelope import FLOOR, U_BF16, U_FP32, assert_within  # noqa: F401  (re-exported)

BM, GROUP = 256, 4            # tile rows; A bands per tile group (gemm.hip kBM, kGroup)
KSTEP = {"bf16": 64, "fp8": 128}
TERNARY_MAX = 256
FP8_SA, FP8_SB = 0.5, 4.0     # exact cases: powers of two, product 2
GELU_ABS = 2.0 ** -21

# (M, N, K) and what each reaches
BF16_CASES = {
    1: (1, 128, 64),          # one K-step, every A row clamped onto row 0
    2: (255, 128, 128),       # two K-steps, tail of 255
    3: (257, 384, 192),       # three K-steps (odd), ntm = 2 (gsize 2), N % 256 != 0, grid 6
    4: (1300, 256, 320),      # five K-steps, a full group of 4 A bands and a partial group of 2
    5: (4400, 3840, 192),     # 18 x 15 = 270 tiles of 256^2: BN = 256, last group of 2, grid % 8 != 0
    6: (300, 128, 4096),      # 64 K-steps, long stage alternation
}
FP8_CASES = {
    7: (1, 128, 128),         # one K-step
    8: (257, 384, 384),       # three K-steps, no split
    9: (200, 128, 2048),      # ksplit 2, even (8 + 8)
    10: (200, 128, 3200),     # ksplit 3, uneven (8, 8, 9)
    11: (300, 256, 17280),    # ksplit 16 over 135 K-steps, uneven, M tail in the partial-tile store
    12: (4400, 3840, 384),    # BN = 256 on the fp8 path
}
ENVELOPE_BF16 = (2, 3, 4, 6)
ENVELOPE_FP8 = (8, 10, 11)
EXPECT_BN256 = {5: BF16_CASES[5], 12: FP8_CASES[12]}
EXPECT_KSPLIT = {9: 2, 10: 3, 11: 16}


def f64(t):
    """Any operand tensor (bf16, e4m3, fp32) as float64, exactly."""
    return t.float().double()


# ----------------------------------------------------------------------------- geometry (gemm.hip's own)
def split_steps(nkt, ksplit):
    """K-step ranges [(first, end)] of the splits: kb = s nkt / ksplit in integer arithmetic."""
    return [(s * nkt // ksplit, (s + 1) * nkt // ksplit) for s in range(ksplit)]


def tile_origin(tid, M, N, bn, full_groups=False):
    """(m0, n0) of tile id ``tid``: groups of GROUP A bands, bands fastest, then N tiles. ``full_groups`` plants
    the fault of treating the last, partial group as if it had GROUP bands."""
    ntn, ntm = N // bn, (M + BM - 1) // BM
    gband = (tid // (GROUP * ntn)) * GROUP
    gsize = GROUP if full_groups else min(ntm - gband, GROUP)
    gi = tid % (GROUP * ntn)
    return (gband + gi % gsize) * BM, (gi // gsize) * bn


# ----------------------------------------------------------------------------- (a) exact fixtures
def ternary(M, N, K, seed=None):
    """A [M, K], B [N, K] fp32 on the CPU with entries in {-1, 0, +1}, nonzero with probability min(1, 32 / sqrt K)."""
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    p = min(1.0, 32.0 / math.sqrt(K))

    def draw(R):
        u = torch.rand(R, K, generator=g)
        return torch.where(u < p / 2, -1.0, torch.where(u < p, 1.0, 0.0))
    return draw(M), draw(N)


def exact_bias(N, device="cpu"):
    """Multiples of 1/4 in [-4, 4], fp32 (bf16-exact)."""
    n = torch.arange(N, device=device)
    return ((7 * n) % 33 - 16).float() / 4


def position_coded(R, K, fp8=False, device="cpu"):
    """[R, K] fp32: ((31 r + 17 k) mod 251) - 125, or mod 31 minus 15 for e4m3."""
    r = torch.arange(R, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    mod, off = (31, 15) if fp8 else (251, 125)
    return ((31 * r + 17 * k) % mod - off).float()


def onehot_passes(R, K):
    return (K + R - 1) // R


def onehot(R, K, p, device="cpu"):
    """Pass ``p``: rows +-e_k(r) with k(r) = (r + p R) mod K. Returns (rows [R, K] fp32, k [R] int64, sign [R] fp32)."""
    r = torch.arange(R, device=device)
    k = (r + p * R) % K
    sign = torch.where((r + p) % 3 == 0, -1.0, 1.0)
    rows = torch.zeros(R, K, device=device)
    rows[r, k] = sign
    return rows, k, sign


def onehot_ref(coded, k, sign, onehot_is_b=True):
    """The exact product as a gather, float64 [M, N]: B one-hot: C[m, n] = sign[n] A[m, k(n)]; A one-hot:
    C[m, n] = sign[m] B[n, k(m)]."""
    c = coded.double()
    if onehot_is_b:
        return c[:, k] * sign.double()[None, :]
    return c[:, k].t() * sign.double()[:, None]


def mismatches(got, want):
    """(number of elements of ``got`` that differ from ``want``, (m, n) of the first or None). NaN differs."""
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return 0, None
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    return n, (i // got.shape[1], i % got.shape[1])


def assert_exact(got, ref64, name="", record=None, bn=128, kstep=64, k_of=None):
    """``got`` (bf16) must equal ``ref64.to(torch.bfloat16)``. ``k_of(m, n)``: the k a one-hot probe selected
    there, named in the report with its K-step. ``record`` collects the mismatch count per name."""
    want = ref64.to(torch.bfloat16)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (name, got.shape, got.dtype, want.shape)
    n, at = mismatches(got, want)
    if record is not None:
        record[name] = max(record.get(name, 0), n)
    if n:
        m, c = at
        where = f"tile ({m // BM}, {c // bn}), row {m % BM}, column {c % bn}"
        if k_of is not None:
            k = int(k_of(m, c))
            where += f", k = {k} (K-step {k // kstep})"
        raise AssertionError(f"{name}: {n} of {got.numel()} elements differ; first at ({m}, {c}): {where}: "
                             f"got {float(got[m, c]):.9g}, want {float(want[m, c]):.9g}")
    return 0


# ----------------------------------------------------------------------------- (b) envelope
def real_operands(M, N, K, kind="randn", fp8=False, seed=0):
    """fp32 CPU operands already holding bf16- (e4m3-) representable values. ``randn``: A ~ N(0, 1), B ~
    N(0, 1.5^2 / K), so that A B^T ~ N(0, 1.5^2) (e4m3: A, B ~ 8 N(0, 1), 4 N(0, 1), to be used with scales whose
    product brings the result back to that range). ``cancel``: the second half of K repeats the first with B
    negated, except that one entry in 64 of B's second half is redrawn: ref is ~2^-7 of |A| |B|^T."""
    g = torch.Generator().manual_seed(1000 * seed + M + N + K + (7 if kind == "cancel" else 0) + (13 if fp8 else 0))
    if fp8:
        q = lambda x: x.clamp(-440, 440).to(torch.float8_e4m3fn).float()  # noqa: E731
        sa_, sb_ = 8.0, 4.0
    else:
        q = lambda x: x.to(torch.bfloat16).float()  # noqa: E731
        sa_, sb_ = 1.0, 1.5 / math.sqrt(K)
    kk = K // 2 if kind == "cancel" else K
    a = q(torch.randn(M, kk, generator=g) * sa_)
    b = q(torch.randn(N, kk, generator=g) * sb_)
    if kind == "cancel":
        redraw = torch.rand(N, kk, generator=g) < 1.0 / 64
        b2 = torch.where(redraw, q(torch.randn(N, kk, generator=g) * sb_), -b)
        a, b = torch.cat([a, a], 1), torch.cat([b, b2], 1)
    return a.contiguous(), b.contiguous()


def fp8_real_scales(K):
    """Dequantisation scales for ``real_operands(fp8=True)``: not powers of two; result ~ N(0, 1.5^2)."""
    return 0.03, 1.5 / (0.03 * 8.0 * 4.0 * math.sqrt(K))


def products(a, b):
    """(A B^T, |A| |B|^T) in float64."""
    A, B = f64(a), f64(b)
    return A @ B.t(), A.abs() @ B.abs().t()


def gemm_envelope(P, E, K, bias=None, scale=1.0, ksplit=1):
    """(ref, env_C) from ``products``: ref = scale P + bias."""
    ref, mag = scale * P, abs(scale) * E
    if bias is not None:
        ref, mag = ref + f64(bias), mag + f64(bias).abs()
    return ref, U_BF16 * ref.abs() + 2 * (K + ksplit + 2) * U_FP32 * mag


# ----------------------------------------------------------------------------- (c) GELU
def gelu64(v, tanh_form):
    """float64 GELU without cancellation in the negative tail: v erfc(-v / sqrt 2) / 2, or v / (1 + e^(-2u))."""
    if tanh_form:
        u = 0.7978845608028654 * (v + 0.044715 * v * v * v)
        return v / (1.0 + torch.exp(-2.0 * u))
    return 0.5 * v * torch.special.erfc(-v * 0.7071067811865476)


def gelu_oracle(h_kernel, bias, tanh_form):
    """(v, G_ref, env_G) from the kernel's own bf16 H and the bias."""
    v = f64(h_kernel) + f64(bias)
    ref = gelu64(v, tanh_form)
    return v, ref, U_BF16 * ref.abs() + GELU_ABS * v.abs()


def bias_bands(N, seed=0):
    """fp32 [N] on the CPU: column n % 4 = 0 near zero, 1 around -6, 2 around +6, 3 randn."""
    g = torch.Generator().manual_seed(77 + seed + N)
    r = torch.randn(N, generator=g)
    n = torch.arange(N) % 4
    return torch.where(n == 0, 0.25 * r, torch.where(n == 1, -6 + 0.5 * r, torch.where(n == 2, 6 + 0.5 * r, r)))


def band_counts(v):
    """How many v lie in [-9, -3], near zero (|v| < 0.5) and in [3, 9]."""
    return int(((v >= -9) & (v <= -3)).sum()), int((v.abs() < 0.5).sum()), int(((v >= 3) & (v <= 9)).sum())
