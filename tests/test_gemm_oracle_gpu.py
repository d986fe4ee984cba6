"""The Linear GEMM kernels (csrc/kernels/gemm.hip: gemm_nt on bf16, gemm_nt_fp8 on e4m3 operands with its
split-K reduce) against the oracles of tests/gemm_oracle.py, whose docstring carries the analysis:
  (a) integer operands (ternary, and one-hot probes in both roles): the output equals the exact float64 product
      rounded once to bf16, bit for bit;
  (b) real-valued operands, randn and nearly cancelling: every element inside
      U_BF16 |ref| + 2 (K + ksplit + 2) U_FP32 ((sa sb) |A| |B|^T + |bias|);
  (c) the GELU epilogue judged from the kernel's own H: inside U_BF16 |G_ref| + 2^-21 |v|.
The shapes are gemm_oracle's twelve cases: M = 1, M tails, odd K-step counts, partial tile groups, a grid that
is no multiple of 8, the 256-wide tile (asserted through the gemm_nt_tile_n query), even and uneven split-K
(asserted through gemm_nt_fp8_ksplit). tests/test_gemm_oracle_cpu.py runs an emulation and planted faults
through the same checks. Every comparison prints ``ratio <name> <value>``; with PDT_GEMM_ORACLE_RATIOS=<path>
the worst per name are written there (kept in profiles/r14/gemm_oracle_ratios.txt)."""
import functools
import os

import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}

# (name, epi, bias dtype, tanh form)
BF16_VARIANTS = [("none", 0, None, False), ("bias_bf16", 1, "bf16", False), ("bias_f32", 1, "f32", False),
                 ("gelu_erf", 2, "f32", False), ("gelu_tanh", 2, "bf16", True)]
FP8_BIAS = [None, "f32", "bf16"]


def _C():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PDT_GEMM_ORACLE_RATIOS")
    if path and RECORD:
        with open(path, "w") as f:
            for name in sorted(RECORD):
                f.write(f"{name:<58} {RECORD[name]:.4g}\n")


def _exact(got, ref, name, **kw):
    try:
        go.assert_exact(got, ref, name, record=RECORD, **kw)
    finally:
        print(f"ratio {name} mismatches {RECORD.get(name)}")


def _within(got, ref, env, name):
    try:
        go.assert_within(got, ref, env, 1.0, go.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


def _cast_bias(bias, kind):
    return bias.to(DEV).bfloat16() if kind == "bf16" else bias.to(DEV).float()


def _store(x, fp8):
    return x.to(DEV).to(torch.float8_e4m3fn if fp8 else torch.bfloat16).contiguous()


def _shape(case):
    return go.BF16_CASES[case] if case in go.BF16_CASES else go.FP8_CASES[case]


@functools.lru_cache(maxsize=2)
def _ternary(case):
    """The case's ternary operands as the kernel takes them and their exact product (float64, on the device),
    computed once and shared by the epilogue variants."""
    M, N, K = _shape(case)
    fp8 = case in go.FP8_CASES
    a, b = go.ternary(M, N, K)
    a, b = _store(a, fp8), _store(b, fp8)
    ref = go.f64(a) @ go.f64(b).t()
    assert ref.abs().max() <= go.TERNARY_MAX  # a precondition on the inputs
    return a, b, ref


@functools.lru_cache(maxsize=2)
def _real(case, kind):
    M, N, K = _shape(case)
    fp8 = case in go.FP8_CASES
    a, b = go.real_operands(M, N, K, kind, fp8)
    a, b = _store(a, fp8), _store(b, fp8)
    return (a, b) + go.products(a, b)


def _tile_n(case):
    M, N, _ = _shape(case)
    bn = _C().gemm_nt_tile_n(M, N)
    assert bn in (128, 256), bn
    if case in go.EXPECT_BN256:
        assert bn == 256, f"case {case} was to reach the 256-wide tile, the kernel reports {bn}"
    return bn


def _onehot_probes(case, run, bias, scale, name, bn):
    """Both roles, every pass. ``run(a, b)`` -> C for fp32 operand values on the device."""
    M, N, K = _shape(case)
    fp8 = case in go.FP8_CASES
    kstep = go.KSTEP["fp8" if fp8 else "bf16"]
    for onehot_is_b, role in ((True, "onehot-B"), (False, "onehot-A")):
        R, Rc = (N, M) if onehot_is_b else (M, N)
        coded = go.position_coded(Rc, K, fp8, device=DEV)
        for p in range(go.onehot_passes(R, K)):
            rows, k, sign = go.onehot(R, K, p, device=DEV)
            want = scale * go.onehot_ref(coded, k, sign, onehot_is_b)
            if bias is not None:
                want = want + go.f64(bias)
            got = run(coded, rows) if onehot_is_b else run(rows, coded)
            _exact(got, want, f"case{case:02d} {name} {role}", bn=bn, kstep=kstep,
                   k_of=(lambda m, n: k[n]) if onehot_is_b else (lambda m, n: k[m]))


# ----------------------------------------------------------------------------- the paths the cases are named for
def test_cases_reach_the_paths_they_name():
    C_ = _C()
    for case, (M, N, _) in go.EXPECT_BN256.items():
        assert C_.gemm_nt_tile_n(M, N) == 256, case
    for case, ks in go.EXPECT_KSPLIT.items():
        assert C_.gemm_nt_fp8_ksplit(*go.FP8_CASES[case]) == ks, case
    for case in (7, 8, 12):
        assert C_.gemm_nt_fp8_ksplit(*go.FP8_CASES[case]) == 1, case
    assert C_.gemm_nt_tile_n(257, 384) == 128  # N % 256 != 0
    assert C_.gemm_nt_tile_n(256, 100) == 0 and C_.gemm_nt_tile_n(0, 128) == 0  # not served
    assert C_.gemm_nt_fp8_ksplit(256, 128, 64) == 1


# ----------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("variant", BF16_VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("case", sorted(go.BF16_CASES))
def test_gemm_nt_exact(case, variant):
    name, epi, bkind, tanh = variant
    M, N, K = _shape(case)
    C_, bn = _C(), _tile_n(case)
    a, b, ref = _ternary(case)
    bias = None
    if epi == 1:
        bias = _cast_bias(go.exact_bias(N), bkind)
    elif epi == 2:
        bias = _cast_bias(go.bias_bands(N), bkind)
    out = C_.gemm_nt(a, b, bias, epi, tanh)
    _exact(out[0], ref + go.f64(bias) if epi == 1 else ref, f"case{case:02d} {name} ternary", bn=bn)
    if epi == 2:
        _, gref, genv = go.gelu_oracle(out[0], bias, tanh)
        _within(out[1], gref, genv, f"case{case:02d} {name} ternary G")
        return
    _onehot_probes(case, lambda x, y: C_.gemm_nt(_store(x, False), _store(y, False), bias, epi, False)[0],
                   bias, 1.0, name, bn)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", go.ENVELOPE_BF16)
def test_gemm_nt_envelope(case, kind):
    M, N, K = _shape(case)
    C_ = _C()
    _tile_n(case)
    a, b, P, E = _real(case, kind)
    if kind == "cancel":
        assert P.abs().median() < E.median() / 32  # the reference nearly cancels (inputs only)
    rb = torch.randn(N, generator=torch.Generator().manual_seed(case))
    for name, epi, bkind, tanh in BF16_VARIANTS:
        bias = None if epi == 0 else _cast_bias(rb if epi == 1 else go.bias_bands(N), bkind)
        out = C_.gemm_nt(a, b, bias, epi, tanh)
        ref, env = go.gemm_envelope(P, E, K, bias if epi == 1 else None)
        _within(out[0], ref, env, f"case{case:02d} {name} {kind} C")
        if epi == 2:
            v, gref, genv = go.gelu_oracle(out[0], bias, tanh)
            _within(out[1], gref, genv, f"case{case:02d} {name} {kind} G")
            if kind == "randn":  # H verified just above: the tails and the centre are all populated
                assert min(go.band_counts(v)) > 0, go.band_counts(v)


# ----------------------------------------------------------------------------- fp8
def _fp8_scales(sa, sb):
    ta, tb = torch.tensor([sa], device=DEV), torch.tensor([sb], device=DEV)
    return ta, tb, float(ta.double() * tb.double())


def _fp8_ksplit(case, bkind):
    """The K splits this call runs with: the binding splits only without a bias."""
    ks = _C().gemm_nt_fp8_ksplit(*_shape(case)) if bkind is None else 1
    if bkind is None and case in go.EXPECT_KSPLIT:
        assert ks == go.EXPECT_KSPLIT[case], f"case {case} was to run {go.EXPECT_KSPLIT[case]} splits, reports {ks}"
    return ks


@pytest.mark.parametrize("bkind", FP8_BIAS, ids=lambda b: f"bias_{b}")
@pytest.mark.parametrize("case", sorted(go.FP8_CASES))
def test_gemm_nt_fp8_exact(case, bkind):
    M, N, K = _shape(case)
    C_, bn = _C(), _tile_n(case)
    _fp8_ksplit(case, bkind)
    a, b, ref = _ternary(case)
    sa, sb, sc = _fp8_scales(go.FP8_SA, go.FP8_SB)
    assert sc == 2.0
    bias = None if bkind is None else _cast_bias(go.exact_bias(N), bkind)
    name = f"fp8 bias_{bkind}"
    out = C_.gemm_nt_fp8(a, b, sa, sb, bias)
    _exact(out, sc * ref if bias is None else sc * ref + go.f64(bias), f"case{case:02d} {name} ternary", bn=bn, kstep=128)
    _onehot_probes(case, lambda x, y: C_.gemm_nt_fp8(_store(x, True), _store(y, True), sa, sb, bias), bias, sc, name, bn)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", go.ENVELOPE_FP8)
def test_gemm_nt_fp8_envelope(case, kind):
    M, N, K = _shape(case)
    C_ = _C()
    _tile_n(case)
    a, b, P, E = _real(case, kind)
    if kind == "cancel":
        assert P.abs().median() < E.median() / 32
    sa, sb, sc = _fp8_scales(*go.fp8_real_scales(K))
    rb = torch.randn(N, generator=torch.Generator().manual_seed(case))
    for bkind in FP8_BIAS:
        bias = None if bkind is None else _cast_bias(rb, bkind)
        ks = _fp8_ksplit(case, bkind)
        out = C_.gemm_nt_fp8(a, b, sa, sb, bias)
        ref, env = go.gemm_envelope(P, E, K, bias, sc, ks)
        _within(out, ref, env, f"case{case:02d} fp8 bias_{bkind} {kind} C")
