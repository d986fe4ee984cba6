"""The GEMM oracle (tests/gemm_oracle.py) on the CPU, before any GPU runs:
  * the fixtures' preconditions: |ref| <= 256 for the ternary operands of all twelve shapes, every k selected by
    the one-hot passes in both roles, the split-K ranges the shapes are named for;
  * a torch emulation of the kernel's arithmetic (fp32 partial products per K-step of 64, or 128 for fp8,
    accumulated in fp32; split partials scaled and summed in fixed order; bias added in fp32; one rounding to
    bf16; H rounded before GELU, whose fp32 formulas are the kernel's) equals the exact references bit for bit
    and lies inside the envelopes (b) and (c) at c = 1;
  * eight planted faults are each rejected by the exact test, by the envelope and, where a probe can see
    them, by the one-hot probes, and every element that fails lies inside the region the fault damaged."""
import functools
import re

import pytest
import torch

import gemm_oracle as go

NAN = float("nan")


# ----------------------------------------------------------------------------- the emulation
def gelu32(v, tanh_form):
    """gemm.hip's gelu_f in fp32 tensor arithmetic (torch.exp for __expf)."""
    if tanh_form:
        u = 0.7978845608028654 * (v + 0.044715 * v * v * v)
        t = 1.0 - 2.0 / (1.0 + torch.exp(2.0 * u))
        return 0.5 * v * (1.0 + t)
    x = v.abs() * 0.7071067811865476
    t = 1.0 / (1.0 + 0.3275911 * x)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    e = 1.0 - p * torch.exp(-x * x)
    return 0.5 * v * (1.0 + torch.copysign(e, v))


def _tile(ti, tj, M, N, bn):
    return slice(ti * go.BM, min((ti + 1) * go.BM, M)), slice(tj * bn, (tj + 1) * bn)


def emulate(a, b, kstep, bias=None, epi=0, tanh_form=False, scale=None, ksplit=1, bn=128, fault=None):
    """(C, G or None), bf16. a [M, K], b [N, K] fp32 holding the operand values. ``fault``: a dict with "kind"
    (BF16_FAULTS and the split-K and GELU tests below) and its parameters."""
    f = fault or {"kind": None}
    kind = f["kind"]
    M, K = a.shape
    N = b.shape[0]
    assert a.dtype == b.dtype == torch.float32 and K % kstep == 0 and N % bn == 0
    parts = []
    for s, (t0, t1) in enumerate(go.split_steps(K // kstep, ksplit)):
        steps = list(range(t0, t1))
        if kind == "split_drop_last" and s == f["split"]:
            steps = steps[:-1]
        if kind == "split_last_twice" and s == f["split"]:
            steps = steps + steps[-1:]
        acc = torch.zeros(M, N)
        for t in steps:
            p = a[:, t * kstep:(t + 1) * kstep] @ b[:, t * kstep:(t + 1) * kstep].t()
            if kind == "skip_step" and t == f["step"]:
                p[_tile(*f["tile"], M, N, bn)] = 0.0
            acc = acc + p
        parts.append(acc * scale if scale is not None else acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    bv = torch.zeros(N) if bias is None else bias.float()
    if kind == "bias_shift":
        bv = torch.roll(bv, 4)
    G = None
    if epi == 2:
        C = acc.to(torch.bfloat16)
        pre = acc if kind == "h_unrounded" else C.float()
        G = gelu32(pre if kind == "gelu_no_bias" else pre + bv, tanh_form).to(torch.bfloat16)
    else:
        C = (acc + bv).to(torch.bfloat16)
    outs = []
    for X in (C, G):
        if X is None:
            outs.append(None)
            continue
        if kind == "swap_rows":
            rs, cs = _tile(*f["tile"], M, N, bn)
            r = rs.start + f["row"]
            X = X.clone()
            X[r, cs], X[r + 1, cs] = X[r + 1, cs].clone(), X[r, cs].clone()
        if kind == "clamp_row":
            X = X.clone()
            X[M - 1] = X[M - 2]
        if kind == "full_groups":  # tiles stored where the faulty map sends them; the rest never written
            Y = torch.full_like(X, NAN)
            for tid in range(((M + go.BM - 1) // go.BM) * (N // bn)):
                m0, n0 = go.tile_origin(tid, M, N, bn, full_groups=True)
                if m0 < M and n0 < N:
                    Y[m0:m0 + go.BM, n0:n0 + bn] = X[m0:m0 + go.BM, n0:n0 + bn]
            X = Y
        outs.append(X)
    return outs[0], outs[1]


def _q(x, fp8):
    """fp32 values -> the stored operand (bf16 or e4m3) and back: must be the identity for every fixture."""
    y = x.to(torch.float8_e4m3fn if fp8 else torch.bfloat16).float()
    assert torch.equal(x, y)
    return x


EMU_BF16 = (1, 2, 3, 4, 6)
EMU_FP8 = (7, 8, 9, 10, 11)
# bias variants of the bf16 kernel: (name, epi, bias kind, tanh)
BF16_VARIANTS = [("none", 0, None, False), ("bias_bf16", 1, "bf16", False), ("bias_f32", 1, "f32", False),
                 ("gelu_erf", 2, "f32", False), ("gelu_tanh", 2, "bf16", True)]


def _shape(case):
    return go.BF16_CASES[case] if case in go.BF16_CASES else go.FP8_CASES[case]


def _ksplit_of(case):
    """What gemm.hip's fp8_ksplit gives these shapes (asserted against the binding's query on the GPU)."""
    return go.EXPECT_KSPLIT.get(case, 1)


@functools.lru_cache(maxsize=None)
def _ternary(case):
    M, N, K = _shape(case)
    a, b = go.ternary(M, N, K)
    return a, b, (a @ b.t()).double()  # integers below 2^24: the fp32 product is exact


# ----------------------------------------------------------------------------- fixture preconditions
@pytest.mark.parametrize("case", sorted(go.BF16_CASES) + sorted(go.FP8_CASES))
def test_ternary_reference_stays_bf16_exact(case):
    a, b, ref = _ternary(case)
    fp8 = case in go.FP8_CASES
    _q(a, fp8), _q(b, fp8)
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and a.abs().sum() > 0 and b.abs().sum() > 0
    assert ref.abs().max() <= go.TERNARY_MAX, float(ref.abs().max())
    assert torch.equal(ref, ref.to(torch.bfloat16).double())
    if case <= 4:  # the fp32 product used above is the float64 one
        assert torch.equal(ref, a.double() @ b.double().t())


@pytest.mark.parametrize("case", sorted(go.BF16_CASES) + sorted(go.FP8_CASES))
def test_onehot_passes_cover_every_k(case):
    M, N, K = _shape(case)
    fp8 = case in go.FP8_CASES
    for R in (N, M):
        seen = torch.zeros(K, dtype=torch.bool)
        for p in range(go.onehot_passes(R, K)):
            rows, k, sign = go.onehot(R, K, p)
            assert torch.equal(rows.abs().sum(1), torch.ones(R)) and torch.equal(rows[torch.arange(R), k], sign)
            seen[k] = True
        assert bool(seen.all()), (case, R)
    _q(go.position_coded(min(M, 300), K, fp8), fp8)
    assert set(go.exact_bias(N).mul(4).abs().tolist()) <= set(float(i) for i in range(17))
    _q(go.exact_bias(N), False)


def test_split_ranges_and_tile_map():
    assert go.split_steps(16, 2) == [(0, 8), (8, 16)]
    assert [e - s for s, e in go.split_steps(25, 3)] == [8, 8, 9]
    lens = [e - s for s, e in go.split_steps(135, 16)]
    assert sum(lens) == 135 and set(lens) == {8, 9}
    for (M, N, bn) in ((1300, 256, 128), (4400, 3840, 256), (257, 384, 128), (1, 128, 128)):
        ntm, ntn = (M + 255) // 256, N // bn
        tiles = {go.tile_origin(t, M, N, bn) for t in range(ntm * ntn)}
        assert tiles == {(i * 256, j * bn) for i in range(ntm) for j in range(ntn)}  # a bijection onto the grid
    assert (18 * 15) % 8 != 0 and 18 % go.GROUP == 2 and 6 % go.GROUP == 2


# ----------------------------------------------------------------------------- the emulation passes
@pytest.mark.parametrize("variant", BF16_VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("case", EMU_BF16)
def test_emulation_bf16_exact(case, variant):
    name, epi, bkind, tanh = variant
    M, N, K = _shape(case)
    a, b, ref = _ternary(case)
    bias = None
    if epi == 1:
        bias = go.exact_bias(N)
        ref = ref + bias.double()
    elif epi == 2:
        bias = go.bias_bands(N)
    if bias is not None and bkind == "bf16":
        bias = bias.bfloat16()
    C, G = emulate(a, b, 64, bias, epi, tanh)
    go.assert_exact(C, ref, f"emu case {case} {name} ternary")
    if epi == 2:
        v, gref, genv = go.gelu_oracle(C, bias, tanh)
        go.assert_within(G, gref, genv, 1.0, go.FLOOR, name=f"emu case {case} {name} G")
        return
    for onehot_is_b in (True, False):
        R, Rc = (N, M) if onehot_is_b else (M, N)
        coded = go.position_coded(Rc, K)
        for p in range(go.onehot_passes(R, K)):
            rows, k, sign = go.onehot(R, K, p)
            want = go.onehot_ref(coded, k, sign, onehot_is_b)
            if bias is not None:
                want = want + bias.double()
            A_, B_ = (coded, rows) if onehot_is_b else (rows, coded)
            C, _ = emulate(A_, B_, 64, bias, epi)
            go.assert_exact(C, want, f"emu case {case} {name} onehot", kstep=64,
                            k_of=(lambda m, n: k[n]) if onehot_is_b else (lambda m, n: k[m]))


@pytest.mark.parametrize("bkind", [None, "f32", "bf16"])
@pytest.mark.parametrize("case", EMU_FP8)
def test_emulation_fp8_exact(case, bkind):
    M, N, K = _shape(case)
    a, b, ref = _ternary(case)
    sc = go.FP8_SA * go.FP8_SB
    ks = _ksplit_of(case) if bkind is None else 1  # a bias runs unsplit
    bias = None if bkind is None else go.exact_bias(N)
    ref = sc * ref if bias is None else sc * ref + bias.double()
    if bkind == "bf16":
        bias = bias.bfloat16()
    C, _ = emulate(a, b, 128, bias, int(bias is not None), scale=sc, ksplit=ks)
    go.assert_exact(C, ref, f"emu case {case} bias={bkind} ternary", kstep=128)
    for onehot_is_b in (True, False):
        R, Rc = (N, M) if onehot_is_b else (M, N)
        coded = _q(go.position_coded(Rc, K, fp8=True), True)
        npass = go.onehot_passes(R, K)
        for p in sorted({0, npass - 1}):  # first and last pass: the emulation is slow at K = 17280
            rows, k, sign = go.onehot(R, K, p)
            want = sc * go.onehot_ref(coded, k, sign, onehot_is_b)
            if bias is not None:
                want = want + bias.double()
            A_, B_ = (coded, rows) if onehot_is_b else (rows, coded)
            C, _ = emulate(A_, B_, 128, bias, int(bias is not None), scale=sc, ksplit=ks)
            go.assert_exact(C, want, f"emu case {case} bias={bkind} onehot", kstep=128,
                            k_of=(lambda m, n: k[n]) if onehot_is_b else (lambda m, n: k[m]))


@functools.lru_cache(maxsize=None)
def _real(case, kind):
    M, N, K = _shape(case)
    fp8 = case in go.FP8_CASES
    a, b = go.real_operands(M, N, K, kind, fp8)
    _q(a, fp8), _q(b, fp8)
    return (a, b) + go.products(a, b)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", go.ENVELOPE_BF16)
def test_emulation_bf16_envelope_and_gelu(case, kind):
    M, N, K = _shape(case)
    a, b, P, E = _real(case, kind)
    if kind == "cancel":
        assert P.abs().median() < E.median() / 32  # the reference nearly cancels
    g = torch.Generator().manual_seed(case)
    rb = torch.randn(N, generator=g)
    for name, epi, bkind, tanh in BF16_VARIANTS:
        bias = None if epi == 0 else (rb if epi == 1 else go.bias_bands(N))
        if bias is not None and bkind == "bf16":
            bias = bias.bfloat16()
        C, G = emulate(a, b, 64, bias, epi, tanh)
        ref, env = go.gemm_envelope(P, E, K, bias if epi == 1 else None)
        go.assert_within(C, ref, env, 1.0, go.FLOOR, name=f"emu case {case} {kind} {name} C")
        if epi == 2:
            v, gref, genv = go.gelu_oracle(C, bias, tanh)
            go.assert_within(G, gref, genv, 1.0, go.FLOOR, name=f"emu case {case} {kind} {name} G")
            if kind == "randn" and M >= 255:
                assert min(go.band_counts(v)) > 0, go.band_counts(v)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", go.ENVELOPE_FP8)
def test_emulation_fp8_envelope(case, kind):
    M, N, K = _shape(case)
    a, b, P, E = _real(case, kind)
    sa, sb = go.fp8_real_scales(K)
    sc = float(torch.tensor(sa) * torch.tensor(sb))  # the kernel's fp32 product of the two scales
    g = torch.Generator().manual_seed(case)
    rb = torch.randn(N, generator=g)
    for bkind in (None, "f32", "bf16"):
        bias = None if bkind is None else (rb if bkind == "f32" else rb.bfloat16())
        ks = _ksplit_of(case) if bias is None else 1
        C, _ = emulate(a, b, 128, bias, int(bias is not None), scale=sc, ksplit=ks)
        ref, env = go.gemm_envelope(P, E, K, bias, sc, ks)
        go.assert_within(C, ref, env, 1.0, go.FLOOR, name=f"emu case {case} {kind} bias={bkind}")


# ----------------------------------------------------------------------------- planted faults
def _region(fault, M, N, bn=128):
    """Boolean [M, N]: the elements the fault can have damaged."""
    reg = torch.zeros(M, N, dtype=torch.bool)
    kind = fault["kind"]
    if kind in ("skip_step", "swap_rows"):
        rs, cs = _tile(*fault["tile"], M, N, bn)
        if kind == "swap_rows":
            rs = slice(rs.start + fault["row"], rs.start + fault["row"] + 2)
        reg[rs, cs] = True
    elif kind == "clamp_row":
        reg[M - 1] = True
    elif kind == "full_groups":
        reg[:] = True
        for tid in range(((M + 255) // 256) * (N // bn)):
            m0, n0 = go.tile_origin(tid, M, N, bn, full_groups=True)
            reg[m0:m0 + 256, n0:n0 + bn] = False
    else:
        reg[:] = True
    return reg


def _reported(msg):
    m = re.search(r"(?:first|worst) at \((\d+), (\d+)\)", msg)
    assert m, msg
    return int(m.group(1)), int(m.group(2))


def _must_fail_exact(C, ref, reg, **kw):
    with pytest.raises(AssertionError) as ei:
        go.assert_exact(C, ref, "planted", **kw)
    assert reg[_reported(str(ei.value))]
    bad = ~(C == ref.to(torch.bfloat16))
    assert bool(bad.any()) and not bool((bad & ~reg).any())  # everything that differs lies in the region
    return str(ei.value)


def _must_fail_env(C, ref, env, reg):
    with pytest.raises(AssertionError) as ei:
        go.assert_within(C, ref, env, 1.0, go.FLOOR, name="planted")
    assert reg[_reported(str(ei.value))]
    bad = ~((C.double() - ref).abs() <= env + go.FLOOR)
    assert bool(bad.any()) and not bool((bad & ~reg).any())


# bf16 faults on case 4 (1300, 256, 320): 6 A bands (a group of 4 and one of 2) x 2 tiles of 128 columns
BF16_FAULTS = [
    {"kind": "skip_step", "tile": (2, 1), "step": 3},
    {"kind": "skip_step", "tile": (5, 0), "step": 4},      # the last K-step, in the tile with the M tail
    {"kind": "swap_rows", "tile": (1, 0), "row": 37},
    {"kind": "bias_shift"},
    {"kind": "full_groups"},
    {"kind": "clamp_row"},
]


@pytest.mark.parametrize("fault", BF16_FAULTS, ids=lambda f: f["kind"])
def test_planted_bf16_faults_are_rejected(fault):
    case = 4
    M, N, K = _shape(case)
    epi = 1 if fault["kind"] == "bias_shift" else 0
    reg = _region(fault, M, N)
    assert bool(reg.any()) and (fault["kind"] == "bias_shift" or not bool(reg.all()))
    # exact operands
    a, b, ref = _ternary(case)
    bias = go.exact_bias(N) if epi else None
    want = ref + bias.double() if epi else ref
    go.assert_exact(emulate(a, b, 64, bias, epi)[0], want, "clean")
    _must_fail_exact(emulate(a, b, 64, bias, epi, fault=fault)[0], want, reg)
    # real operands
    ar, br, P, E = _real(case, "randn")
    rb = torch.randn(N, generator=torch.Generator().manual_seed(4)) if epi else None
    rref, env = go.gemm_envelope(P, E, K, rb)
    go.assert_within(emulate(ar, br, 64, rb, epi)[0], rref, env, 1.0, go.FLOOR, name="clean")
    _must_fail_env(emulate(ar, br, 64, rb, epi, fault=fault)[0], rref, env, reg)
    # one-hot probes: a skipped K-step is named by the probe that selects a k inside it
    if fault["kind"] == "skip_step":
        coded = go.position_coded(M, K)
        named = set()
        for p in range(go.onehot_passes(N, K)):
            rows, k, sign = go.onehot(N, K, p)
            C = emulate(coded, rows, 64, fault=fault)[0]
            want = go.onehot_ref(coded, k, sign)
            if torch.equal(C, want.to(torch.bfloat16)):
                continue
            msg = _must_fail_exact(C, want, reg, kstep=64, k_of=lambda m, n: k[n])
            named.add(int(re.search(r"K-step (\d+)", msg).group(1)))
        assert named == {fault["step"]}


# split-K faults on case 10 (200, 128, 3200): splits of 8, 8 and 9 K-steps of 128
@pytest.mark.parametrize("kind", ["split_drop_last", "split_last_twice"])
@pytest.mark.parametrize("split", [1, 2])
def test_planted_split_k_faults_are_rejected(kind, split):
    case, ks, sc = 10, 3, go.FP8_SA * go.FP8_SB
    M, N, K = _shape(case)
    fault = {"kind": kind, "split": split}
    step = go.split_steps(K // 128, ks)[split][1] - 1
    reg = _region(fault, M, N)
    a, b, ref = _ternary(case)
    go.assert_exact(emulate(a, b, 128, scale=sc, ksplit=ks)[0], sc * ref, "clean")
    _must_fail_exact(emulate(a, b, 128, scale=sc, ksplit=ks, fault=fault)[0], sc * ref, reg)
    ar, br, P, E = _real(case, "randn")
    sa, sb = go.fp8_real_scales(K)
    rs = float(torch.tensor(sa) * torch.tensor(sb))
    rref, env = go.gemm_envelope(P, E, K, None, rs, ks)
    _must_fail_env(emulate(ar, br, 128, scale=rs, ksplit=ks, fault=fault)[0], rref, env, reg)
    ar, br, P, E = _real(case, "cancel")
    rref, env = go.gemm_envelope(P, E, K, None, rs, ks)
    _must_fail_env(emulate(ar, br, 128, scale=rs, ksplit=ks, fault=fault)[0], rref, env, reg)
    # the one-hot pass that selects the k of that K-step names it
    coded = go.position_coded(M, K, fp8=True)
    named = set()
    for p in range(go.onehot_passes(N, K)):
        rows, k, sign = go.onehot(N, K, p)
        C = emulate(coded, rows, 128, scale=sc, ksplit=ks, fault=fault)[0]
        want = sc * go.onehot_ref(coded, k, sign)
        if not torch.equal(C, want.to(torch.bfloat16)):
            msg = _must_fail_exact(C, want, reg, kstep=128, k_of=lambda m, n: k[n])
            named.add(int(re.search(r"K-step (\d+)", msg).group(1)))
    assert named == {step}


@pytest.mark.parametrize("tanh", [False, True], ids=["erf", "tanh"])
@pytest.mark.parametrize("kind", ["h_unrounded", "gelu_no_bias"])
def test_planted_gelu_faults_are_rejected(kind, tanh):
    case = 3
    M, N, K = _shape(case)
    a, b, P, E = _real(case, "randn")
    bias = go.bias_bands(N)
    C, G = emulate(a, b, 64, bias, 2, tanh)
    v, gref, genv = go.gelu_oracle(C, bias, tanh)
    go.assert_within(G, gref, genv, 1.0, go.FLOOR, name="clean")
    C2, G2 = emulate(a, b, 64, bias, 2, tanh, fault={"kind": kind})
    assert torch.equal(C2, C)  # H itself is untouched: only the check of G can see these
    with pytest.raises(AssertionError) as ei:
        go.assert_within(G2, gref, genv, 1.0, go.FLOOR, name="planted")
    m, n = _reported(str(ei.value))
    assert 0 <= m < M and 0 <= n < N
    if kind == "h_unrounded":  # seen where the bias has cancelled most of H: |v| well below |H|
        bad = ~((G2.double() - gref).abs() <= genv + go.FLOOR)
        assert int(bad.sum()) > 100


def test_envelope_is_not_a_whole_tensor_tolerance():
    """One element moved by one bf16 ulp fails the exact test; one element of the cancelling reference moved by
    2^-10 of |A| |B|^T fails the envelope, where err / max|ref| is 1e-4 and a norm ratio 1e-6."""
    a, b, ref = _ternary(3)
    C = emulate(a, b, 64)[0].clone()
    C[200, 300] = (C[200, 300].float() + (1.0 if C[200, 300] == 0 else C[200, 300].float().abs() * 2 ** -7)).bfloat16()
    with pytest.raises(AssertionError, match=r"first at \(200, 300\)"):
        go.assert_exact(C, ref, "one ulp")
    ar, br, P, E = _real(3, "cancel")
    rref, env = go.gemm_envelope(P, E, 192)
    C = emulate(ar, br, 64)[0].float()
    C[100, 7] += float(E[100, 7]) * 2 ** -10
    with pytest.raises(AssertionError, match=r"worst at \(100, 7\)"):
        go.assert_within(C, rref, env, 1.0, go.FLOOR, name="cancel")
