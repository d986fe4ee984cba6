"""The BatchNorm oracle (tests/bn_oracle.py) is sharp, shown on the CPU before any GPU runs:
  * its fp64 reference agrees with torch's float64 autograd of F.batch_norm (+ residual)(+ ReLU), running
    statistics included;
  * an fp32 emulation of the kernels — shifted sums from row 0, partitioned into nrow blocks and R row
    slots exactly as the replica geometry says, slab sums in the finalize's order, the variance step in
    double, bf16 rounding at the outputs — stays inside every envelope at ratio < 1 for the per-channel
    results and < 2 elementwise, on every case the GPU tests run (bn_oracle.all_cases);
  * each listed mutation of the emulation is rejected on inputs at which the clean emulation passes;
  * the share of ambiguous ReLU decisions (and pool winners) is within the cap for every one of those inputs,
    the apply-kernel, eval and stem inputs included (bn_oracle.apply_cases, STEM_SHAPES);
  * the stem pool's reference is max_pool2d in float64, its tie rule (first maximum in scan order) is
    really decided by the bf16 inputs, and a dropped pool gradient is far outside its bound.
The replica of the launch geometry is pinned against hand-computed values of reduce_geo3, and bn_tune is
shown to refuse the variants that no longer exist (the binding loads without a GPU)."""
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as bo

SUM_OUTPUTS = ("mean", "invstd", "running_mean", "running_var", "dbeta", "dgamma", "A", "B", "D")
ELT_OUTPUTS = ("y", "dx")


# ----------------------------------------------------------------------------- fp32 emulation of the kernels
def _reduce(T1, T2, M, C, U, path, weight=None):
    """bn_reduce3_kernel + its finalize's slab sum on fp32 term tensors [M, C]: per block and row slot r the
    rows m0 + r, m0 + r + R, ... in order; the R slots in order; the slabs in bn_fin_kernel's order (variant
    5: 8 strided subsets, then the subsets) or the in-kernel finalize's (variant 3: groups of 16 in order,
    then the groups). ``weight`` [M]: how often a row is counted (the mutations)."""
    g = bo.reduce_geo3(M, C, U, path.target_blocks)
    steps = -(-g.rows_per_block // g.R)
    blk = torch.arange(g.nrow).view(-1, 1, 1)
    i = torch.arange(steps).view(1, -1, 1)
    r = torch.arange(g.R).view(1, 1, -1)
    inb = i * g.R + r
    m = blk * g.rows_per_block + inb
    valid = (inb < g.rows_per_block) & (m < M)
    m = m.clamp_max(M - 1)
    wt = valid.float()
    if weight is not None:
        wt = wt * weight[m]
    out = []
    for T in (T1, T2):
        acc = torch.zeros(g.nrow, g.R, C, dtype=torch.float32)
        for s in range(steps):
            acc = acc + T[m[:, s]] * wt[:, s].unsqueeze(-1)
        slab = torch.zeros(g.nrow, C, dtype=torch.float32)
        for rr in range(g.R):
            slab = slab + acc[:, rr]
        if path.variant == 5:
            tot = torch.zeros(C, dtype=torch.float32)
            for j in range(8):
                a = torch.zeros(C, dtype=torch.float32)
                for b in range(j, g.nrow, 8):
                    a = a + slab[b]
                tot = tot + a
        else:
            groups = []
            for g0 in range(0, g.nrow, bo.K_G):
                n = min(bo.K_G, g.nrow - g0)
                a = slab[g0].clone() if n == 1 else torch.zeros(C, dtype=torch.float32)
                if n > 1:
                    for b in range(g0, g0 + n):
                        a = a + slab[b]
                groups.append(a)
            tot = groups[0]
            if len(groups) > 1:
                tot = torch.zeros(C, dtype=torch.float32)
                for a in groups:
                    tot = tot + a
        out.append(tot)
    return out


def _block_last_row(M, C, U, path):
    g = bo.reduce_geo3(M, C, U, path.target_blocks)
    b = g.nrow // 2
    return min(M, (b + 1) * g.rows_per_block) - 1


def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def emulate(inp, case, mut=None, res_ab=None):
    """Forward + backward of the train path in fp32 where the kernels use fp32, double where they use
    double, bf16 at the outputs. ``mut`` plants one bug. Returns the outputs by the oracle's names."""
    M, C, path = case.M, case.C, case.path
    f32 = torch.float32
    x = inp["x"].float()
    w = inp["w"] if case.wb else torch.ones(C)
    b = inp["b"] if case.wb else torch.zeros(C)
    p = torch.tensor(case.momentum, dtype=f32)
    eps = float(torch.tensor(1e-5, dtype=f32))
    k = x[0]
    d = x - k
    wf = None
    if mut in ("fwd_drop", "fwd_twice"):
        wf = torch.ones(M)
        wf[_block_last_row(M, C, path.u_fwd, path)] = 0.0 if mut == "fwd_drop" else 2.0
    S1, S2 = _reduce(d, d * d, M, C, path.u_fwd, path, wf)
    d1 = S1.double() / M
    mean_d = k.double() + d1
    var = (S2.double() / M - d1 * d1).clamp_min(0)
    mu = mean_d.to(f32)
    inv = (1.0 / torch.sqrt(var + eps)).to(f32)
    a = w * inv
    bb = b - mu * w * inv
    unb = var if (M == 1 or mut == "rv_biased") else var * M / (M - 1)
    one_p = torch.tensor(1.0, dtype=f32) - p
    if mut == "rm_swapped":
        rm = p * inp["rm"] + one_p * mu
    else:
        rm = one_p * inp["rm"] + p * mu
    rv = one_p * inp["rv"] + p * unb.to(f32)
    if mut == "coef_plus8":
        a, bb = a.roll(-8), bb.roll(-8)
    t = x * a + bb
    if case.res:
        t = t + (inp["r"].float() if res_ab is None else inp["r"].float() * res_ab[0] + res_ab[1])
    pos = t > 0
    yf = torch.where(pos, t, torch.zeros_like(t)) if case.relu else t
    y = _truncate_bf16(yf) if mut == "y_truncated" else yf.bfloat16()
    out = {"mean": mu, "invstd": inv, "running_mean": rm, "running_var": rv, "y": y, "a": a, "b": bb}
    mask = None
    if case.relu:
        mask = pos.clone()
        if mut == "mask_flip":
            mask[M // 2, C // 2] = ~mask[M // 2, C // 2]
        out["mask"] = mask
    # backward
    dz = inp["dy"].float()
    if case.relu:
        dz = dz * mask.float()
    wb = None
    if mut == "bwd_drop":
        wb = torch.ones(M)
        wb[_block_last_row(M, C, path.u_bwd, path)] = 0.0
    xc = x - mu
    S1b, S2b = _reduce(dz, dz * xc, M, C, path.u_bwd, path, wb)
    db, dg = S1b, S2b * inv
    inv_m = torch.tensor(1.0, dtype=f32) / torch.tensor(float(M), dtype=f32)
    inv_d = torch.tensor(1.0, dtype=f32) / torch.tensor(float(max(M - 1, 1)), dtype=f32) if mut == "D_m_minus_1" else inv_m
    A = w * inv
    B = -w * inv * inv * dg * inv_m
    D = -w * inv * db * inv_d
    out.update(dbeta=db, dgamma=dg, A=A, B=B, D=D, dx=(A * dz + B * xc + D).bfloat16(), dres=dz.bfloat16())
    return out


def _oracle(inp, case, mask=None, res_ab=None):
    return bo.batchnorm_oracle(inp["x"], inp.get("r") if case.res else None, inp["w"] if case.wb else None,
                               inp["b"] if case.wb else None, inp["rm"], inp["rv"], case.momentum, 1e-5, case.relu,
                               dy=inp["dy"], res_ab=res_ab, path=case.path, mask=mask)


def compare(got, ref, env, case, record=None, pool=None):
    """Every output through the comparator; returns {name: ratio | AssertionError}. The checks (and their
    constants) are the GPU tests' own: bn_oracle.check_relu for the ReLU contract, dres bit for bit."""
    res = {}
    for names, c in ((SUM_OUTPUTS, bo.BN_C_SUM), (ELT_OUTPUTS, bo.BN_C)):
        for n in names:
            if n not in got or n not in ref:
                continue
            try:
                res[n] = bo.assert_within(got[n], ref[n], env[n], c, bo.FLOOR, name=f"{case.name} {n}", record=record)
            except AssertionError as e:
                res[n] = e
    if case.relu:
        try:
            res["relu"] = bo.check_relu(got["y"], got["mask"], ref, case.name, pool)
        except AssertionError as e:
            res["relu"] = e
    if "dres" in got:
        same = torch.equal(got["dres"].double(), ref["dz"])
        res["dres"] = 0.0 if same else AssertionError(f"{case.name}: dres differs from dy * mask")
    return res


def _failed(res):
    return {n for n, r in res.items() if isinstance(r, AssertionError)}


def _run(case, mut=None, pool=None):
    inp = bo.make_inputs(case.regime, case.M, case.C, case.seed, res=case.res, U=case.path.u_fwd, path=case.path)
    res_ab = bo.make_res_ab(case.C) if case.name.startswith("res_ab") else None
    got = emulate(inp, case, mut, res_ab)
    ref, env = _oracle(inp, case, mask=got.get("mask"), res_ab=res_ab)
    return compare(got, ref, env, case, pool=pool), got, ref


# ----------------------------------------------------------------------------- the replica
def test_geometry_replica_known_values():
    """reduce_geo3 worked by hand from batchnorm.hip: ResNet-50 layer 1 at batch 128 (M = 401,408, C = 64:
    the 512-block cap, 784 rows each), a capped multi-chunk width, a tiny M, and the issue's two > 128-slab
    shapes under bn_tune(5, 512, 2, 2)."""
    assert bo.reduce_geo3(401408, 64, 8) == bo.Geo(64, 32, 1, 512, 784, 32)
    assert bo.reduce_geo3(6272, 2048, 8) == bo.Geo(512, 4, 4, 98, 64, 7)
    assert bo.reduce_geo3(3, 192, 8) == bo.Geo(64, 32, 3, 1, 3, 1)
    assert bo.reduce_geo3(16520, 64, 2).nrow == 130 and bo.reduce_geo3(2100, 512, 2).nrow == 132
    assert [bo.chunk3(c) for c in (64, 128, 192, 256, 320, 512, 1024, 4096)] == [64, 128, 64, 256, 64, 512, 512, 512]
    assert {bo.reduce_geo3(c.M, c.C, 2).nrow for c in bo.variant3_cases()} == {1, 2, 16, 17, 33, 130}
    for c in bo.partition_cases():
        U = int(c.name.split("U=")[1][0])
        g = bo.reduce_geo3(c.M, c.C, U, c.path.target_blocks)
        nfull = int(c.name.split("nfull=")[1][0])
        assert g.rows_per_block % (U * g.R) != 0 and g.rows_per_block // (U * g.R) == nfull and c.M % g.rows_per_block != 0


# ----------------------------------------------------------------------------- reference against autograd
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M", [2, 37])
def test_reference_matches_float64_autograd(M, relu, res):
    g = torch.Generator().manual_seed(M)
    C = 64
    x = torch.randn(M, C, generator=g, dtype=torch.float64, requires_grad=True)
    r = torch.randn(M, C, generator=g, dtype=torch.float64, requires_grad=True) if res else None
    w = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    b = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    eps, p = bo._f32(1e-5), bo._f32(0.1)
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm2, rv2, w, b, True, p, eps)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    grads = torch.autograd.grad(y, (x, w, b) + ((r,) if res else ()), dy)
    ref, _ = bo.batchnorm_oracle(x.detach(), r.detach() if res else None, w.detach(), b.detach(), rm, rv, 0.1, 1e-5,
                                 relu, dy=dy)
    pairs = [(ref["y"], y.detach()), (ref["dx"], grads[0]), (ref["dgamma"], grads[1]), (ref["dbeta"], grads[2]),
             (ref["running_mean"], rm2), (ref["running_var"], rv2)]
    if res:
        pairs.append((ref["dz"], grads[3]))
    for a, bb in pairs:
        torch.testing.assert_close(a, bb, rtol=1e-11, atol=1e-11)


def test_reference_single_row_keeps_biased_variance():
    """M = 1: var = 0, invstd = eps^-1/2, y = beta, running_var' = (1 - p) rv (the op's Mt > 1 ? ... : var)."""
    x = torch.randn(1, 64, dtype=torch.float64)
    rm, rv = torch.zeros(64, dtype=torch.float64), torch.full((64,), 2.0, dtype=torch.float64)
    ref, env = bo.batchnorm_oracle(x, None, None, None, rm, rv, 0.25, 1e-5, False)
    assert torch.equal(ref["var"], torch.zeros(64, dtype=torch.float64))
    torch.testing.assert_close(ref["running_var"], torch.full((64,), 1.5, dtype=torch.float64), rtol=1e-12, atol=0)
    torch.testing.assert_close(ref["running_mean"], 0.25 * x[0], rtol=1e-12, atol=0)
    assert torch.equal(ref["y"], torch.zeros(1, 64, dtype=torch.float64))
    assert all(bool(torch.isfinite(e).all()) for e in env.values())


# ----------------------------------------------------------------------------- the clean emulation
_RATIOS = {}


@pytest.mark.parametrize("group", ["w64", "w128", "w192", "w256", "w320", "w512", "w1024", "w4096", "partition", "slabs5",
                                   "slabs3", "variant3", "large_mean", "wgs1", "res_ab", "coef", "nodgamma"])
def test_clean_emulation_inside_every_envelope(group):
    """Every case of the GPU tests: ratio < 1 per channel, < 2 elementwise, the ambiguous share within the
    cap (check_relu), dres bit for bit."""
    cases = {"partition": bo.partition_cases, "slabs5": lambda: bo.slab_cases(5), "slabs3": lambda: bo.slab_cases(3),
             "variant3": bo.variant3_cases, "large_mean": lambda: [bo.large_mean_case()]}
    if group in cases:
        cs = cases[group]()
    elif group in bo.apply_cases():
        cs = bo.apply_cases()[group]
    else:
        cs = bo.width_cases(int(group[1:]))
    errors = []
    pool = bo.AmbiguityPool()
    for case in cs:
        res, got, ref = _run(case, pool=pool)
        for n, r in res.items():
            if isinstance(r, AssertionError):
                errors.append(str(r))
            elif n != "relu":
                _RATIOS[n] = max(_RATIOS.get(n, 0.0), r)
                lim = 1.0 if n in SUM_OUTPUTS else 2.0
                if not r < lim:
                    errors.append(f"{case.name} {n}: ratio {r:.3g} not below {lim}")
        if case.regime == "dense" and case.M * case.C >= 100000:
            bias, n = bo.rounding_bias(got["y"], ref["y"])
            if not abs(bias) <= bo.ROUNDING_BIAS_MAX:
                errors.append(f"{case.name}: rounding bias {bias:.3g} over {n} elements")
    print(f"ambiguous {pool.amb} of {pool.total}")
    pool.check(group)
    print("worst emulation ratios so far:", {k: round(v, 3) for k, v in _RATIOS.items()})
    assert not errors, "\n".join(errors[:20])


def test_eval_emulation_inside_envelope():
    """bn_fwd_eval's arithmetic in fp32 (a = gamma rsqrt(rv + eps), b = beta - rm gamma invstd) on the eval
    cases of the GPU test: y inside 2 x envelope, ReLU decisions, the ambiguity cap."""
    for case in bo.apply_cases()["eval"]:
        inp = bo.make_inputs(case.regime, case.M, case.C, case.seed, res=case.res)
        w = inp["w"] if case.wb else torch.ones(case.C)
        b = inp["b"] if case.wb else torch.zeros(case.C)
        inv = torch.rsqrt(inp["rv"] + torch.tensor(1e-5, dtype=torch.float32))
        a, bb = w * inv, b - inp["rm"] * w * inv
        t = inp["x"].float() * a + bb
        if case.res:
            t = t + inp["r"].float()
        y = t.clamp_min(0).bfloat16()
        ref, env = bo.eval_oracle(inp["x"], inp.get("r"), inp["w"] if case.wb else None, inp["b"] if case.wb else None,
                                  inp["rm"], inp["rv"], 1e-5, True)
        assert bo.assert_within(y, ref["y"], env["y"], bo.BN_C, bo.FLOOR, name=case.name) < 2
        pool = bo.AmbiguityPool()
        bo.check_relu(y, t > 0, ref, case.name, pool)
        pool.check(case.name)
        # the wrong running statistic (rv without eps is fine; rm of channel c + 8 is not)
        y_bad = (inp["x"].float() * a + (b - inp["rm"].roll(-8) * w * inv) + (inp["r"].float() if case.res else 0)).clamp_min(0)
        with pytest.raises(AssertionError):
            bo.assert_within(y_bad.bfloat16(), ref["y"], env["y"], bo.BN_C, bo.FLOOR, name=case.name)


def _emulate_pool(x4, a, b, tie="first"):
    """bn_apply_pool_kernel in fp32: z = fma(x, a, b) (one rounding), the max with a strict > in scan order."""
    N, H, W, C = x4.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z = (x4.double() * a.double() + b.double()).float()
    win = bo._windows(z, Ho, Wo, float("-inf"))
    m = win.amax(0)
    ks = torch.arange(9).view(9, 1, 1, 1, 1)
    hit = win == m
    k = torch.where(hit, ks, torch.full_like(ks, 99)).amin(0) if tie == "first" else torch.where(hit, ks, -1).amax(0)
    return m.clamp_min(0).bfloat16(), torch.where(m > 0, k, torch.full_like(k, 15))


@pytest.mark.parametrize("shape", bo.STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_pool_emulation_and_tie_rule(shape):
    """The stem shapes of the GPU test: pooled y inside the envelope, winner codes equal to the reference off the
    ambiguous windows, the cap; keeping the LAST maximum of a window instead of the first is rejected wherever
    the bf16 inputs tie (they do at the 16 x 16 shape)."""
    N, C, H, W = shape
    inp = bo.stem_inputs(shape)
    case = bo.Case("stem", "dense", N * H * W, C, False, False, True, 0.1, bo.Path(), 0)
    got = emulate(inp, case)
    ref, env = bo.batchnorm_oracle(inp["x"], None, inp["w"], inp["b"], inp["rm"], inp["rv"], 0.1, 1e-5, False)
    x4 = inp["x"].view(N, H, W, C)
    pr, pe = bo.pool_oracle(x4, ref, env)
    y, code = _emulate_pool(x4, got["a"], got["b"])
    assert bo.assert_within(y, pr["y"], pe["y"], bo.BN_C, bo.FLOOR, name=f"stem {shape} y") < 2
    pool = bo.AmbiguityPool()
    pool.add(pr["amb"], f"stem {shape}")
    pool.check(f"stem {shape}")
    assert not bool(((code != pr["code"]) & ~pr["amb"]).any())
    assert bool(((code == 15) == (y.double() <= 0)).all())
    if shape == (3, 64, 16, 16):
        _, last = _emulate_pool(x4, got["a"], got["b"], tie="last")
        assert bool(((last != pr["code"]) & ~pr["amb"]).any())
    g = torch.Generator().manual_seed(1)
    dy = torch.randn(pr["y"].shape, generator=g).bfloat16()
    dz, e = bo.pool_bwd_oracle(dy, code, H, W)
    lost = dz.clone()
    lost.view(-1)[int(dz.abs().reshape(-1).argmax())] = 0  # one pixel's gradient dropped
    assert bo.worst_ratio(dz.bfloat16(), dz, e)[0] <= 1
    assert bo.worst_ratio(lost.bfloat16(), dz, e)[0] > 100


# ----------------------------------------------------------------------------- mutations
_DENSE = bo.Case("mut dense", "dense", 1153, 64, True, True, True, 0.1, bo.Path(5, 3, 8, 4), 5)
_PROBE = _DENSE._replace(name="mut probe", regime="probe")
_SMALL = bo.Case("mut small", "dense", 33, 64, True, False, True, 0.1, bo.Path(), 6)
_BIG = bo.slab_cases(5)[1]  # dense, > 1e5 elements


@pytest.mark.parametrize("case", [_DENSE, _PROBE, _SMALL], ids=lambda c: c.name)
def test_mutation_inputs_pass_clean(case):
    res, _, _ = _run(case)
    assert not _failed(res), res


@pytest.mark.parametrize("mut,case,must_fail", [
    ("fwd_drop", _PROBE, {"mean", "invstd"}),
    ("fwd_drop", _DENSE, {"mean"}),
    ("fwd_twice", _PROBE, {"mean", "invstd"}),
    ("fwd_twice", _DENSE, {"mean"}),
    ("bwd_drop", _PROBE, {"dbeta", "dgamma"}),
    ("bwd_drop", _DENSE, {"dbeta"}),
    ("rv_biased", _DENSE, {"running_var"}),
    ("rm_swapped", _DENSE, {"running_mean"}),
    ("coef_plus8", _DENSE, {"y"}),
    ("mask_flip", _DENSE, {"relu"}),
    ("D_m_minus_1", _DENSE, {"D"}),
    ("D_m_minus_1", _SMALL, {"D", "dx"}),
])
def test_mutation_is_rejected(mut, case, must_fail):
    res, _, _ = _run(case, mut)
    failed = _failed(res)
    assert must_fail <= failed, (mut, case.name, failed, {k: (v if not isinstance(v, AssertionError) else "FAIL") for k, v in res.items()})


def test_truncated_output_is_rejected_by_rounding_bias():
    """Truncation stays inside 2 u_out |y| elementwise; the mean signed relative error gives it away."""
    _, got, ref = _run(_BIG)
    bias, n = bo.rounding_bias(got["y"], ref["y"])
    assert n >= 100000 and abs(bias) <= bo.ROUNDING_BIAS_MAX, (bias, n)
    _, got, ref = _run(_BIG, "y_truncated")
    bias, n = bo.rounding_bias(got["y"], ref["y"])
    assert bias < -bo.ROUNDING_BIAS_MAX, (bias, n)


def test_biased_running_var_is_rejected_at_the_old_tests_shape():
    """M = 1456, momentum 0.1 (test_batchnorm_train_fwd_bwd's shape): the biased variance moves running_var by
    ~1e-4, inside the old rtol = atol = 1e-3, and is many envelopes out here."""
    case = bo.Case("rv 1456", "dense", 1456, 64, False, False, True, 0.1, bo.Path(), 9)
    assert not _failed(_run(case)[0])
    res, _, _ = _run(case, "rv_biased")
    assert "running_var" in _failed(res)


# ----------------------------------------------------------------------------- stem pool oracle
@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (1, 1, 1, 8), (2, 2, 3, 8), (1, 16, 16, 8)])
def test_pool_oracle_matches_float64_max_pool(shape):
    """pool_oracle's y is max_pool2d(relu(a x + b), 3, 2, 1) and pool_bwd_oracle's dz its float64 gradient
    (random float64 inputs: no ties); with bf16-like inputs that tie, the code is the first maximum in scan order."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    a, b = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    zero = torch.zeros(C, dtype=torch.float64)
    ref, env = bo.pool_oracle(x, {"a": a, "b": b}, {"a": zero, "b": zero})
    z = (x * a + b).permute(0, 3, 1, 2).requires_grad_()
    yt = F.max_pool2d(F.relu(z), 3, 2, 1)
    torch.testing.assert_close(ref["y"], yt.detach().permute(0, 2, 3, 1), rtol=0, atol=0)
    dy = torch.randn(ref["y"].shape, generator=g, dtype=torch.float64)
    (gz,) = torch.autograd.grad(yt, z, dy.permute(0, 3, 1, 2))
    dz, _ = bo.pool_bwd_oracle(dy, ref["code"], H, W)
    torch.testing.assert_close(dz, gz.permute(0, 2, 3, 1), rtol=1e-13, atol=1e-13)
    assert bool(((ref["code"] == 15) == (ref["y"] <= 0)).all())
    # exact ties: a constant positive image -> the first valid window element wins everywhere
    one = torch.ones(1, 4, 4, 8, dtype=torch.float64)
    r2, _ = bo.pool_oracle(one, {"a": torch.ones(8, dtype=torch.float64), "b": zero}, {"a": zero, "b": zero})
    assert r2["code"][0, :, :, 0].tolist() == [[4, 3], [1, 0]] and not bool(r2["amb"].any())


# ----------------------------------------------------------------------------- bn_tune
def test_bn_tune_accepts_only_variants_0_3_5():
    """The binding loads without a GPU: variant 0 keeps the setting, 3 and 5 select a finalize, and every
    other value (2 and 4 were silently ignored / left the statistics unwritten) raises ValueError."""
    from pytorch_distributed_training_example_amd.ops._native import native
    C_ = native()
    try:
        for v in (0, 3, 5):
            C_.bn_tune(v, 512, 8, 4)
        for v in (1, 2, 4, 6, -1):
            with pytest.raises(ValueError):
                C_.bn_tune(v, 512, 8, 4)
    finally:
        C_.bn_tune(5, 512, 8, 4)
