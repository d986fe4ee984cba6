"""The 3x3 convolution kernels (csrc/kernels/conv3x3.hip, conv3x3_s2.hip, conv3x3_wgrad.hip) against the oracles of
tests/conv_oracle.py, whose docstring carries the analysis:
  (a) integer operands (ternary, offset, one-hot weights on a position-coded input, impulse output gradients):
      the output equals the exact float64 result rounded once to bf16, bit for bit;
  (b) real-valued operands, randn and nearly cancelling: every element inside
      U_BF16 |ref| + 2 (Kred + nsplit + 2) U_FP32 (the reference on absolute values);
  (c) the fused BatchNorm epilogues on the exact fixtures: per-tile sums and the backward partials bit for bit,
      centred sums of squares inside (n_t + 16) U_FP32 (sum (y - K)^2 + (sum (y - K))^2 / n_t).
Every case asserts, through the host-only queries conv3x3s1_variant and conv3x3_wgrad_geo, which kernel and which
split geometry it reached. tests/test_conv3x3_oracle_cpu.py runs an emulation and planted faults through the same
checks. Every comparison prints ``ratio <name> <value>`` or a mismatch count; with PDT_CONV_ORACLE_RATIOS=<path> the
worst per name are written there (kept in profiles/r15/conv3x3_oracle_ratios.txt)."""
import functools
import os

import pytest
import torch

import conv_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}
OPT_DEFAULT = 41

# case -> (forward variant, data-gradient variant) under the default bits, 256 compute units
EXPECT_VARIANT = {
    1: ("tap_narrow", "tap_narrow"), 2: ("tap_wide", "tap_narrow"), 3: ("tap_wide", "tap_narrow"),
    4: ("halo_narrow", "halo_narrow"), 5: ("halo_narrow", "halo_narrow"), 6: ("halo_wide", "halo_narrow"),
    7: ("wst", "wst"), 8: ("wst", "wst"), 9: ("wsr", "wsr"), 10: ("wsr", "wsr"), 11: ("wst", "wst"),
}
# with bit 5 cleared the row-tile shapes go elsewhere: case 9's halo (696 rows) is beyond the weight-stationary
# kernel's 640, case 10 is that kernel under its largest halo BOUND (580 rows; its tiles align with the images and
# stage 464: case 11 is the shape whose tiles cross images at W = 56 and stage all 580)
EXPECT_NO_WSR = {9: ("tap_narrow", "tap_narrow"), 10: ("wst", "wst")}
# (case, opt bits): the default everywhere; each variant bit on the cases whose kernel reads it
OPT_RUNS = [(c, OPT_DEFAULT) for c in sorted(co.S1_CASES)] + [
    # bit 0: wst skips the DMA of halo rows past its tile's extent
    (7, OPT_DEFAULT & ~1), (8, OPT_DEFAULT & ~1), (10, OPT_DEFAULT & ~1 & ~32), (11, OPT_DEFAULT & ~1),
    (7, OPT_DEFAULT & ~8), (8, OPT_DEFAULT & ~8), (10, OPT_DEFAULT & ~8 & ~32),   # bit 3: wst pipeline pinned
    (9, OPT_DEFAULT & ~32), (10, OPT_DEFAULT & ~32),                              # bit 5: row-tile kernel
    (4, OPT_DEFAULT | 64), (5, OPT_DEFAULT | 64), (6, OPT_DEFAULT | 64),          # bit 6: halo DMA through asm
    (10, OPT_DEFAULT | 128),                                                      # bit 7: row-tile BSTATS
]
OPT_RUNS.sort()


def _C():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PDT_CONV_ORACLE_RATIOS")
    if path and RECORD:
        with open(path, "w") as f:
            for name in sorted(RECORD):
                f.write(f"{name:<72} {RECORD[name]:.4g}\n")


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """A kernel fault poisons the process's device context: end the session there, launch nothing more."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after this test, nothing more is launched: {e}", returncode=3)


class _opt:
    """conv3x3_opt bits for a block, restored with conv3x3_opt(-1)."""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        _C().conv3x3_opt(self.bits)

    def __exit__(self, *exc):
        _C().conv3x3_opt(-1)


class _tune:
    """conv3x3_wgrad_tune(target_wgs, co_tile) for a block. (-1 leaves a field as it is, so (-1, 0) alone would
    keep a forced target: the restore is (0, 0), both fields back to their defaults.)"""

    def __init__(self, target_wgs, co_tile):
        self.args = (target_wgs, co_tile)

    def __enter__(self):
        _C().conv3x3_wgrad_tune(*self.args)

    def __exit__(self, *exc):
        _C().conv3x3_wgrad_tune(0, 0)


def _exact(got, ref, name, **kw):
    try:
        co.assert_exact_nhwc(got, ref, name, record=RECORD, **kw)
    finally:
        print(f"ratio {name} mismatches {RECORD.get(name)}")


def _exact_dw(got, ref, name, **kw):
    try:
        co.assert_exact_dw(got, ref, name, record=RECORD, **kw)
    finally:
        print(f"ratio {name} mismatches {RECORD.get(name)}")


def _equal(got, want, name):
    """Bit for bit on fp32 partials."""
    n, at = co.mismatches(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]))
    RECORD[name] = max(RECORD.get(name, 0), n)
    print(f"ratio {name} mismatches {n}")
    assert n == 0, (f"{name}: {n} of {got.numel()} differ; first at (row {at[0]}, channel {at[1]}): "
                    f"got {float(got.reshape(-1, got.shape[-1])[at]):.9g}, "
                    f"want {float(want.reshape(-1, want.shape[-1])[at]):.9g}")


def _within(got, ref, env, name):
    try:
        co.assert_within(got, ref, env, 1.0, co.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


def _bf(t):
    return t.to(DEV).to(torch.bfloat16).contiguous()


def _nhwc(t4):
    """A channels_last [N, C, H, W] result as contiguous NHWC."""
    out = t4.permute(0, 2, 3, 1)
    assert out.is_contiguous()
    return out


def _variant(shape, dgrad=False):
    N, H, W, Ci, Co = shape
    v = _C().conv3x3s1_variant(N, H, W, Co, Ci) if dgrad else _C().conv3x3s1_variant(N, H, W, Ci, Co)
    assert v in co.VARIANTS, v
    return v


def _expect(case, opt):
    return EXPECT_NO_WSR[case] if case in EXPECT_NO_WSR and not opt & 32 else EXPECT_VARIANT[case]


def _assert_variant(case, opt=OPT_DEFAULT):
    """Under the bits now set, the case reaches the variants it names (forward, data gradient)."""
    want = _expect(case, opt)
    got = (_variant(co.S1_CASES[case]), _variant(co.S1_CASES[case], dgrad=True))
    assert got == want, f"case {case} (opt {opt}) was to reach {want}, the launcher decides {got}"
    return got


def _rows(variant):
    return co.BM_WSR if variant == "wsr" else co.BM


def _poison(*sizes):
    """NaN into the blocks the next allocations of these sizes ((numel, dtype) each) will most likely be given
    back by the caching allocator: an element a kernel leaves unwritten then cannot pass by still holding an
    earlier call's equal result."""
    blocks = [torch.full((n,), float("nan"), dtype=dt, device=DEV) for n, dt in sizes]
    del blocks


def fwd1(x, w):
    _poison((x.numel() // x.shape[3] * w.shape[0], torch.bfloat16))
    return _nhwc(_C().conv3x3s1_fwd(co.nchw(x), co.w_nchw(w)))


def dgrad1(dy, w):
    wf = _C().conv3x3_flip(co.w_nchw(w))
    _poison((dy.numel() // dy.shape[3] * w.shape[2], torch.bfloat16))
    return _nhwc(_C().conv3x3s1_fwd(co.nchw(dy), wf))


def fwd2(x, w):
    N, H, W, _ = x.shape
    _poison((N * co.out_size(H, 2) * co.out_size(W, 2) * w.shape[0], torch.bfloat16))
    out = _C().conv3x3s2_fwd(co.nchw(x), co.w_nchw(w), False)
    assert len(out) == 1, "stride-2 forward declined the shape"
    return _nhwc(out[0])


def dgrad2(dy, w, H, W):
    wf = _C().conv3x3_flip(co.w_nchw(w))
    _poison((dy.shape[0] * H * W * w.shape[2], torch.bfloat16))
    out = _C().conv3x3s2_dgrad(co.nchw(dy), wf, H, W)
    assert len(out) == 1, "stride-2 data gradient declined the shape"
    return _nhwc(out[0])


def wgrad(x, dy, stride):
    f = _C().conv3x3s1_wgrad if stride == 1 else _C().conv3x3s2_wgrad
    geo = _C().conv3x3_wgrad_geo(*x.shape, dy.shape[3], stride)
    if geo is not None:  # the split-K workspace and the result
        per = 9 * x.shape[3] * dy.shape[3]
        _poison((geo[3] * per, torch.float32), (per, torch.bfloat16))
    dw = f(co.nchw(x), co.nchw(dy))
    return None if dw is None else co.from_w_nchw(dw).contiguous()


@functools.lru_cache(maxsize=2)
def _exact_case(shape, stride, role, kind="ternary"):
    """The fixture's operands as the kernels take them (bf16, NHWC, on the device) and the exact float64 result,
    computed once and shared by the variant bits / tune settings."""
    N, H, W, Ci, Co = shape
    if role == "fwd":
        a, b = (_bf(t) for t in co.fwd_operands(shape, stride, kind))
        ref = co.conv_fwd(co.f64(a), co.f64(b), stride)
    elif role == "dgrad":
        a, b = (_bf(t) for t in co.dgrad_operands(shape, stride, kind))
        ref = co.conv_dgrad(co.f64(a), co.f64(b), H, W, stride)
    else:
        a, b = (_bf(t) for t in co.wgrad_operands(shape, stride, kind))
        ref = co.conv_wgrad(co.f64(a), co.f64(b), stride)
    assert ref.abs().max() <= co.TERNARY_MAX  # a precondition on the inputs
    if kind == "offset":
        assert ref.min() >= 0
    return a, b, ref


# ----------------------------------------------------------------------------- the paths the cases are named for
def test_cases_reach_the_variants_they_name():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for case in sorted(co.S1_CASES):
        _assert_variant(case)
    for case in EXPECT_NO_WSR:
        with _opt(OPT_DEFAULT & ~32):
            _assert_variant(case, OPT_DEFAULT & ~32)
    def tiles(case, rows):
        N, H, W = co.S1_CASES[case][:3]
        return -(-N * H * W // rows)
    assert [tiles(c, 256) for c in (2, 3, 4, 5, 7)] == [1, 6, 1, 3, 2]
    assert tiles(6, 256) * (512 // 128) == 260
    # persistent kernels: more tiles than workgroups, so some workgroups walk two tiles
    assert tiles(8, 256) == 262 and tiles(8, 256) > ncu
    assert tiles(9, 224) == 300 and tiles(9, 224) > ncu and tiles(10, 224) == 264 and tiles(10, 224) > ncu
    # the weight-stationary kernel's largest halo (of 640 rows): the host's bound at W = 56, reached by case 11
    assert co.halo_rows_bound(32, 56) == 580 and co.halo_rows_need(*co.S1_CASES[11][:3]) == 580
    with pytest.raises(RuntimeError):
        _C().conv3x3s1_variant(1, 8, 8, 48, 64)  # a shape conv3x3s1_fwd refuses


def test_poison_reaches_the_next_allocation():
    """``_poison`` does what the run helpers rely on: the next buffer of that size comes back full of NaN."""
    for n, dt in ((2 * 13 * 11 * 64, torch.bfloat16), (3 * 9 * 64 * 64, torch.float32)):
        _poison((n, dt))
        assert torch.empty(n, dtype=dt, device=DEV).isnan().all()


def test_flip_is_the_permutation():
    g = torch.Generator().manual_seed(5)
    for Co, Ci in ((64, 64), (128, 64), (64, 192)):
        w = _bf(torch.randn(Co, 9, Ci, generator=g))
        wf = _C().conv3x3_flip(co.w_nchw(w))
        assert wf.shape == (Ci, Co, 3, 3) and wf.is_contiguous(memory_format=torch.channels_last)
        n = int((wf != co.flip_ref(co.w_nchw(w))).sum())
        RECORD["flip"] = max(RECORD.get("flip", 0), n)
        print(f"ratio flip mismatches {n}")
        assert n == 0


# ----------------------------------------------------------------------------- stride 1, forward and data gradient
@pytest.mark.parametrize("case,opt", OPT_RUNS, ids=[f"case{c:02d}-opt{o}" for c, o in OPT_RUNS])
def test_s1_ternary_exact(case, opt):
    shape = co.S1_CASES[case]
    x, w, ref = _exact_case(shape, 1, "fwd")
    dy, wd, dref = _exact_case(shape, 1, "dgrad")
    with _opt(opt):
        vf, vd = _assert_variant(case, opt)
        y, dx = fwd1(x, w), dgrad1(dy, wd)
    _exact(y, ref, f"s1 case{case:02d} opt{opt} {vf} fwd ternary", rows=_rows(vf))
    _exact(dx, dref, f"s1 case{case:02d} opt{opt} {vd} dgrad ternary", rows=_rows(vd))


@pytest.mark.parametrize("case", co.S1_ONEHOT)
def test_s1_onehot(case):
    N, H, W, Ci, Co = shape = co.S1_CASES[case]
    vf, vd = _assert_variant(case)
    x = co.position_coded(N, H, W, Ci, device=DEV)
    for p in range(co.onehot_passes(Ci, Co)):
        w, tap, ch, sign = co.onehot_weights(Ci, Co, p, device=DEV)
        _exact(fwd1(_bf(x), _bf(w)), co.onehot_fwd_ref(x, tap, ch, sign), f"s1 case{case:02d} {vf} fwd onehot",
               rows=_rows(vf), tap=tap, ch=ch)
    dy = co.position_coded(N, H, W, Co, device=DEV)
    for p in range(co.onehot_passes(Ci, Co, dgrad=True)):
        w, tap, ch, sign = co.onehot_weights(Ci, Co, p, dgrad=True, device=DEV)
        # the data gradient runs the forward kernel with tap 8 - t: report the kernel's tap
        _exact(dgrad1(_bf(dy), _bf(w)), co.onehot_dgrad_ref(dy, tap, ch, sign, H, W),
               f"s1 case{case:02d} {vd} dgrad onehot", rows=_rows(vd), tap=8 - tap, ch=ch)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", co.S1_ENVELOPE)
def test_s1_envelope(case, kind):
    N, H, W, Ci, Co = shape = co.S1_CASES[case]
    vf, vd = _assert_variant(case)
    x, w = (_bf(t) for t in co.real_operands(shape, "fwd", kind))
    ref, mag = co.conv_fwd(co.f64(x), co.f64(w)), co.conv_fwd(co.f64(x).abs(), co.f64(w).abs())
    if kind == "cancel":
        assert ref.abs().median() < mag.median() / 32  # the reference nearly cancels (inputs only)
    _within(fwd1(x, w), ref, co.conv_envelope(ref, mag, 9 * Ci), f"s1 case{case:02d} {vf} fwd {kind}")
    del ref, mag
    dy, w = (_bf(t) for t in co.real_operands(shape, "dgrad", kind))
    ref, mag = co.conv_dgrad(co.f64(dy), co.f64(w), H, W), co.conv_dgrad(co.f64(dy).abs(), co.f64(w).abs(), H, W)
    if kind == "cancel":
        assert ref.abs().median() < mag.median() / 32
    _within(dgrad1(dy, w), ref, co.conv_envelope(ref, mag, 9 * Co), f"s1 case{case:02d} {vd} dgrad {kind}")


def _check_stats(part, ref, rows, name):
    """part [2, T, C] of the kernel against the statistics of the exact output (which y was shown to equal)."""
    s, m2, env = co.stats_oracle(ref, rows)
    assert part.shape == (2,) + tuple(s.shape) and part.dtype == torch.float32, (name, part.shape, s.shape)
    assert s.abs().max() <= 256 * 256
    _equal(part[0], s.float(), f"{name} sums")
    _within(part[1], m2, env, f"{name} m2")


@pytest.mark.parametrize("kind", ["ternary", "offset"])
@pytest.mark.parametrize("case", co.S1_STATS)
def test_s1_fwd_stats(case, kind):
    shape = co.S1_CASES[case]
    vf, _ = _assert_variant(case)
    x, w, ref = _exact_case(shape, 1, "fwd", kind)
    out = _C().conv3x3s1_fwd_stats(co.nchw(x), co.w_nchw(w))
    if len(out) == 1:  # the one-element fallback: only where no kernel with the epilogue runs
        assert vf in ("tap_wide", "tap_narrow"), vf
    assert len(out) == 2, f"case {case} ({vf}) has the statistics epilogue"
    y = _nhwc(out[0])
    name = f"s1 case{case:02d} {vf} stats {kind}"
    assert torch.equal(y, fwd1(x, w)), f"{name}: output differs from conv3x3s1_fwd's"
    _exact(y, ref, f"{name} y", rows=_rows(vf))
    _check_stats(out[1], ref, _rows(vf), name)


@pytest.mark.parametrize("case,opt", [(5, OPT_DEFAULT), (6, OPT_DEFAULT), (10, OPT_DEFAULT | 128)])
def test_s1_fwd_bnbwd(case, opt):
    N, H, W, Ci, Co = shape = co.S1_CASES[case]
    x, w, ref = _exact_case(shape, 1, "fwd")
    bx, mean, keep, mask = co.bn_inputs(N, H, W, Co)
    with _opt(opt):
        vf, _ = _assert_variant(case, opt)
        out = _C().conv3x3s1_fwd_bnbwd(co.nchw(x), co.w_nchw(w), co.nchw(_bf(bx)), mask.to(DEV), mean.to(DEV))
        plain = fwd1(x, w)
    assert len(out) == 2, f"case {case} ({vf}) has the backward-reduction epilogue"
    name = f"s1 case{case:02d} opt{opt} {vf} bnbwd"
    y = _nhwc(out[0])
    assert torch.equal(y, plain), f"{name}: output differs from conv3x3s1_fwd's"
    _exact(y, ref, f"{name} y", rows=_rows(vf))
    want = co.bnbwd_oracle(ref, bx.to(DEV), mean.to(DEV), keep.to(DEV), _rows(vf))
    assert want.abs().max() < 2 ** 24 and out[1].shape == want.shape, (out[1].shape, want.shape)
    _equal(out[1][0], want[0].float(), f"{name} sum dz")
    _equal(out[1][1], want[1].float(), f"{name} sum dz (x - mean)")
    # without a ReLU mask every bit counts as set
    if opt == OPT_DEFAULT:
        out = _C().conv3x3s1_fwd_bnbwd(co.nchw(x), co.w_nchw(w), co.nchw(_bf(bx)), None, mean.to(DEV))
        want = co.bnbwd_oracle(ref, bx.to(DEV), mean.to(DEV), torch.ones_like(keep).to(DEV), _rows(vf))
        _equal(out[1][1], want[1].float(), f"{name} no mask sum dz (x - mean)")


# ----------------------------------------------------------------------------- stride 2
S2_IDS = ["x".join(map(str, s)) for s in co.S2_CASES]


@pytest.mark.parametrize("shape", co.S2_CASES, ids=S2_IDS)
def test_s2_exact(shape):
    N, H, W, Ci, Co = shape
    tag = f"s2 {'x'.join(map(str, shape))}"
    for kind in ("ternary", "offset"):
        x, w, ref = _exact_case(shape, 2, "fwd", kind)
        y = fwd2(x, w)
        _exact(y, ref, f"{tag} fwd {kind}")
        out = _C().conv3x3s2_fwd(co.nchw(x), co.w_nchw(w), True)
        assert len(out) == 2
        assert torch.equal(_nhwc(out[0]), y), f"{tag}: output with statistics differs"
        _check_stats(out[1], ref, co.BM, f"{tag} stats {kind}")
    dy, w, ref = _exact_case(shape, 2, "dgrad")
    dx = dgrad2(dy, w, H, W)
    _exact(dx, ref, f"{tag} dgrad ternary", stride2_dgrad=True)
    bx, mean, keep, mask = co.bn_inputs(N, H, W, Ci)
    out = _C().conv3x3s2_dgrad(co.nchw(dy), _C().conv3x3_flip(co.w_nchw(w)), H, W, bn_x=co.nchw(_bf(bx)),
                               bn_mask=mask.to(DEV), bn_mean=mean.to(DEV))
    assert len(out) == 2
    assert torch.equal(_nhwc(out[0]), dx), f"{tag}: data gradient with bn_x differs"
    want = co.bnbwd_oracle(ref, bx.to(DEV), mean.to(DEV), keep.to(DEV), co.BM, phases=True)
    assert want.abs().max() < 2 ** 24 and out[1].shape == want.shape, (out[1].shape, want.shape)
    _equal(out[1][0], want[0].float(), f"{tag} dgrad sum dz")
    _equal(out[1][1], want[1].float(), f"{tag} dgrad sum dz (x - mean)")


@pytest.mark.parametrize("i", co.S2_ONEHOT, ids=[S2_IDS[i] for i in co.S2_ONEHOT])
def test_s2_onehot(i):
    N, H, W, Ci, Co = shape = co.S2_CASES[i]
    Ho, Wo = co.out_size(H, 2), co.out_size(W, 2)
    tag = f"s2 {S2_IDS[i]}"
    x = co.position_coded(N, H, W, Ci, device=DEV)
    for p in range(co.onehot_passes(Ci, Co)):
        w, tap, ch, sign = co.onehot_weights(Ci, Co, p, device=DEV)
        _exact(fwd2(_bf(x), _bf(w)), co.onehot_fwd_ref(x, tap, ch, sign, 2), f"{tag} fwd onehot", tap=tap, ch=ch)
    dy = co.position_coded(N, Ho, Wo, Co, device=DEV)
    for p in range(co.onehot_passes(Ci, Co, dgrad=True)):
        w, tap, ch, sign = co.onehot_weights(Ci, Co, p, dgrad=True, device=DEV)
        _exact(dgrad2(_bf(dy), _bf(w), H, W), co.onehot_dgrad_ref(dy, tap, ch, sign, H, W, 2), f"{tag} dgrad onehot",
               tap=tap, ch=ch, stride2_dgrad=True)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("i", co.S2_ENVELOPE, ids=[S2_IDS[i] for i in co.S2_ENVELOPE])
def test_s2_envelope(i, kind):
    N, H, W, Ci, Co = shape = co.S2_CASES[i]
    tag = f"s2 {S2_IDS[i]}"
    x, w = (_bf(t) for t in co.real_operands(shape, "fwd", kind, 2))
    ref, mag = co.conv_fwd(co.f64(x), co.f64(w), 2), co.conv_fwd(co.f64(x).abs(), co.f64(w).abs(), 2)
    if kind == "cancel":
        assert ref.abs().median() < mag.median() / 32
    _within(fwd2(x, w), ref, co.conv_envelope(ref, mag, 9 * Ci), f"{tag} fwd {kind}")
    dy, w = (_bf(t) for t in co.real_operands(shape, "dgrad", kind, 2))
    ref, mag = co.conv_dgrad(co.f64(dy), co.f64(w), H, W, 2), co.conv_dgrad(co.f64(dy).abs(), co.f64(w).abs(), H, W, 2)
    if kind == "cancel":
        assert ref.abs().median() < mag.median() / 32
    _within(dgrad2(dy, w, H, W), ref, co.conv_envelope(ref, mag, 9 * Co), f"{tag} dgrad {kind}")


# ----------------------------------------------------------------------------- weight gradient
WGRAD_RUNS = [(1, s) for s in co.WGRAD_S1_CASES] + [(2, s) for s in co.S2_CASES]
WGRAD_IDS = [f"s{st}-" + "x".join(map(str, s)) for st, s in WGRAD_RUNS]
SETTINGS = ("default", "one_split", "three_splits", "co_tile_64")


def _settings(shape, stride):
    """[(name, (target_wgs, co_tile))] of the runs of one weight-gradient case; nblk is the default geometry's."""
    N, H, W, Ci, Co = shape
    g = _C().conv3x3_wgrad_geo(N, H, W, Ci, Co, stride)
    assert g is not None and g == co.wgrad_geo(N, H, W, Ci, Co, stride), (shape, stride, g)
    nblk = (Co // g[4]) * (Ci // 64)
    runs = [("default", (0, 0)), ("one_split", (1, 0)), ("three_splits", (3 * nblk, 0))]
    if stride == 2:
        runs.append(("co_tile_64", (0, 64)))
    return runs


def _geo(shape, stride, name, tune):
    """The geometry under the tune now set, asserted to be what the setting is for."""
    N, H, W, Ci, Co = shape
    g = _C().conv3x3_wgrad_geo(N, H, W, Ci, Co, stride)
    assert g is not None and g == co.wgrad_geo(N, H, W, Ci, Co, stride, *tune), (shape, stride, name, g)
    R, ntiles, tps, nsplit, co_t = g
    assert (nsplit - 1) * tps < ntiles <= nsplit * tps
    if name == "one_split":
        assert (tps, nsplit) == (ntiles, 1), g
    elif name == "three_splits":  # three where the tiles allow: ceil(ntiles / 3) tiles each, the last split fewer
        assert tps == -(-ntiles // min(3, ntiles)) and nsplit == -(-ntiles // tps) and nsplit <= 3, g
        assert nsplit == 3 or ntiles < 5, g
    elif name == "co_tile_64":
        assert co_t == 64, g
    else:
        assert co_t == (128 if Co % 128 == 0 else 64), g
    return g


def test_wgrad_geometry_of_the_named_cases():
    C_ = _C()
    assert C_.conv3x3_wgrad_geo(2, 56, 56, 64, 64, 1) == (2, 56, 1, 56, 64)
    with _tune(3, 0):   # 19 / 19 / 18 tiles
        assert C_.conv3x3_wgrad_geo(2, 56, 56, 64, 64, 1) == (2, 56, 19, 3, 64)
    with _tune(1, 0):
        assert C_.conv3x3_wgrad_geo(2, 56, 56, 64, 64, 1) == (2, 56, 56, 1, 64)
        assert C_.conv3x3_wgrad_geo(7, 14, 14, 256, 256, 1) == (8, 13, 13, 1, 128)
    with _tune(0, 64):
        assert C_.conv3x3_wgrad_geo(9, 14, 14, 128, 128, 2)[4] == 64
    assert C_.conv3x3_wgrad_geo(2, 56, 56, 64, 64, 1) == (2, 56, 1, 56, 64)  # the tune was restored


@pytest.mark.parametrize("stride,shape", WGRAD_RUNS, ids=WGRAD_IDS)
def test_wgrad_exact(stride, shape):
    N, H, W, Ci, Co = shape
    Ho, Wo = co.out_size(H, stride), co.out_size(W, stride)
    x, dy, ref = _exact_case(shape, stride, "wgrad")
    xc = co.position_coded(N, H, W, Ci, device=DEV)
    for name, tune in _settings(shape, stride):
        with _tune(*tune):
            R, ntiles, tps, nsplit, co_t = _geo(shape, stride, name, tune)
            tag = f"wgrad s{stride} {'x'.join(map(str, shape))} {name}"
            dw = wgrad(x, dy, stride)
            assert dw is not None, f"{tag}: the kernel declined a shape its geometry query takes"
            _exact_dw(dw, ref, f"{tag} ternary")
            pixels = co.impulse_pixels(N, Ho, Wo, R, tps)
            for p in range(co.impulse_passes(Co, pixels)):
                idy, which, sign = co.impulse_dy(N, Ho, Wo, Co, pixels, p * Co, device=DEV)
                _exact_dw(wgrad(_bf(xc), _bf(idy), stride), co.impulse_wgrad_ref(xc, pixels, which, sign, stride),
                          f"{tag} impulse", R=R, Ho=Ho, tiles_per_split=tps, pixels=pixels, which=which)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("stride,shape",
                         [(1, s) for s in co.WGRAD_S1_ENVELOPE] + [(2, s) for s in co.WGRAD_S2_ENVELOPE],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_wgrad_envelope(stride, shape, kind):
    N, H, W, Ci, Co = shape
    Ho, Wo = co.out_size(H, stride), co.out_size(W, stride)
    x, dy = (_bf(t) for t in co.real_operands(shape, "wgrad", kind, stride))
    ref, mag = co.conv_wgrad(co.f64(x), co.f64(dy), stride), co.conv_wgrad(co.f64(x).abs(), co.f64(dy).abs(), stride)
    if kind == "cancel":
        assert ref.abs().median() < mag.median() / 32
    for name, tune in _settings(shape, stride):
        with _tune(*tune):
            nsplit = _geo(shape, stride, name, tune)[3]
            dw = wgrad(x, dy, stride)
            assert dw is not None
            _within(dw, ref, co.conv_envelope(ref, mag, N * Ho * Wo, nsplit),
                    f"wgrad s{stride} {'x'.join(map(str, shape))} {name} {kind}")


def test_wgrad_declined_shapes_are_declared():
    """Where the geometry query declines, so does the binding; every such shape is listed, none of the cases is."""
    for shape, stride in co.EXPECT_DECLINED:
        N, H, W, Ci, Co = shape
        assert _C().conv3x3_wgrad_geo(N, H, W, Ci, Co, stride) is None and co.wgrad_geo(N, H, W, Ci, Co, stride) is None
        x, dy = (_bf(t) for t in co.wgrad_operands(shape, stride))
        assert wgrad(x, dy, stride) is None, (shape, stride)
    for stride, shape in WGRAD_RUNS:
        assert (shape, stride) not in co.EXPECT_DECLINED
        assert _C().conv3x3_wgrad_geo(*shape, stride) is not None, (shape, stride)
