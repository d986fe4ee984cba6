"""The any-row W4A16 GEMM (csrc/kernels/gemm_w4.hip) on the MI355X against tests/gemm_oracle.py, as
tests/test_gemm_skinny_w4_gpu.py judges its skinny sibling: bit for bit on exact operands with power-of-two scales
that differ by row and group, one-hot probes that name the k of a misplaced nibble or token row, inside the
any-order envelope on real operands (reference from the dequantised bytes), rows past M never read or written, the
same bits on every replay. Seams: the token tile BM (64, or 128 from 128 tiles of 128 x 128 on: the two large
cases, with a last token tile of 1 and of 127 rows), the 128-feature tile with a partial last one (N = 16, 48,
144, 1808, 1840), one / several / uneven 256-wide K steps, forced splits. The printed ratios are kept in
profiles/r28/gemm_w4_tall.txt."""
import pytest
import torch

import gemm_oracle as go
from pytorch_distributed_training_example_amd.ops import linear as L
from pytorch_distributed_training_example_amd.ops._native import native as _C

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}
# (M, N, K, splits): splits 0 is the kernel's own rule
CASES = [(65, 16, 256, 0), (127, 48, 768, 0), (128, 144, 768, 2), (129, 48, 1280, 3), (200, 16, 1280, 1),
         (257, 144, 256, 0), (1, 16, 256, 0), (64, 48, 768, 0), (1025, 1840, 512, 2), (1151, 1808, 256, 0)]


def _scale(N, K):
    return 2.0 ** (((torch.arange(N)[None, :] + 3 * torch.arange(K // 128)[:, None]) % 8) - 3).float()


def _run(a, q, scale, splits=0):
    return _C().gemm_w4(a.to(DEV, torch.bfloat16), L.pack_int4(q.to(torch.int8)).to(DEV), scale.to(DEV), splits).cpu()


def _quantised(M, N, K, kind="randn", seed=0, gain=1.0):
    a, b = go.real_operands(M, N, K, kind, seed=seed)
    wq, scale = _C().quantize_groups_int4(b.to(DEV, torch.bfloat16))
    return (gain * a).to(DEV, torch.bfloat16), wq, scale


def _ids(c):
    return "M{}-N{}-K{}-s{}".format(*c)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_ternary_operands_are_exact(case):
    M, N, K, sp = case
    a, b = go.ternary(M, N, K)
    s = _scale(N, K)
    part = torch.einsum("mgk,ngk->gmn", go.f64(a).view(M, K // 128, 128), go.f64(b).view(N, K // 128, 128))
    assert part.abs().max() <= go.TERNARY_MAX
    go.assert_exact(_run(a, b, s, sp), (part * s.double()[:, None, :]).sum(0), name=f"ternary {_ids(case)}",
                    record=RECORD, bn=128, kstep=256)


@pytest.mark.parametrize("case", [(129, 48, 1280, 3), (257, 144, 256, 0)], ids=_ids)
def test_onehot_probes_are_exact_in_both_roles(case):
    M, N, K, sp = case
    s = _scale(N, K).double()
    for p in range(go.onehot_passes(N, K)):  # W one-hot, X coded
        rows, k, sign = go.onehot(N, K, p)
        coded = go.position_coded(M, K)
        go.assert_exact(_run(coded, rows, s.float(), sp), go.onehot_ref(coded, k, sign, True) * s[k // 128, torch.arange(N)],
                        name=f"onehot W {_ids(case)}", record=RECORD, bn=128, kstep=256, k_of=lambda m, n: k[n])
    n_, k_ = torch.arange(N)[:, None], torch.arange(K)[None, :]
    coded = ((31 * n_ + 17 * k_) % 15 - 7).float()  # int4-exact
    for p in range(go.onehot_passes(M, K)):  # X one-hot, W coded
        rows, k, sign = go.onehot(M, K, p)
        go.assert_exact(_run(rows, coded, s.float(), sp), go.onehot_ref(coded, k, sign, False) * s[k // 128],
                        name=f"onehot X {_ids(case)}", record=RECORD, bn=128, kstep=256, k_of=lambda m, n: k[m])


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_real_operands_stay_inside_the_envelope(case, kind):
    M, N, K, sp = case
    a, b = go.real_operands(M, N, K, kind, fp8=False)
    wq, scale = _C().quantize_groups_int4(b.to(DEV, torch.bfloat16))
    S, BM, BN = _C().gemm_w4_geo(M, N, K, sp)
    assert (BM, BN) == (128 if M > 1000 else 64, 128) and S == (sp or 1)  # the cases reach both tiles and the splits
    P, E = go.products(a, L.dequantize_groups_int4(wq, scale).cpu())  # from the bytes the kernel reads
    ref, env = go.gemm_envelope(P, E, K, ksplit=K // 128 + S)  # gemm_w4.hip's header: one per group fma, one per split
    got = _C().gemm_w4(a.to(DEV, torch.bfloat16), wq, scale, sp).cpu()
    name = f"{kind} {_ids(case)}"
    try:
        go.assert_within(got.double(), ref, env, 1.0, go.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


@pytest.mark.parametrize("M,N,K,sp", [(129, 96, 768, 0), (200, 144, 1280, 3)])
def test_guard_bands_hold_and_replays_give_the_same_bits(M, N, K, sp):
    x, wq, scale = _quantised(M, N, K, "cancel", seed=5)
    xbuf = torch.full((M + 130, K), float("nan"), device=DEV, dtype=torch.bfloat16)  # NaN behind the M rows
    xbuf[:M] = x
    ybuf = torch.full((M + 130, N), -512.0, device=DEV, dtype=torch.bfloat16)
    want = _C().gemm_w4(x, wq, scale, sp)  # the same rows with nothing behind them
    y = _C().gemm_w4(xbuf[:M], wq, scale, sp, ybuf[:M])
    assert torch.isfinite(y.float()).all() and torch.equal(y, want) and (ybuf[M:] == -512.0).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _C().gemm_w4(x, wq, scale, sp)
    for _ in range(3):
        out.fill_(0)
        graph.replay()
        assert torch.equal(out, want)


def test_linear_w4_swiglu_is_the_swiglu_kernel_on_this_kernels_output():
    x, wq, scale = _quantised(129, 96, 768, seed=3, gain=4.0)
    n0 = L.SKINNY_STATS["w4_tall_calls"]
    with torch.no_grad():
        fused = L.linear_w4(x, wq, scale, swiglu=True)
    want = _C().swiglu_fwd(_C().gemm_w4(x, wq, scale, 0))
    assert L.SKINNY_STATS["w4_tall_calls"] == n0 + 1 and L.SKINNY_STATS["geo"] == tuple(_C().gemm_w4_geo(129, 96, 768, 0))
    assert fused.shape == (129, 48) and torch.equal(fused.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("what", ["K % 256", "N % 16", "scale shape", "wq not contiguous"])
def test_refusals_name_the_op(what):
    M, N, K = {"K % 256": (80, 64, 384), "N % 16": (80, 24, 512)}.get(what, (80, 64, 512))
    x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    wq = torch.zeros(N, K // 2, device=DEV, dtype=torch.uint8)
    s = torch.ones(K // 128, N, device=DEV)
    s = s.t().contiguous() if what == "scale shape" else s
    wq = torch.zeros(N, K, device=DEV, dtype=torch.uint8)[:, ::2] if what == "wq not contiguous" else wq
    with pytest.raises(RuntimeError, match="gemm_w4"):
        _C().gemm_w4(x, wq, s, 0)
