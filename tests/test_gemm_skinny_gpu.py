"""The weight-streaming skinny GEMM (csrc/kernels/gemm_skinny.hip) on the MI355X against tests/gemm_oracle.py:
bit for bit on integer operands, inside the any-order envelope on real ones, the SwiGLU epilogue equal to the
SwiGLU kernel on the unfused output, rows past M untouched, the same bits every launch and replay. Shapes: M at
and past each column-tile boundary (16, 32), N of one and three feature tiles, K = 64 (fewer chunks than waves),
320 (a partial last chunk), 768 (3 chunks over 4 waves), 1088 (5 chunks, uneven round-robin and a partial one).
Every comparison prints ``ratio <name> <value>``; PDT_SKINNY_RATIOS=<path> keeps the worst per name
(profiles/r21/skinny_oracle_ratios.txt)."""
import os

import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}
# (M, N, K, splits): splits 0 is the kernel's own rule; K = 64 has one chunk, so its 2 comes out as 1
CASES = [(1, 16, 64, 0), (3, 48, 320, 0), (16, 16, 768, 2), (17, 48, 1088, 3), (33, 16, 1088, 1), (64, 48, 768, 3),
         (64, 16, 320, 2), (17, 16, 64, 2), (3, 48, 1088, 2), (33, 48, 768, 0), (16, 48, 1088, 0)]
ONEHOT = [c for c in CASES if c[0] >= 16 and c[2] > 64]  # passes = ceil(K / rows): kept to a few dozen launches


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    path = os.environ.get("PDT_SKINNY_RATIOS")
    if path and RECORD:
        with open(path, "w") as f:
            for name in sorted(RECORD):
                f.write(f"{name:<44} {RECORD[name]:.4g}\n")


def _C():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _run(a, b, mode=0, splits=0):
    return _C().gemm_skinny(a.to(DEV, torch.bfloat16), b.to(DEV, torch.bfloat16), mode, splits).cpu()


def _ids(c):
    return "M{}-N{}-K{}-s{}".format(*c)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_ternary_operands_are_exact(case):
    M, N, K, sp = case
    a, b = go.ternary(M, N, K)
    ref = go.f64(a) @ go.f64(b).t()
    assert ref.abs().max() <= go.TERNARY_MAX
    go.assert_exact(_run(a, b, 0, sp), ref, name=f"ternary {_ids(case)}", record=RECORD, bn=16)


@pytest.mark.parametrize("case", ONEHOT, ids=_ids)
def test_onehot_probes_are_exact_in_both_roles(case):
    M, N, K, sp = case
    for p in range(go.onehot_passes(N, K)):  # W one-hot, X coded
        rows, k, sign = go.onehot(N, K, p)
        coded = go.position_coded(M, K)
        go.assert_exact(_run(coded, rows, 0, sp), go.onehot_ref(coded, k, sign, True), name=f"onehot W {_ids(case)}",
                        record=RECORD, bn=16, k_of=lambda m, n: k[n])
    for p in range(go.onehot_passes(M, K)):  # X one-hot, W coded
        rows, k, sign = go.onehot(M, K, p)
        coded = go.position_coded(N, K)
        go.assert_exact(_run(rows, coded, 0, sp), go.onehot_ref(coded, k, sign, False), name=f"onehot X {_ids(case)}",
                        record=RECORD, bn=16, k_of=lambda m, n: k[m])


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_real_operands_stay_inside_the_envelope(case, kind):
    M, N, K, sp = case
    a, b = go.real_operands(M, N, K, kind)
    S = _C().gemm_skinny_geo(M, N, K, 0, sp)[0]
    ref, env = go.gemm_envelope(*go.products(a, b), K, ksplit=S + 4)  # S splits, 4 waves: any order is allowed
    name = f"{kind} {_ids(case)}"
    try:
        go.assert_within(_run(a, b, 0, sp).double(), ref, env, 1.0, go.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M,F,K", [(3, 16, 320), (17, 48, 1088), (64, 48, 768), (33, 16, 64)])
def test_swiglu_mode_equals_the_swiglu_kernel_on_the_unfused_output(M, F, K, splits):
    a, b = go.real_operands(M, 2 * F, K, "randn", seed=3)
    a, b = (4 * a).to(DEV, torch.bfloat16), b.to(DEV, torch.bfloat16)  # gates over +-6: sigma well off 1/2
    fused = _C().gemm_skinny(a, b, 1, splits)
    want = _C().swiglu_fwd(_C().gemm_skinny(a, b, 0, splits))
    assert fused.shape == (M, F) and torch.equal(fused.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [(3, 64, 320, 0), (17, 32, 1088, 2), (33, 32, 768, 3)], ids=_ids)
def test_rows_past_m_are_neither_read_nor_written(case, mode):
    M, N, K, sp = case
    a, b = go.real_operands(M, N, K, "randn", seed=5)
    b = b.to(DEV, torch.bfloat16)
    xbuf = torch.full((64 + 16, K), float("nan"), device=DEV, dtype=torch.bfloat16)  # NaN behind the M rows
    xbuf[:M] = a.to(DEV, torch.bfloat16)
    No = N // 2 if mode else N
    ybuf = torch.full((64 + 16, No), -512.0, device=DEV, dtype=torch.bfloat16)
    y = _C().gemm_skinny(xbuf[:M], b, mode, sp, ybuf[:M])
    want = _C().gemm_skinny(xbuf[:M].clone(), b, mode, sp)  # the same rows with nothing behind them
    assert torch.isfinite(y.float()).all() and torch.equal(y, want)
    assert (ybuf[M:] == -512.0).all()


def test_launches_and_graph_replays_give_the_same_bits():
    M, N, K = 17, 96, 1088  # F = 48 in SwiGLU mode
    a, b = go.real_operands(M, N, K, "cancel", seed=7)
    a, b = a.to(DEV, torch.bfloat16), b.to(DEV, torch.bfloat16)
    for mode, sp in [(0, 0), (0, 3), (1, 2)]:
        want = _C().gemm_skinny(a, b, mode, sp)
        assert torch.equal(_C().gemm_skinny(a, b, mode, sp), want)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _C().gemm_skinny(a, b, mode, sp)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _C().gemm_skinny(a, b, mode, sp)
        for _ in range(3):
            out.fill_(0)
            graph.replay()
            assert torch.equal(out, want)
    torch.cuda.synchronize()


def test_geometry_and_refusals():
    C = _C()
    assert [C.gemm_skinny_geo(m, 48, 768, 0, 0)[2] for m in (1, 16, 17, 32, 33, 64)] == [1, 1, 2, 2, 4, 4]
    assert C.gemm_skinny_geo(8, 16, 64, 0, 2)[0] == 1 and C.gemm_skinny_geo(8, 16, 1088, 0, 3)[0] == 3
    assert C.gemm_skinny_geo(8, 32000, 1024, 0, 0)[0] == 1  # enough tiles: no split
    x = torch.zeros(8, 128, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(64, 128, device=DEV, dtype=torch.bfloat16)
    bad = [(x.float(), w, 0), (torch.zeros(65, 128, device=DEV, dtype=torch.bfloat16), w, 0), (x, w[:24], 0),
           (x[:, :96].contiguous(), w[:, :96].contiguous(), 0), (x[:, :64].contiguous(), w[:, ::2], 0), (x[:, ::2], w[:, :64].contiguous(), 0),
           (x, w[:48], 1), (x, w, 2)]
    for xa, wa, mode in bad:
        with pytest.raises(RuntimeError, match="gemm_skinny"):
            C.gemm_skinny(xa, wa, mode, 0)


def test_linear_skinny_runs_the_kernel_and_counts():
    from pytorch_distributed_training_example_amd.ops import linear as L
    x = torch.randn(2, 4, 128, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(64, 128, device=DEV, dtype=torch.bfloat16)
    n0 = L.SKINNY_STATS["native_calls"]
    with torch.no_grad():
        y, z = L.linear_skinny(x, w), L.linear_skinny(x, w, swiglu=True, splits=1)
    assert L.SKINNY_STATS["native_calls"] == n0 + 2 and L.SKINNY_STATS["geo"] == (1, 2, 1)
    assert y.shape == (2, 4, 64) and z.shape == (2, 4, 32)
    assert torch.equal(y.view(8, 64), _C().gemm_skinny(x.view(8, 128), w, 0, 0))
    big = torch.randn(65, 128, device=DEV, dtype=torch.bfloat16)
    assert not L.skinny_ok(big, w) and torch.equal(L.linear_skinny(big, w), torch.nn.functional.linear(big, w))
    assert L.SKINNY_STATS["native_calls"] == n0 + 2
