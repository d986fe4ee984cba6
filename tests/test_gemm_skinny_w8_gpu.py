"""The W8A16 skinny GEMM and its row-wise e4m3 quantiser (csrc/kernels/gemm_skinny_w8.hip) on the MI355X against
tests/gemm_oracle.py: bit for bit on exact operands with power-of-two scales, inside the any-order envelope on
real ones (reference taken from the quantised bytes), quantiser bytes equal to the CPU formula, the SwiGLU
epilogue equal to the SwiGLU kernel on the unfused output, rows past M untouched, the same bits every launch and
replay. The kernel's chunk is 256 wide (two 128-wide steps), so K = 128 is a single step with fewer chunks than
waves, 640 three chunks over four waves with a partial last one, 768 three full chunks, 1152 five chunks with a
partial last one (uneven round-robin); 1536 and 2688 are more turns of the ring. PDT_SKINNY_RATIOS=<path> keeps
the worst ratio per name (profiles/r22/skinny_w8_oracle_ratios.txt)."""
import os

import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}
# (M, N, K, splits): splits 0 is the kernel's own rule; K = 128 has one chunk, so its 2 comes out as 1
CASES = [(1, 16, 128, 0), (3, 48, 640, 0), (16, 16, 768, 2), (17, 48, 1152, 3), (33, 16, 1152, 1), (64, 48, 768, 3),
         (64, 16, 640, 2), (17, 16, 128, 2), (3, 48, 2688, 2), (33, 48, 1536, 0), (16, 48, 1152, 0), (1, 48, 2688, 1)]
ONEHOT = [(17, 48, 1152, 3), (64, 16, 640, 2)]


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


def _scale(N):
    return 2.0 ** ((torch.arange(N) % 8) - 3).float()  # powers of two that differ by row


def _run(a, b, scale, mode=0, splits=0):
    """a bf16-exact, b e4m3-exact fp32 CPU operands."""
    return _C().gemm_skinny_w8(a.to(DEV, torch.bfloat16), b.to(DEV).to(torch.float8_e4m3fn), scale.to(DEV), mode,
                               splits).cpu()


def _quantised(M, N, K, kind="randn", seed=0, gain=1.0):
    """(x bf16, wq, scale) on the GPU, the weight quantised by the op under test."""
    a, b = go.real_operands(M, N, K, kind, seed=seed)
    wq, scale = _C().quantize_rows_e4m3(b.to(DEV, torch.bfloat16))
    return (gain * a).to(DEV, torch.bfloat16), wq, scale


def _ids(c):
    return "M{}-N{}-K{}-s{}".format(*c)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_ternary_operands_are_exact(case):
    M, N, K, sp = case
    a, b = go.ternary(M, N, K)
    s = _scale(N)
    ref = (go.f64(a) @ go.f64(b).t()) * s.double()
    assert (go.f64(a) @ go.f64(b).t()).abs().max() <= go.TERNARY_MAX
    go.assert_exact(_run(a, b, s, 0, sp), ref, name=f"ternary {_ids(case)}", record=RECORD, bn=16, kstep=128)


@pytest.mark.parametrize("case", ONEHOT, ids=_ids)
def test_onehot_probes_are_exact_in_both_roles(case):
    M, N, K, sp = case
    s = _scale(N)
    for p in range(go.onehot_passes(N, K)):  # W one-hot, X coded
        rows, k, sign = go.onehot(N, K, p)
        coded = go.position_coded(M, K)
        go.assert_exact(_run(coded, rows, s, 0, sp), go.onehot_ref(coded, k, sign, True) * s.double(),
                        name=f"onehot W {_ids(case)}", record=RECORD, bn=16, kstep=128, k_of=lambda m, n: k[n])
    for p in range(go.onehot_passes(M, K)):  # X one-hot, W coded in e4m3-exact values
        rows, k, sign = go.onehot(M, K, p)
        coded = go.position_coded(N, K, fp8=True)
        go.assert_exact(_run(rows, coded, s, 0, sp), go.onehot_ref(coded, k, sign, False) * s.double(),
                        name=f"onehot X {_ids(case)}", record=RECORD, bn=16, kstep=128, k_of=lambda m, n: k[m])


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_real_operands_stay_inside_the_envelope(case, kind):
    M, N, K, sp = case
    a, b = go.real_operands(M, N, K, kind, fp8=False)
    wq, scale = _C().quantize_rows_e4m3(b.to(DEV, torch.bfloat16))
    S = _C().gemm_skinny_w8_geo(M, N, K, 0, sp)[0]
    P, E = go.products(a, wq.cpu().float())  # the reference is taken from the bytes the kernel reads
    ref, env = go.gemm_envelope(P, E, K, scale=scale.cpu().double()[None, :], ksplit=S + 4)
    got = _C().gemm_skinny_w8(a.to(DEV, torch.bfloat16), wq, scale, 0, sp).cpu()
    name = f"{kind} {_ids(case)}"
    try:
        go.assert_within(got.double(), ref, env, 1.0, go.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


def _special_rows(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g)
    w[1] = 0.0                                                   # a zero row: scale 1, bytes 0
    w[2] = (w[2] * 2.0 ** -23).clamp(-2.0 ** -20, 2.0 ** -20)    # amax exactly 2^-20
    w[2, 5] = -2.0 ** -20
    w[3, 7] = 3e38                                               # inv underflows everything else to e4m3 zero
    return w.to(torch.bfloat16)


@pytest.mark.parametrize("N,K", [(16, 128), (48, 640)])
def test_quantiser_equals_the_cpu_formula_bit_for_bit(N, K):
    from pytorch_distributed_training_example_amd.ops import linear as L
    w = _special_rows(N, K)
    wq, scale = L.quantize_rows_e4m3(w.to(DEV))
    wq_c, scale_c = L.quantize_rows_e4m3(w)
    assert wq.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (N,)
    assert torch.equal(scale.cpu().view(torch.int32), scale_c.view(torch.int32))
    assert torch.equal(wq.cpu().view(torch.uint8), wq_c.view(torch.uint8))
    deq, amax = wq.cpu().float().double() * scale.cpu().double()[:, None], w.double().abs().amax(1)
    assert torch.isfinite(deq).all() and scale[1] == 1.0 and not wq.cpu().float()[1].any()
    assert scale[2] == 2.0 ** -20 / 448 and (wq.cpu().float()[3] != 0).sum() == 1
    # half an e4m3 ulp in the top binade is 16 / 448 = 1 / 28 of amax; tiny: scale and 448 / amax carry three fp32
    # roundings, 3 2^-24 relative on a grid point of at most amax
    assert ((deq - w.double()).abs() <= amax[:, None] * (1 / 28 + 2.0 ** -20)).all()
    with pytest.raises(ValueError, match="NaN or Inf"):
        L.quantize_rows_e4m3(torch.full((16, 128), float("inf"), dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M,F,K", [(3, 16, 640), (17, 48, 2688), (64, 48, 1536), (33, 16, 128)])
def test_swiglu_mode_equals_the_swiglu_kernel_on_the_unfused_output(M, F, K, splits):
    x, wq, scale = _quantised(M, 2 * F, K, seed=3, gain=4.0)  # gates over +-6: sigma well off 1/2
    plain = _C().gemm_skinny_w8(x, wq, scale, 0, splits)
    assert plain[:, :F].float().abs().max() > 6
    fused = _C().gemm_skinny_w8(x, wq, scale, 1, splits)
    want = _C().swiglu_fwd(plain)
    assert fused.shape == (M, F) and torch.equal(fused.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [(3, 64, 640, 0), (17, 32, 1152, 2), (33, 32, 768, 3)], ids=_ids)
def test_rows_past_m_are_neither_read_nor_written(case, mode):
    M, N, K, sp = case
    x, wq, scale = _quantised(M, N, K, seed=5)
    xbuf = torch.full((64 + 16, K), float("nan"), device=DEV, dtype=torch.bfloat16)  # NaN behind the M rows
    xbuf[:M] = x
    No = N // 2 if mode else N
    ybuf = torch.full((64 + 16, No), -512.0, device=DEV, dtype=torch.bfloat16)
    y = _C().gemm_skinny_w8(xbuf[:M], wq, scale, mode, sp, ybuf[:M])
    want = _C().gemm_skinny_w8(x, wq, scale, mode, sp)  # the same rows with nothing behind them
    assert torch.isfinite(y.float()).all() and torch.equal(y, want)
    assert (ybuf[M:] == -512.0).all()


@pytest.mark.parametrize("mode,sp", [(0, 3), (1, 2)])
def test_launches_and_graph_replays_give_the_same_bits(mode, sp):
    x, wq, scale = _quantised(17, 96, 1152, "cancel", seed=7)  # F = 48 in SwiGLU mode
    assert _C().gemm_skinny_w8_geo(17, 96, 1152, mode, sp)[0] == sp
    want = _C().gemm_skinny_w8(x, wq, scale, mode, sp)
    assert torch.equal(_C().gemm_skinny_w8(x, wq, scale, mode, sp), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _C().gemm_skinny_w8(x, wq, scale, mode, sp)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(on_side, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _C().gemm_skinny_w8(x, wq, scale, mode, sp)
    for _ in range(3):
        out.fill_(0)
        graph.replay()
        assert torch.equal(out, want)
    torch.cuda.synchronize()


def test_geometry_and_refusals():
    C = _C()
    assert [C.gemm_skinny_w8_geo(m, 48, 768, 0, 0)[2] for m in (1, 16, 17, 32, 33, 64)] == [1, 1, 2, 2, 4, 4]
    assert C.gemm_skinny_w8_geo(8, 16, 128, 0, 2)[0] == 1 and C.gemm_skinny_w8_geo(8, 16, 1152, 0, 3)[0] == 3
    assert C.gemm_skinny_w8_geo(8, 32000, 1024, 0, 0) == [1, 2, 1]  # enough tiles: no split, two tiles per workgroup
    assert C.gemm_skinny_w8_geo(8, 1024, 1024, 1, 0)[1] == 2  # SwiGLU: gate and up tiles in pairs
    x = torch.zeros(8, 256, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(64, 256, device=DEV, dtype=torch.float8_e4m3fn)
    s = torch.ones(64, device=DEV)
    flat_x = torch.zeros(8 * 256 + 8, device=DEV, dtype=torch.bfloat16)
    flat_w = torch.zeros(64 * 256 + 16, device=DEV, dtype=torch.float8_e4m3fn)
    bad = [(x.float(), w, s, 0), (x, w.to(torch.bfloat16), s, 0),                       # dtypes
           (x, w.cpu(), s, 0), (x.cpu(), w, s, 0), (x, w, s.cpu(), 0),                  # devices
           (torch.zeros(65, 256, device=DEV, dtype=torch.bfloat16), w, s, 0),           # M > 64
           (x, w[:24], s[:24], 0),                                                      # N % 16
           (x[:, :64].contiguous(), w[:, :64].contiguous(), s, 0),                      # K % 128
           (x[:, :128].contiguous(), w[:, ::2], s, 0), (x[:, ::2], w[:, :128].contiguous(), s, 0),  # not contiguous
           (flat_x[4:-4].view(8, 256), w, s, 0), (x, flat_w[8:-8].view(64, 256), s, 0),  # misaligned
           (x, w, s.double(), 0), (x, w, s[:48], 0), (x, w, s[:, None], 0),             # scale: fp32 [N]
           (x, w[:48], s[:48], 1), (x, w, s, 2)]                                        # SwiGLU N % 32; mode
    for xa, wa, sa, mode in bad:
        with pytest.raises(RuntimeError, match="gemm_skinny_w8"):
            C.gemm_skinny_w8(xa, wa, sa, mode, 0)
    with pytest.raises(RuntimeError, match="gemm_skinny_w8.*2\\^31"):
        C.gemm_skinny_w8_geo(1, 1 << 24, 128, 0, 0)  # a weight of 2^31 bytes
