"""The W4A16 skinny GEMM and its group-wise int4 quantiser (csrc/kernels/gemm_skinny_w4.hip) on the MI355X against
tests/gemm_oracle.py: bit for bit on exact operands with power-of-two scales that differ by row and by group,
one-hot probes that name the k of a misplaced nibble, inside the any-order envelope on real operands (reference
taken from the dequantised bytes), quantiser bytes equal to the torch formula, the SwiGLU epilogue equal to the
SwiGLU kernel on the unfused output, rows past M untouched, the same bits every launch and replay. The seams are
the 256-wide chunk and the 128-wide group: K = 256 is one chunk and three idle waves, 768 three chunks over four
waves, 1280 five (uneven round-robin), 2816 eleven (more than one turn of the ring); M sits at the column-tile
boundaries. PDT_SKINNY_RATIOS=<path> keeps the worst ratio per name (profiles/r26/skinny_w4_gemm.txt)."""
import os

import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = {}
# (M, N, K, splits): splits 0 is the kernel's own rule; K = 256 has one chunk, so its 2 comes out as 1
CASES = [(1, 16, 256, 0), (3, 48, 768, 0), (16, 16, 768, 2), (17, 48, 1280, 3), (33, 16, 1280, 1), (64, 48, 768, 3),
         (64, 16, 256, 2), (3, 48, 2816, 2), (33, 48, 2816, 0), (1, 48, 1280, 1)]
ONEHOT = [(17, 48, 1280, 3), (64, 16, 256, 2)]


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


def _L():
    from pytorch_distributed_training_example_amd.ops import linear
    return linear


def _scale(N, K):
    """[K / 128, N] powers of two that differ by row and by group."""
    return 2.0 ** (((torch.arange(N)[None, :] + 3 * torch.arange(K // 128)[:, None]) % 8) - 3).float()


def _run(a, q, scale, mode=0, splits=0):
    """a bf16-exact fp32, q integer-valued fp32 in [-7, 7], CPU operands."""
    return _C().gemm_skinny_w4(a.to(DEV, torch.bfloat16), _L().pack_int4(q.to(torch.int8)).to(DEV), scale.to(DEV), mode,
                               splits).cpu()


def _grouped_ref(a, q, scale):
    """(sum_g scale[g, n] (a_g q_g^T), max |a_g q_g^T|) in float64."""
    M, K = a.shape
    part = torch.einsum("mgk,ngk->gmn", go.f64(a).view(M, K // 128, 128), go.f64(q).view(-1, K // 128, 128))
    return (part * scale.double()[:, None, :]).sum(0), part.abs().max()


def _quantised(M, N, K, kind="randn", seed=0, gain=1.0):
    """(x bf16, wq, scale) on the GPU, the weight quantised by the op under test."""
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
    ref, pmax = _grouped_ref(a, b, s)
    assert pmax <= go.TERNARY_MAX
    go.assert_exact(_run(a, b, s, 0, sp), ref, name=f"ternary {_ids(case)}", record=RECORD, bn=16, kstep=256)


@pytest.mark.parametrize("case", ONEHOT, ids=_ids)
def test_onehot_probes_are_exact_in_both_roles(case):
    M, N, K, sp = case
    s = _scale(N, K).double()
    for p in range(go.onehot_passes(N, K)):  # W one-hot, X coded
        rows, k, sign = go.onehot(N, K, p)
        coded = go.position_coded(M, K)
        go.assert_exact(_run(coded, rows, s.float(), 0, sp), go.onehot_ref(coded, k, sign, True) * s[k // 128, torch.arange(N)],
                        name=f"onehot W {_ids(case)}", record=RECORD, bn=16, kstep=256, k_of=lambda m, n: k[n])
    n_, k_ = torch.arange(N)[:, None], torch.arange(K)[None, :]
    coded = ((31 * n_ + 17 * k_) % 15 - 7).float()  # int4-exact
    for p in range(go.onehot_passes(M, K)):  # X one-hot, W coded
        rows, k, sign = go.onehot(M, K, p)
        go.assert_exact(_run(rows, coded, s.float(), 0, sp), go.onehot_ref(coded, k, sign, False) * s[k // 128],
                        name=f"onehot X {_ids(case)}", record=RECORD, bn=16, kstep=256, k_of=lambda m, n: k[m])


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_real_operands_stay_inside_the_envelope(case, kind):
    M, N, K, sp = case
    a, b = go.real_operands(M, N, K, kind, fp8=False)
    wq, scale = _C().quantize_groups_int4(b.to(DEV, torch.bfloat16))
    S = _C().gemm_skinny_w4_geo(M, N, K, 0, sp)[0]
    P, E = go.products(a, _L().dequantize_groups_int4(wq, scale).cpu())  # from the bytes the kernel reads
    ref, env = go.gemm_envelope(P, E, K, ksplit=S + 4 + K // 128)  # the W8 test's S + 4, one rounding per group fma
    got = _C().gemm_skinny_w4(a.to(DEV, torch.bfloat16), wq, scale, 0, sp).cpu()
    name = f"{kind} {_ids(case)}"
    try:
        go.assert_within(got.double(), ref, env, 1.0, go.FLOOR, name=name, record=RECORD)
    finally:
        print(f"ratio {name} {RECORD.get(name, float('nan')):.4g}")


@pytest.mark.parametrize("N,K", [(16, 512), (48, 768)])
def test_quantiser_equals_the_torch_formula_bit_for_bit(N, K):
    L = _L()
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K))
    w[1, :128] = 0.0                                                          # a zero group: scale 1, nibbles 0
    w[2, 128:256] = (w[2, 128:256] * 2.0 ** -23).clamp(-2.0 ** -20, 2.0 ** -20)
    w[2, 133] = -2.0 ** -20                                                   # amax exactly 2^-20
    w[3, 263] = 3e38                                                          # inv sends the rest of the group to 0
    w[4, :128] = torch.tensor([0.5, -0.5, 2.5, -2.5, 7.0, 1.5, -3.5, 6.5]).repeat(16)  # inv = 1: exact ties
    w = w.to(torch.bfloat16)
    wq, scale = L.quantize_groups_int4(w.to(DEV))
    wq_c, scale_c = L.quantize_groups_int4(w)
    assert wq.dtype == torch.uint8 and wq.shape == (N, K // 2) and scale.shape == (K // 128, N)
    assert torch.equal(scale.cpu().view(torch.int32), scale_c.view(torch.int32)) and torch.equal(wq.cpu(), wq_c)
    q = L.unpack_int4(wq.cpu())
    assert torch.equal(L.unpack_int4(L.pack_int4(q)), q) and q.abs().max() == 7
    assert scale[0, 1] == 1.0 and not q[1, :128].any() and scale[1, 2] == 2.0 ** -20 / 7
    assert (q[3, 256:384] != 0).sum() == 1 and q[4, :8].tolist() == [0, 0, 2, -2, 7, 2, -4, 6]
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="NaN or Inf"):
            L.quantize_groups_int4(torch.full((16, 256), bad, dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("M,F,K", [(3, 16, 768), (17, 48, 2816), (64, 48, 1280), (33, 16, 256)])
def test_swiglu_mode_equals_the_swiglu_kernel_on_the_unfused_output(M, F, K, splits):
    x, wq, scale = _quantised(M, 2 * F, K, seed=3, gain=4.0)  # gates over +-6: sigma well off 1/2
    plain = _C().gemm_skinny_w4(x, wq, scale, 0, splits)
    assert plain[:, :F].float().abs().max() > 6
    fused = _C().gemm_skinny_w4(x, wq, scale, 1, splits)
    want = _C().swiglu_fwd(plain)
    assert fused.shape == (M, F) and torch.equal(fused.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("M,N,K,sp,mode", [(3, 64, 768, 0, 0), (17, 96, 1280, 3, 0), (33, 32, 768, 2, 1)])
def test_guard_bands_hold_and_launches_and_replays_give_the_same_bits(M, N, K, sp, mode):
    x, wq, scale = _quantised(M, N, K, "cancel", seed=5)
    xbuf = torch.full((64 + 16, K), float("nan"), device=DEV, dtype=torch.bfloat16)  # NaN behind the M rows
    xbuf[:M] = x
    ybuf = torch.full((64 + 16, N // 2 if mode else N), -512.0, device=DEV, dtype=torch.bfloat16)
    want = _C().gemm_skinny_w4(x, wq, scale, mode, sp)  # the same rows with nothing behind them
    y = _C().gemm_skinny_w4(xbuf[:M], wq, scale, mode, sp, ybuf[:M])
    assert torch.isfinite(y.float()).all() and torch.equal(y, want) and (ybuf[M:] == -512.0).all()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _C().gemm_skinny_w4(x, wq, scale, mode, sp)
    for _ in range(3):
        out.fill_(0)
        graph.replay()
        assert torch.equal(out, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("what", ["K % 256", "N % 16", "M = 65", "scale shape", "wq not contiguous"])
def test_refusals_name_the_op(what):
    M, N, K = {"K % 256": (8, 64, 384), "N % 16": (8, 24, 512), "M = 65": (65, 64, 512)}.get(what, (8, 64, 512))
    x = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    wq = torch.zeros(N, K // 2, device=DEV, dtype=torch.uint8)
    s = torch.ones(K // 128, N, device=DEV)
    if what == "scale shape":
        s = s.t().contiguous()
    if what == "wq not contiguous":
        wq = torch.zeros(N, K, device=DEV, dtype=torch.uint8)[:, ::2]
    with pytest.raises(RuntimeError, match="gemm_skinny_w4"):
        _C().gemm_skinny_w4(x, wq, s, 0, 0)
