"""The statistics-only 1x1-conv GEMM (csrc/kernels/conv1x1.hip NOST) and the persistent APPLY GEMM.

Statistics-only: ``conv1x1_gemm(..., stats=True, no_store=True)`` must return partials EQUAL (torch.equal) to the
storing call's for the same operands — the ALG backward's gradients with a bottleneck conv3 output written and
unwritten are compared bit for bit — and must not touch ``y``. Every tile (64 / 128 / 256 channels), the one-tile
kernel with a tail tile and each persistent variant, with a tile count that is no multiple of the grid (some
workgroups walk one tile more) and M no multiple of 256. Which kernel ran is asserted through
``conv1x1_last_persistent()``: 0 = one tile per workgroup, else waves per workgroup + 256 (statistics-only) + 512
(APPLY).

Persistent APPLY (the 8-wave tile staged in four parts, coefficients in LDS): bit-identical (output and ReLU
bits) to the one-tile kernel, with and without a deferred shortcut BatchNorm (``rab``), at the smallest M that
reaches it (>= 1024 tiles of 256 x 128) plus a tail, and against the fp32 formula of
tests/test_bn_apply_gemm_gpu.py::test_gemm_apply_matches_fp32 (same 1e-2 relative bound, same mask rule).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

NOST, APPLY = 256, 512


def _n():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


@functools.lru_cache(maxsize=None)
def _operands(M, K, N):
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    a = torch.randn(M, K, device="cuda", generator=g).bfloat16() + 0.25
    b = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    return a, b


def _stats_pair(M, K, N):
    """(storing partials, its y, which kernel), (statistics-only partials, its y, which kernel, y before)."""
    n = _n()
    a, b = _operands(M, K, N)
    y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    part = n.conv1x1_gemm(a, b, y, False, True)
    k_store = n.conv1x1_last_persistent()
    pattern = torch.full((M, N), -1.5, device="cuda", dtype=torch.bfloat16)
    pattern.view(-1)[::7] = 3.0
    y2 = pattern.clone()
    part2 = n.conv1x1_gemm(a, b, y2, False, True, no_store=True)
    k_nost = n.conv1x1_last_persistent()
    torch.cuda.synchronize()
    return (part, y, k_store), (part2, y2, k_nost, pattern)


def _check_stats_only(M, K, N, want_kernel):
    (part, y, k_store), (part2, y2, k_nost, pattern) = _stats_pair(M, K, N)
    assert k_store == want_kernel and k_nost == (want_kernel | NOST if want_kernel else 0), (k_store, k_nost)
    assert torch.equal(part2, part), "statistics-only partials differ from the storing kernel's"
    assert torch.equal(y2, pattern), "the statistics-only GEMM wrote to y"
    # and the partials are those of the values the storing kernel wrote: the last (tail) tile's channel sums.
    # Tolerance: <= 256 values of magnitude <= ~5 summed in fp32 in another order: 256 * 2^-24 * 1280 ~ 2e-2
    T = (M + 255) // 256
    rows = y[(T - 1) * 256:M].float()
    torch.testing.assert_close(part[0, T - 1], rows.sum(0), rtol=1e-4, atol=5e-2)


@pytest.mark.parametrize("M,K,N", [(1000, 64, 256), (777, 128, 512), (513, 64, 64)])
def test_stats_only_one_tile_equals_storing(M, K, N):
    """The one-tile kernels (128- and 64-channel tiles, a tail tile of 232 / 9 / 1 rows)."""
    _check_stats_only(M, K, N, 0)


def test_stats_only_persistent_256_equals_storing():
    """The 16-wave 256-channel persistent tile (the default for ResNet-50 layers 1-3 at the bench batch): 2049
    tiles over 256 workgroups, a tail tile of 77 rows. 67 MB read, nothing written."""
    _check_stats_only(2048 * 256 + 77, 64, 256, 16)


@pytest.mark.parametrize("M,K,N,waves", [(512 * 256 + 77, 64, 128, 8), (1024 * 256 + 77, 64, 64, 4)])
def test_stats_only_persistent_small_tiles_equal_storing(M, K, N, waves):
    """The 8- and 4-wave persistent tiles (``conv1x1_persist(2)``: every kind and tile persistent)."""
    n = _n()
    old = n.conv1x1_persist(2)
    try:
        _check_stats_only(M, K, N, waves)
    finally:
        n.conv1x1_persist(old)


def test_stats_only_needs_stats():
    """no_store without the statistics epilogue is an error, not a silent no-op."""
    a, b = _operands(513, 64, 64)
    y = torch.empty(513, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _n().conv1x1_gemm(a, b, y, False, False, no_store=True)


def _apply_inputs(M, K, N, rab):
    a, b = _operands(M, K, N)
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + (1 if rab else 0))
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    res = r(M, N).bfloat16()
    ab = torch.stack([r(N).abs() + 0.5, r(N) * 0.1])
    rabt = torch.stack([r(N).abs() + 0.5, r(N) * 0.1]) if rab else None
    return a, b, res, ab, rabt


@pytest.mark.parametrize("rab", [False, True])
@pytest.mark.parametrize("M,K,N", [(512 * 256 + 77, 64, 256), (256 * 256 + 77, 128, 512)])
def test_apply_persistent_equals_one_tile_and_fp32(M, K, N, rab):
    n = _n()
    a, b, res, ab, rabt = _apply_inputs(M, K, N, rab)
    old = n.conv1x1_persist(0)
    try:
        y0, m0 = n.conv1x1_gemm_apply(a, b, res, ab, rabt)
        k0 = n.conv1x1_last_persistent()
        n.conv1x1_persist(1)
        y1, m1 = n.conv1x1_gemm_apply(a, b, res, ab, rabt)
        k1 = n.conv1x1_last_persistent()
        torch.cuda.synchronize()
    finally:
        n.conv1x1_persist(old)
    assert k0 == 0 and k1 == (8 | APPLY), (k0, k1)
    assert torch.equal(y1, y0), "persistent APPLY output differs from the one-tile kernel's"
    assert torch.equal(m1, m0), "persistent APPLY ReLU bits differ from the one-tile kernel's"
    z = (a.float() @ b.float().t()).bfloat16().float()  # the conv output as the first GEMM stored it
    rr = res.float() if rabt is None else res.float() * rabt[0] + rabt[1]
    t = z * ab[0] + ab[1] + rr
    want = t.clamp_min(0)
    err = (y1.float() - want).norm() / want.norm()
    assert err < 1e-2, float(err)
    bits = (m1.view(-1, 1) >> torch.arange(8, device="cuda", dtype=torch.uint8)) & 1
    pos = bits.view(M, N).bool()
    sure = t.abs() > 0.05  # away from the ReLU threshold (z rounding differences)
    assert torch.equal(pos[sure], (t > 0)[sure])
    assert torch.equal(pos, y1.float() > 0) or bool(((y1.float() > 0) & ~pos).sum() == 0)


@pytest.mark.parametrize("hw", [8, 7])
def test_apply_gemm_block_writes_subsample(hw):
    """A stage's last bottleneck on the APPLY GEMM path still hands the next stage's strided shortcut its input:
    the output's stride-2 subsample (``_pdt_sub``) equals ``y[:, :, ::2, ::2]``, at 8 x 8 and 7 x 7 pixels."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.ops import batchnorm as bn_ops
    from pytorch_distributed_training_example_amd.ops.conv import subsample_of
    torch.manual_seed(0)
    net = to_bf16_mixed(get_model("resnet50").cuda().to(memory_format=torch.channels_last))
    blk = net.layer1[-1]
    assert blk.emit_sub == 2
    g = torch.Generator(device="cuda").manual_seed(hw)
    x = torch.randn(4, 256, hw, hw, device="cuda", generator=g).relu().bfloat16()
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    calls = []
    orig = bn_ops.native

    class Spy:
        def __getattr__(self, n):
            if n == "conv1x1_gemm_apply":
                calls.append(1)
            return getattr(orig(), n)
    bn_ops.native = lambda: Spy()
    try:
        y = blk(x)
    finally:
        bn_ops.native = orig
    assert calls, "the GEMM apply path did not run"
    ys = subsample_of(y, 2)
    assert ys is not None, "no subsample attached to the block output"
    assert torch.equal(ys, y[:, :, ::2, ::2])
