"""LayerNorm / add+LayerNorm (csrc/kernels/layernorm.hip) against the fp64 oracle, elementwise inside the
envelopes of tests/oracle_envelope.py: every supported width (so every RF = 4 and RF = 2 instantiation
of the backward, D = 2048 at exactly 64 KB of LDS), row counts below / at / just past one wave per
row-slot, and the row counts at which the backward's 512-workgroup cap sets an odd rows_per_block.
dgamma / dbeta are held to the worst case of any fp32 summation order, (N + 16) 2^-24 sum|terms|, and
run with *probe* gradients too: dy zero except on rows next to workgroup boundaries, so a row left
out of (or counted twice in) a partition is an O(1) relative error."""
import math

import pytest
import torch

import oracle_envelope as oe

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = [256 * k for k in (1, 2, 3, 4, 5, 6, 8)]
EPS = 1e-5


def _ln(D):
    from pytorch_distributed_training_example_amd.ops.layernorm import LayerNorm
    torch.manual_seed(D)
    ln = LayerNorm(D, eps=EPS).to(DEV)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_()
    return ln


def probe_rows(N, seed=0):
    """0, N-1, the rows on either side of the boundaries of the first, a middle and the last workgroup
    of the backward's partition (rows_per_block = ceil(N / min(512, ceil(N / 32)))), and 8 random rows."""
    rpb = math.ceil(N / min(512, math.ceil(N / 32)))
    nblk = math.ceil(N / rpb)
    rows = {0, N - 1}
    for m in {1, nblk // 2, nblk - 1}:
        rows |= {m * rpb - 1, m * rpb}
    g = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, N, (8,), generator=g).tolist())
    return sorted(r for r in rows if 0 <= r < N)


def _masked(t, rows):
    z = torch.zeros_like(t)
    z[rows] = t[rows]
    return z


def _run_and_compare(ln, x, dy, h=None, ds=None, tag=""):
    from pytorch_distributed_training_example_amd.ops.layernorm import add_layer_norm, layer_norm
    ln.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_()
    got = {}
    if h is None:
        y = layer_norm(xg, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
        assert type(y.grad_fn).__name__.startswith("_LNFn"), y.grad_fn  # the HIP kernel, not F.layer_norm
        y.backward(dy)
    else:
        hg = h.clone().requires_grad_()
        s, y = add_layer_norm(xg, hg, ln)
        assert type(y.grad_fn).__name__.startswith("_AddLNFn"), y.grad_fn
        torch.autograd.backward([s, y], [ds, dy])
        got["s"], got["dh"] = s.detach(), hg.grad
    got.update(y=y.detach(), dx=xg.grad, dw=ln.weight.grad, db=ln.bias.grad)
    ref, env = oe.layernorm_oracle(x, ln.weight.detach(), ln.bias.detach(), EPS, dy, h, ds)
    errors = []
    if h is not None:
        if not torch.equal(got["s"], ref["s"]):
            errors.append(f"{tag}: s = x + h differs from the correctly rounded sum")
        if not torch.equal(got["dh"], got["dx"]):
            errors.append(f"{tag}: dh != dx")
    for name, c in (("y", oe.LN_C), ("dx", oe.LN_C), ("dw", oe.LN_C_SUM), ("db", oe.LN_C_SUM)):
        try:
            r = oe.assert_within(got[name], ref[name], env[name], c, oe.FLOOR, name=f"{tag} {name}")
            print(f"ratio {tag} {name} {r:.4g}")
        except AssertionError as e:
            errors.append(str(e))
            print(f"FAIL {e}")
    assert not errors, "\n".join(errors)


def _data(N, D, dtype, fused, seed, mean=0.0, std=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda s=1.0: torch.randn(N, D, device=DEV, generator=g) * s  # noqa: E731
    x = (mean + std * r()).to(dtype)
    dy = r().to(dtype)
    h, ds = ((std * r()).to(dtype), r().to(dtype)) if fused else (None, None)
    return x, dy, h, ds


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", WIDTHS)
def test_small_row_counts(D, dtype, fused):
    """N in {1, 3, 4, 5, 33, 129}: fewer rows than waves, one full slot, one past it, two workgroups, five;
    dense and probe gradients."""
    ln = _ln(D)
    name = f"ln D={D} {'bf16' if dtype == torch.bfloat16 else 'fp32'} {'add' if fused else 'plain'}"
    for N in (1, 3, 4, 5, 33, 129):
        x, dy, h, ds = _data(N, D, dtype, fused, seed=N)
        _run_and_compare(ln, x, dy, h, ds, tag=f"{name} N={N} dense")
        rows = probe_rows(N)
        _run_and_compare(ln, x, _masked(dy, rows), h, None if ds is None else _masked(ds, rows),
                         tag=f"{name} N={N} probe")


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [256, 1280])
@pytest.mark.parametrize("N", [16385, 25216])
def test_capped_partition(N, D, dtype, fused):
    """N > 16384: the backward runs at its 512-workgroup cap with rows_per_block = 33 / 50, no multiple of
    the 4 RF rows a workgroup takes per step (D = 256: RF = 4, D = 1280: RF = 2). Probe gradients."""
    ln = _ln(D)
    x, dy, h, ds = _data(N, D, dtype, fused, seed=N)
    rows = probe_rows(N)
    assert len(rows) >= 12
    _run_and_compare(ln, x, _masked(dy, rows), h, None if ds is None else _masked(ds, rows),
                     tag=f"ln-cap D={D} {'bf16' if dtype == torch.bfloat16 else 'fp32'} "
                         f"{'add' if fused else 'plain'} N={N} probe")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [256, 768])
def test_empty_input(D, dtype):
    """x of shape [0, D] straight into the launchers (an empty micro-batch reaches them: the op's native-path
    test does not look at numel): empty y / s / dx, no statistics, and dgamma = dbeta = 0 exactly, with and
    without the residual branch. The backward's partition once divided by zero here, on the host."""
    from pytorch_distributed_training_example_amd.ops._native import native
    ln = _ln(D)
    w, b = ln.weight.detach(), ln.bias.detach()
    x = torch.empty(0, D, device=DEV, dtype=dtype)
    for fused in (False, True):
        other = torch.empty_like(x) if fused else None
        y, mean, rstd, s = native().ln_fwd(x, w, b, EPS, other)
        assert y.shape == (0, D) and y.dtype == dtype
        assert mean.shape == (0,) and rstd.shape == (0,) and mean.dtype == rstd.dtype == torch.float32
        assert (s.shape == (0, D) and s.dtype == dtype) if fused else s is None
        dx, dw, db = native().ln_bwd(torch.empty_like(x), x, w, mean, rstd, other)
        torch.cuda.synchronize()
        assert dx.shape == (0, D) and dx.dtype == dtype
        for g in (dw, db):
            assert g.shape == (D,) and g.dtype == torch.float32 and not bool(g.any()), "dgamma / dbeta of no rows"


@pytest.mark.parametrize("D", WIDTHS)
def test_large_mean_fp32(D):
    """x = 50 + 0.1 randn: the same bounds. A one-pass variance E[x^2] - mean^2 loses ~4 digits here and
    fails y and dx by two orders of magnitude (tests/test_oracle_envelope_cpu.py)."""
    ln = _ln(D)
    x, dy, _, _ = _data(33, D, torch.float32, False, seed=7, mean=50.0, std=0.1)
    _run_and_compare(ln, x, dy, tag=f"ln-largemean D={D} fp32 N=33")
