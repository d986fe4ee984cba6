"""The binding's argument checks (csrc/binding.cpp f32_ptr / u8_ptr / bn_side / residual_ptr): a tensor whose
raw pointer goes to a launcher is rejected when its length, dtype or contiguity is not what the kernel reads.

Every bad argument here stays in bounds even if its check were missing, so a missed check is a failed
assertion, never a bad device access: twice the required elements, a strided view (``buf[::2]``) of a buffer
twice as long (right numel, not contiguous), or a dtype of equal or larger element size (int8 for uint8,
float64 for fp32, fp32 for bf16). After the rejected calls the valid call runs once more and must repeat its
first result bit for bit: a rejected call launched nothing (the BatchNorm arrival counters included).
Tiny tensors: N = 2, C = 64, H = W = 4, so M = 32.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, C, H, W = 2, 64, 4, 4
M = N * H * W
EPS = 1e-5


def _native():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _nhwc(*shape):
    return torch.randn(*shape, device=DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def _longer(t):
    return torch.cat([t.reshape(-1), t.reshape(-1)])


def _strided(t):
    buf = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    view = buf[::2]
    view.copy_(t.reshape(-1))
    assert view.numel() == t.numel() and not view.is_contiguous()
    return view


def _wider(t):
    return t.to({torch.uint8: torch.int8, torch.float32: torch.float64, torch.bfloat16: torch.float32}[t.dtype])


def _same(a, b):
    if torch.is_tensor(a):
        assert torch.equal(a, b)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert a is None and b is None


def _check(call, good, bad):
    """call(*good) succeeds; with argument i replaced by each bad value it raises a RuntimeError naming the
    argument; then call(*good) repeats its first result exactly. call returns everything the op wrote."""
    first = call(*good)
    torch.cuda.synchronize()
    for i, name, values in bad:
        for v in values:
            args = list(good)
            args[i] = v
            with pytest.raises(RuntimeError, match=rf"\b{re.escape(name)}\b"):
                call(*args)
    again = call(*good)
    torch.cuda.synchronize()
    _same(first, again)


def _all_bad(t):
    return [_longer(t), _strided(t), _wider(t)]


@pytest.fixture(scope="module")
def bn():
    """One BatchNorm(+ReLU) forward: its input, outputs and saved statistics, shared and left unchanged."""
    torch.manual_seed(0)
    x = _nhwc(N, C, H, W)
    w = torch.rand(C, device=DEV) + 0.5
    b = torch.randn(C, device=DEV)
    y, mask, mean, invstd = _native().bn_fwd_train(x, None, w, b, None, None, 0.1, EPS, True)
    return dict(x=x, w=w, b=b, y=y, mask=mask, mean=mean, invstd=invstd, dy=_nhwc(N, C, H, W))


def test_bn_bwd_train(bn):
    good = [bn["dy"], bn["x"], bn["mask"], bn["w"], bn["mean"], bn["invstd"], True, True, True]
    _check(_native().bn_bwd_train, good,
           [(4, "mean", _all_bad(bn["mean"])), (5, "invstd", _all_bad(bn["invstd"])),
            (2, "mask", _all_bad(bn["mask"]))])


def test_bn_bwd_coef(bn):
    good = [bn["dy"], bn["x"], None, bn["mask"], bn["w"], bn["mean"], bn["invstd"], True, True]
    _check(_native().bn_bwd_coef, good,
           [(5, "mean", _all_bad(bn["mean"])), (3, "mask", _all_bad(bn["mask"]))])


def test_bn_fwd_train(bn):
    rm0, rv0 = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()

    def call(x, res, w, b, rm_, rv_):
        rm.copy_(rm0)  # updated in place: every call starts from the same running statistics
        rv.copy_(rv0)
        out = _native().bn_fwd_train(x, res, w, b, rm_, rv_, 0.1, EPS, True)
        return out, rm.clone(), rv.clone()

    good = [bn["x"], None, bn["w"], bn["b"], rm, rv]
    _check(call, good, [(4, "running_mean", _all_bad(rm0)), (2, "weight", _all_bad(bn["w"]))])


def test_bn_fwd_eval(bn):
    rm, rv = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    res = _nhwc(N, C, H, W)
    good = [bn["x"], res, bn["w"], bn["b"], rm, rv, EPS, True]
    _check(_native().bn_fwd_eval, good,
           [(5, "running_var", _all_bad(rv)),
            # twice the elements; fp32 in x's shape and strides; x's shape but not channels_last
            (1, "residual", [_nhwc(N, C, H, 2 * W), _wider(res), res.contiguous()])])


def test_maxpool3s2_bwd(bn):
    _, code, _, _ = _native().bn_relu_maxpool_fwd(bn["x"], bn["w"], bn["b"], None, None, 0.1, EPS)
    dy = _nhwc(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert code.numel() == dy.numel()
    _check(_native().maxpool3s2_bwd, [dy, code, H, W], [(1, "code", _all_bad(code))])


def test_gap_bwd(bn):
    g = torch.randn(N, C, device=DEV).to(torch.bfloat16)

    def call(g, bn_x, bn_mask, bn_mean):
        out = _native().gap_bwd(g, H, W, bn_x=bn_x, bn_mask=bn_mask, bn_mean=bn_mean)
        assert len(out) == 2  # the reduction applies to C = 64: the BatchNorm arguments are read
        return out

    _check(call, [g, bn["x"], bn["mask"], bn["mean"]],
           [(3, "bn_mean", _all_bad(bn["mean"])), (2, "bn_mask", _all_bad(bn["mask"]))])


def test_conv1x1_gemm(bn):
    K = 64
    a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    b = torch.randn(C, K, device=DEV).to(torch.bfloat16)
    bn_x = bn["x"].permute(0, 2, 3, 1).reshape(M, C)  # the channels_last storage as [M, C]
    assert bn_x.is_contiguous()

    def call(bn_x, bn_mask, bn_mean):
        out = torch.zeros(M, C, device=DEV, dtype=torch.bfloat16)
        part = _native().conv1x1_gemm(a, b, out, False, False, bn_x=bn_x, bn_mask=bn_mask, bn_mean=bn_mean)
        return out, part

    _check(call, [bn_x, bn["mask"], bn["mean"]],
           [(2, "bn_mean", _all_bad(bn["mean"])), (1, "bn_mask", _all_bad(bn["mask"]))])

    coef = torch.stack([torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV)])

    def call_coef(a_coef):
        out = torch.zeros(M, C, device=DEV, dtype=torch.bfloat16)
        assert _native().conv1x1_gemm(a, b, out, False, False, a_coef=a_coef) is None
        return out

    _check(call_coef, [coef], [(0, "a_coef", [_longer(coef), _strided(coef), _wider(coef)])])


def test_conv3x3s2_dgrad(bn):
    Co = 64
    dy = _nhwc(N, Co, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    wf = _native().conv3x3_flip(_nhwc(Co, C, 3, 3))

    def call(bn_mask):
        out = _native().conv3x3s2_dgrad(dy, wf, H, W, bn_x=bn["x"], bn_mask=bn_mask, bn_mean=bn["mean"])
        assert len(out) == 2  # the kernel takes the shape: {dx, partials}
        return out

    _check(call, [bn["mask"]], [(0, "bn_mask", _all_bad(bn["mask"]))])
