"""Counter-generated dropout on the MI355X: the kernels apply exactly the CPU reference mask
(csrc/philox.h, ops/dropout.py), fused and unfused forms agree bit for bit, the models reproduce,
and a captured step draws fresh masks on every replay."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 5


def _D():
    from pytorch_distributed_training_example_amd.ops import dropout
    return dropout


def _ticket(step, seed=SEED, device=DEV):
    st = _D().DropoutState(seed)
    st.set_state(seed, step)
    return st.begin_forward(device)


@functools.lru_cache(maxsize=None)
def _ref_mask(step, stream, shape, p, kind):
    """Shared CPU reference masks (computed once per distinct argument set, never modified)."""
    return _D().reference_mask(SEED, step, stream, shape, p, kind)


# ------------------------------------------------------------------ 8. mask identity
@pytest.mark.parametrize("step,stream", [(0, 0), (123456789, 7)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("kind,shape", [("flat", (4099,)), ("flat", (37, 768)), ("attn", (2, 3, 64, 64)),
                                        ("attn", (1, 2, 200, 200))])
def test_gpu_mask_equals_reference(kind, shape, p, step, stream):
    D = _D()
    t = _ticket(step)
    assert t.tensor.tolist() == [SEED, step]
    got = D.dropout_mask(t, stream, shape, p, kind)
    assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == shape
    assert torch.equal(got.cpu(), _ref_mask(step, stream, shape, p, kind))


def test_begin_forward_advances_on_device():
    D = _D()
    st = D.DropoutState(9)
    st.set_state(9, 40)
    a, b = st.begin_forward(DEV), st.begin_forward(DEV)
    assert a.tensor.tolist() == [9, 40] and b.tensor.tolist() == [9, 41]
    assert a.tensor.data_ptr() != b.tensor.data_ptr()  # two forwards before a backward keep their own
    assert st.get_state() == {"seed": 9, "step": 42}
    assert (a.next_stream(), a.next_stream(), b.next_stream()) == (0, 1, 0)


# ------------------------------------------------------------------ 9. elementwise op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_elementwise_dropout_bitwise(dtype, p):
    D = _D()
    torch.manual_seed(0)
    x = torch.randn(37, 768, device=DEV).to(dtype).requires_grad_()
    dy = torch.randn(37, 768, device=DEV).to(dtype)
    y = D.dropout(x, p, _ticket(3), stream=2)
    (dx,) = torch.autograd.grad(y, x, dy)
    m = _ref_mask(3, 2, (37, 768), p, "flat").to(DEV)
    scale = D.scale_of(D.threshold(p))
    zero = torch.zeros((), dtype=dtype, device=DEV)
    assert torch.equal(y, torch.where(m, (x.detach().float() * scale).to(dtype), zero))
    assert torch.equal(dx, torch.where(m, (dy.float() * scale).to(dtype), zero))


@pytest.mark.parametrize("n", [1, 15, 4099])
def test_elementwise_dropout_ragged_tail(n):
    D = _D()
    x = torch.randn(n, device=DEV)
    y = D.dropout(x, 0.5, _ticket(1), stream=0)
    m = _ref_mask(1, 0, (n,), 0.5, "flat").to(DEV)
    assert torch.equal(y, torch.where(m, x * 2.0, torch.zeros((), device=DEV)))


# ------------------------------------------------------------------ 10. fused add + LayerNorm
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("Dm", [256, 512, 768, 1024, 1280, 1536, 2048])
def test_fused_dropout_add_layernorm_bitwise(Dm, p, dtype):
    D = _D()
    from pytorch_distributed_training_example_amd.ops.layernorm import LayerNorm, add_layer_norm
    torch.manual_seed(Dm)
    N = 37
    ln = LayerNorm(Dm).to(DEV)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_()
    x0 = torch.randn(N, Dm, device=DEV).to(dtype)
    h0 = torch.randn(N, Dm, device=DEV).to(dtype)
    gs, gy = torch.randn(N, Dm, device=DEV).to(dtype), torch.randn(N, Dm, device=DEV).to(dtype)

    def run(fused):
        ln.zero_grad(set_to_none=True)
        x, h = x0.clone().requires_grad_(), h0.clone().requires_grad_()
        t = _ticket(17)
        if fused:
            s, y = add_layer_norm(x, h, ln, p, t, stream=3)
        else:
            s, y = add_layer_norm(x, D.dropout(h, p, t, stream=3), ln)
        torch.autograd.backward([s, y], [gs, gy])
        return s, y, x.grad, h.grad, ln.weight.grad.clone(), ln.bias.grad.clone()

    a, b = run(True), run(False)
    for name, u, v in zip(("s", "y", "dx", "dh", "dw", "db"), a, b):
        assert torch.equal(u, v), (name, (u.float() - v.float()).abs().max().item())
    # and the residual branch really was dropped with the reference mask
    m = _ref_mask(17, 3, (N, Dm), p, "flat").to(DEV)
    assert torch.equal(a[3] == 0, ~m | (a[2] == 0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_add_layernorm_p0_with_ticket_is_todays_path(dtype):
    from pytorch_distributed_training_example_amd.ops.layernorm import LayerNorm, add_layer_norm
    torch.manual_seed(2)
    ln = LayerNorm(768).to(DEV)
    x = torch.randn(37, 768, device=DEV).to(dtype)
    h = torch.randn(37, 768, device=DEV).to(dtype)
    t = _ticket(0)
    s0, y0 = add_layer_norm(x, h, ln)
    s1, y1 = add_layer_norm(x, h, ln, 0.0, t)
    assert torch.equal(s0, s1) and torch.equal(y0, y1)
    assert t.next_stream() == 0  # p = 0 consumed no stream id


# ------------------------------------------------------------------ 11. attention applies the reference mask
def _onehot_qkv(B, T, H):
    """Q = K = 0 (uniform P over the allowed keys), V[k, :] = onehot(k mod 64)."""
    qkv = torch.zeros(B, T, 3, H, 64, device=DEV)
    k = torch.arange(T, device=DEV)
    qkv[:, k, 2, :, k % 64] = 1.0
    return qkv.view(B, T, 3 * H * 64).bfloat16()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,T,causal", [(1, 2, 64, False), (2, 3, 200, False), (1, 2, 257, True)])
def test_attention_forward_applies_reference_mask(B, H, T, causal, p):
    D = _D()
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    pe = D.effective_p(p)
    out = attention_qkv(_onehot_qkv(B, T, H), H, causal=causal, dropout_p=p, ticket=_ticket(11), stream=1)
    keep = _ref_mask(11, 1, (B, H, T, T), p, "attn").to(DEV)
    allowed = torch.ones(T, T, dtype=torch.bool, device=DEV)
    if causal:
        allowed = allowed.tril()
    onehot = torch.nn.functional.one_hot(torch.arange(T, device=DEV) % 64, 64).float()  # [k, d]
    want = (keep & allowed).float() @ onehot  # [B, H, q, d]: kept keys k = d (mod 64)
    n_allowed = allowed.sum(-1).float()  # [q]
    got = out.float().view(B, T, H, 64).permute(0, 2, 1, 3) * n_allowed[None, None, :, None] * (1 - pe)
    assert want.max() <= 5
    assert torch.equal(got.round(), want), (got - want).abs().max().item()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,T", [(1, 2, 64), (2, 3, 200)])
def test_attention_dkdv_applies_reference_mask(B, H, T, p):
    """dO[q, :] = onehot(q mod 64), P = 1 / T everywhere: dV[k, d] T (1 - p_eff) counts the kept queries
    q = d (mod 64) of key k — the dK/dV kernel's own lane layout against the same reference."""
    D = _D()
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    pe = D.effective_p(p)
    qkv = _onehot_qkv(B, T, H).requires_grad_()
    out = attention_qkv(qkv, H, causal=False, dropout_p=p, ticket=_ticket(12), stream=0)
    q = torch.arange(T, device=DEV)
    do = torch.zeros(B, T, H, 64, device=DEV)
    do[:, q, :, q % 64] = 1.0
    out.backward(do.view(B, T, H * 64).bfloat16())
    keep = _ref_mask(12, 0, (B, H, T, T), p, "attn").to(DEV)
    onehot = torch.nn.functional.one_hot(q % 64, 64).float()  # [q, d]
    want = keep.float().transpose(-1, -2) @ onehot  # [B, H, k, d]
    dv = qkv.grad.float().view(B, T, 3, H, 64)[:, :, 2].permute(0, 2, 1, 3)  # [B, H, k, d]
    got = dv * T * (1 - pe)
    assert want.max() <= 4
    assert torch.equal(got.round(), want), (got - want).abs().max().item()


# ------------------------------------------------------------------ 12. attention numerics
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,T,H,causal", [(2, 197, 3, False), (2, 256, 2, True), (1, 100, 4, True)])
def test_flash_attention_dropout_numerics(B, T, H, causal, p):
    """Inputs of tests/test_kernels_gpu.py::test_flash_attention_qkv; oracle fp32 softmax(S) m scale @ V and
    its autograd gradients. Tolerance: that test's 2e-2 (3e-2 per gradient slice) over (1 - p_eff) — the
    only new error is bf16 P scaled by 1 / (1 - p_eff)."""
    D = _D()
    from pytorch_distributed_training_example_amd.ops.attention import _views, attention_qkv, attention_reference
    torch.manual_seed(0)
    Dh, pe = 64, D.effective_p(p)
    tol = 2e-2 / (1 - pe)
    qkv = (torch.randn(B, T, 3 * H * Dh, device=DEV) * 1.5).bfloat16().requires_grad_(True)
    y = attention_qkv(qkv, H, causal=causal, dropout_p=p, ticket=_ticket(31), stream=5)
    keep = _ref_mask(31, 5, (B, H, T, T), p, "attn").to(DEV)
    ref_in = qkv.detach().float().requires_grad_(True)
    (q, k, v), _ = _views(ref_in, H)
    yr = attention_reference(q, k, v, causal, keep=keep, keep_scale=1 / (1 - pe)).transpose(1, 2).reshape(B, T, H * Dh)
    torch.testing.assert_close(y.float(), yr, rtol=tol, atol=tol)
    g = torch.randn_like(yr)
    y.backward(g.bfloat16())
    yr.backward(g.bfloat16().float())
    err = (qkv.grad.float() - ref_in.grad).norm() / ref_in.grad.norm()
    print(f"dropout attention p={p} B={B} T={T} H={H} causal={causal}: grad rel err {err.item():.4g} (tol {tol:.4g})")
    assert err < tol, err
    for i in range(3):  # dq / dk / dv
        a = qkv.grad.float().view(B, T, 3, H, Dh)[:, :, i]
        b = ref_in.grad.view(B, T, 3, H, Dh)[:, :, i]
        e = ((a - b).norm() / (b.norm() + 1e-6)).item()
        print(f"  slice {i}: {e:.4g}")
        assert e < 3e-2 / (1 - pe), (i, e)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_p0_with_ticket_is_todays_path(causal):
    from pytorch_distributed_training_example_amd.ops.attention import attention_qkv
    torch.manual_seed(1)
    qkv = (torch.randn(2, 197, 3 * 3 * 64, device=DEV) * 1.5).bfloat16()
    g = torch.randn(2, 197, 3 * 64, device=DEV).bfloat16()
    res = []
    for t in (None, _ticket(0)):
        x = qkv.clone().requires_grad_()
        y = attention_qkv(x, 3, causal=causal, dropout_p=0.0, ticket=t)
        y.backward(g)
        res.append((y, x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ------------------------------------------------------------------ 13. models
def _tiny(name, dropout):
    from pytorch_distributed_training_example_amd.models import get_model
    torch.manual_seed(0)
    m = get_model(name, dropout=dropout) if dropout is not None else get_model(name)
    if name == "vit_tiny":
        with torch.no_grad():
            m.heads.head.weight.normal_(0, 0.02)  # zero-initialised: the logits would not depend on the encoder
    return m


def _batch(name, device):
    g = torch.Generator().manual_seed(7)
    if name == "gpt2_tiny":
        x, y = torch.randint(0, 512, (4, 64), generator=g), torch.randint(0, 512, (4, 64), generator=g)
    else:
        x, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 1000, (8,), generator=g)
    return x.to(device), y.to(device)


def _loss(name, model, batch):
    from pytorch_distributed_training_example_amd.ops.cross_entropy import cross_entropy
    x, y = batch
    if x.is_floating_point() and next(model.parameters()).dtype == torch.bfloat16:
        x = x.bfloat16()
    if name == "gpt2_tiny":
        return model(x, y)
    return cross_entropy(model(x), y)


@pytest.mark.parametrize("name", ["gpt2_tiny", "vit_tiny"])
def test_tiny_models_with_dropout_gpu(name):
    D = _D()
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    base = _tiny(name, 0.1)
    m = to_bf16_mixed(copy.deepcopy(base).cuda())
    batch = _batch(name, DEV)
    D.set_state(SEED, 0)
    a = _loss(name, m, batch)
    b = _loss(name, m, batch)
    assert a.item() != b.item()
    D.set_state(SEED, 0)
    a2 = _loss(name, m, batch)
    assert torch.equal(a2, a)
    a2.backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    # same weights, same (seed, step) on the CPU path in fp32: the masks are the same, only arithmetic differs
    D.set_state(SEED, 0)
    l32 = _loss(name, base, _batch(name, "cpu")).item()
    print(f"{name}: GPU bf16 loss {a.item():.6f}, CPU fp32 loss {l32:.6f}")
    assert abs(a.item() - l32) <= 0.02 * max(1.0, abs(l32)), (a.item(), l32)
    # eval: exactly the model built without the argument
    m0 = to_bf16_mixed(copy.deepcopy(_tiny(name, None)).cuda())
    m0.load_state_dict(m.state_dict())
    m.eval(), m0.eval()
    before = D.get_state()
    with torch.no_grad():
        assert torch.equal(_loss(name, m, batch), _loss(name, m0, batch))
    assert D.get_state() == before


@pytest.mark.parametrize("name", ["gpt2_tiny", "vit_tiny"])
def test_tiny_models_aten_dropout_switch(name, switch):
    """PDT_DROPOUT_FUSED=0: the same sites from F.dropout / SDPA (other masks: only finiteness is checked)."""
    D = _D()
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    switch("PDT_DROPOUT_FUSED", "0")
    m = to_bf16_mixed(_tiny(name, 0.1).cuda())
    before = D.get_state()
    loss = _loss(name, m, _batch(name, DEV))
    loss.backward()
    assert torch.isfinite(loss).item()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert D.get_state() == before  # no ticket, no counter


def test_unfused_block_path_draws_the_same_masks(switch):
    """PDT_FUSED_ADDLN=0 (Block.forward, elementwise dropout op) == run_blocks' fused kernels, bit for bit."""
    D = _D()
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    m = to_bf16_mixed(_tiny("gpt2_tiny", 0.1).cuda())
    batch = _batch("gpt2_tiny", DEV)
    D.set_state(SEED, 3)
    fused = _loss("gpt2_tiny", m, batch)
    switch("PDT_FUSED_ADDLN", "0")
    D.set_state(SEED, 3)
    assert torch.equal(_loss("gpt2_tiny", m, batch), fused)


# ------------------------------------------------------------------ 14. fp8
def test_fp8_blocks_with_dropout_run():
    D = _D()
    from pytorch_distributed_training_example_amd.models.transformer import Block, run_blocks
    from pytorch_distributed_training_example_amd.ops.fp8 import enable_fp8
    from pytorch_distributed_training_example_amd.ops.layernorm import LayerNorm
    torch.manual_seed(7)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = torch.nn.ModuleList([Block(512, 8, dropout=0.1) for _ in range(2)])
            self.ln_f = LayerNorm(512)

        def forward(self, x):
            return run_blocks(self.blocks, x, self.ln_f, D.begin_forward(x.device))
    net = Net().cuda()
    for mod in net.modules():  # bf16 weights, fp32 LayerNorm parameters (models/precision.py)
        if isinstance(mod, torch.nn.Linear):
            mod.to(torch.bfloat16)
    enable_fp8(net, history=4)
    x0 = torch.randn(16, 64, 512, device=DEV).bfloat16()
    g = torch.randn(16, 64, 512, device=DEV).bfloat16()
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = net(x)
        y.backward(g)
    assert torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in net.parameters())


# ------------------------------------------------------------------ 15. captured step
def test_captured_step_draws_fresh_masks_and_matches_eager():
    D = _D()
    from pytorch_distributed_training_example_amd.engine.graph import StaticStep
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.optim import FusedSGD
    base = to_bf16_mixed(_tiny("gpt2_tiny", 0.1).cuda())
    x, y = _batch("gpt2_tiny", DEV)

    def run(mode):
        m = copy.deepcopy(base)
        opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9)

        def step(xi, yi):
            opt.zero_grad(set_to_none=True)
            loss = m(xi, yi)
            loss.backward()
            opt.step()
            return loss.detach()

        D.set_state(SEED, 0)
        if mode == "eager":
            for _ in range(3):
                step(x, y)
            D.set_state(SEED, 100)
            out = [float(step(x, y)) for _ in range(3)]
        else:
            runner = StaticStep(step, [x, y], warmup=3)
            runner.capture()
            D.set_state(SEED, 100)
            out = [float(runner(x, y)) for _ in range(3)]
        assert D.get_state() == {"seed": SEED, "step": 103}
        return out

    le, lg = run("eager"), run("graph")
    assert len(set(lg)) == 3, lg  # every replay advanced the step: fresh masks
    assert lg == le, (lg, le)
