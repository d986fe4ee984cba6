"""FusedLARS / FusedLAMB on the gfx950 kernels (csrc/kernels/layerwise.hip): the norm pass and the trust
ratios against float64, the 36-tensor batch boundary, the update against the float64 contract, bf16 with
master weights, AMP scale and skip, run-to-run determinism, hipGraph capture, and two small models."""
import copy
import functools

import numpy as np
import pytest
import torch

from layerwise_oracle import SHAPES, TOL, lamb_oracle, lars_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 16384  # PDT_MT_CHUNK
MAX_TENSORS = 36  # PDT_MT_MAX_TENSORS
U = 2.0 ** -24  # fp32 unit roundoff
# A tensor's sum of squares: each of the 256 threads of a chunk adds its CHUNK / 256 = 64 squares one after the
# other, the wave and block tree adds 6 + 4 more levels, each square is rounded once, the partials are rounded
# to fp32 once; the finalize is in double. (64 + 12) roundings of relative size U, twice that for slack.
SUMSQ_BOUND = 2 * (CHUNK // 256 + 12) * U

LARS_KW = dict(lr=10.0, momentum=0.9, weight_decay=1e-4)  # lr 10: trust ratios are ~1e-3
LAMB_KW = dict(lr=1e-2, weight_decay=0.01)


def _native():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _optim():
    from pytorch_distributed_training_example_amd import optim
    return optim


def _cls(name):
    return _optim().FusedLARS if name == "lars" else _optim().FusedLAMB


def _kw(name):
    return dict(LARS_KW if name == "lars" else LAMB_KW)


def _oracle(name):
    return lars_oracle if name == "lars" else lamb_oracle


def _scratch(kparams):
    from pytorch_distributed_training_example_amd.optim.fused import _LayerwiseScratch
    return _LayerwiseScratch(kparams)


@functools.lru_cache(maxsize=None)
def _inputs(steps=3):
    """fp32 weights and gradients of the optimizer shape set, on the CPU (never modified)."""
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(steps)]
    return ws, grads


def _params(ws, dtype=torch.float32, channels_last=False):
    ps = []
    for w in ws:
        w = w.to(DEV)
        if channels_last and w.dim() == 4:
            w = w.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(w.to(dtype)))
    return ps


def _set_grads(ps, gs, dtype=None, scale=1.0):
    for p, g in zip(ps, gs):
        g = (g.to(DEV) * scale).to(dtype or p.dtype)
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
            g = g.contiguous(memory_format=torch.channels_last)
        if g.dtype != p.dtype and hasattr(p, "grad_dtype"):
            p.grad_dtype = g.dtype  # newer torch: a gradient of another dtype (a bf16 bucket view) is opt-in
        p.grad = g


def _state(opt, ps):
    keys = ("momentum_buffer", "exp_avg", "exp_avg_sq", "step", "master_param")
    return [opt.state[p][k].detach().clone() for p in ps for k in keys if k in opt.state[p]]


def _run(name, ps, grads, grad_dtype=None, **over):
    opt = _cls(name)(ps, **{**_kw(name), **over})
    for gs in grads:
        _set_grads(ps, gs, grad_dtype)
        opt.step()
    torch.cuda.synchronize()
    return opt


# ----------------------------------------------------------------------------- norm pass, finalize
def _norm_tensors(dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = [torch.randn(n, device=DEV, generator=g).to(dtype) for n in (1, 3, 16383, 16384, 16385, 70001)]
    out.append(torch.randn(1000, 2048, device=DEV, generator=g).to(dtype))
    out.append(torch.randn(5004, device=DEV, generator=g).to(dtype)[1:])  # starts 1 element into its storage
    assert out[-1].data_ptr() % 16 != 0  # the scalar path
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lars_norm_pass_and_ratio(dtype):
    ws, gs = _norm_tensors(dtype, 1), _norm_tensors(dtype, 2)
    before = [w.clone() for w in ws]
    sc = _scratch(ws)
    sc.partials.fill_(float("nan"))  # every slot in use is written: no zero-fill is needed
    tc, wd, eps = 0.02, 1e-4, 1e-8
    _native().lars(ws, gs, [], [], 0.1, None, 0.9, 0.0, wd, False, False, tc, eps, False, None, None,
                   sc.partials, sc.sums, sc.ratio, True)
    torch.cuda.synchronize()
    tc, wd, eps = (float(np.float32(v)) for v in (tc, wd, eps))  # the kernel's hyper-parameters are fp32
    for i, (w, g) in enumerate(zip(ws, gs)):
        assert torch.equal(w, before[i])  # norms_only: no update
        a, b = float(w.double().pow(2).sum()), float(g.double().pow(2).sum())
        ka, kb = float(sc.sums[i, 0]), float(sc.sums[i, 1])
        print(f"lars {dtype} tensor {i} numel {w.numel()}: rel err w {abs(ka - a) / a:.3e} g {abs(kb - b) / b:.3e} "
              f"(bound {SUMSQ_BOUND:.3e})")
        assert abs(ka - a) <= SUMSQ_BOUND * a and abs(kb - b) <= SUMSQ_BOUND * b
        r = tc * ka ** 0.5 / (kb ** 0.5 + wd * ka ** 0.5 + eps)  # the formula on the kernel's own sums
        assert abs(float(sc.ratio[i]) - r) <= 2 * U * r  # one rounding to fp32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lamb_norm_pass_and_ratio(dtype):
    """First step from m = v = 0 with hyper-parameters that are exact in fp32 and no decay, so that u has a
    closed form with no cancellation: m = (1 - b1) g, v = (1 - b2) g^2, u = (m / (1 - b1)) / (sqrt(v / (1 - b2)) + eps)."""
    ws, gs = _norm_tensors(dtype, 3), _norm_tensors(dtype, 4)
    ms = [torch.zeros(w.shape, device=DEV) for w in ws]
    vs = [torch.zeros(w.shape, device=DEV) for w in ws]
    sc = _scratch(ws)
    sc.partials.fill_(float("nan"))
    b1, b2, eps = 0.5, 0.75, 2.0 ** -20
    step = torch.ones(1, device=DEV)
    _native().lamb(ws, gs, ms, vs, [], 0.1, None, b1, b2, eps, 0.0, step, 0.0, False, None, None,
                   sc.partials, sc.sums, sc.ratio, True)
    torch.cuda.synchronize()
    # u from fp32 inputs: one rounding in m, two in v, then m / bc1, v / bc2, sqrt (halves what v carries), + eps
    # and the quotient: at most 8 roundings in u, 16 U in u^2 on top of the reduction
    u_bound = SUMSQ_BOUND + 16 * U
    for i, (w, g) in enumerate(zip(ws, gs)):
        g64 = g.double()
        m64, v64 = (1 - b1) * g64, (1 - b2) * g64 * g64
        torch.testing.assert_close(ms[i].double(), m64, rtol=4 * U, atol=0)
        torch.testing.assert_close(vs[i].double(), v64, rtol=4 * U, atol=1e-30)
        u64 = (m64 / (1 - b1)) / ((v64 / (1 - b2)).sqrt() + eps)
        a, b = float(w.double().pow(2).sum()), float(u64.pow(2).sum())
        ka, kb = float(sc.sums[i, 0]), float(sc.sums[i, 1])
        print(f"lamb {dtype} tensor {i} numel {w.numel()}: rel err w {abs(ka - a) / a:.3e} u {abs(kb - b) / b:.3e} "
              f"(bounds {SUMSQ_BOUND:.3e}, {u_bound:.3e})")
        assert abs(ka - a) <= SUMSQ_BOUND * a and abs(kb - b) <= u_bound * b
        r = (ka / kb) ** 0.5
        assert abs(float(sc.ratio[i]) - r) <= 2 * U * r


def test_zero_norms_and_empty_tensor():
    ws = [torch.zeros(100, device=DEV), torch.randn(100, device=DEV)]
    gs = [torch.randn(100, device=DEV), torch.zeros(100, device=DEV)]
    sc = _scratch(ws)
    _native().lars(ws, gs, [], [], 0.1, None, 0.0, 0.0, 0.0, False, False, 0.001, 1e-8, False, None, None,
                   sc.partials, sc.sums, sc.ratio, True)
    assert sc.ratio.tolist() == [1.0, 1.0]
    for name in ("lars", "lamb"):
        ps = [torch.nn.Parameter(w.clone()) for w in ws] + [torch.nn.Parameter(torch.zeros(0, 4, device=DEV))]
        opt = _cls(name)(ps, **_kw(name))
        _set_grads(ps, gs + [torch.zeros(0, 4)])
        opt.step()  # the empty parameter is left out, the others step with r = 1
        assert all(torch.isfinite(p).all() for p in ps)
        assert [float(r) for r in opt.trust_ratios().values()][:1] == [1.0]
    with pytest.raises(RuntimeError, match="zero-element"):
        e = [torch.zeros(0, device=DEV)]
        _native().lars(e, e, [], [], 0.1, None, 0.0, 0.0, 0.0, False, False, 0.001, 1e-8, False, None, None,
                       None, None, None, False)


# ----------------------------------------------------------------------------- batch boundary
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_batch_boundary(name):
    """40 tensors = one full batch of 36 and a second of 4; tensor 3 has three chunks, so partial slots and
    tensor indices differ from there on. The last tensor of the first batch and the first of the second must
    come out exactly as when stepped alone."""
    g = torch.Generator().manual_seed(5)
    sizes = [100 + 7 * i for i in range(40)]
    sizes[3] = 2 * CHUNK + 5
    sizes[MAX_TENSORS] = CHUNK + 1
    ws = [torch.randn(n, generator=g) for n in sizes]
    gs = [torch.randn(n, generator=g) for n in sizes]
    ps = _params(ws)
    opt = _run(name, ps, [gs])
    ratios = opt.trust_ratios()
    for i in (MAX_TENSORS - 1, MAX_TENSORS, 39, 3):
        alone = _params([ws[i]])
        o1 = _run(name, alone, [[gs[i]]])
        r_all, r_one = float(ratios[ps[i]]), float(o1.trust_ratios()[alone[0]])
        assert r_all == r_one and 0 < r_one < 1e3 and r_one != 1.0, (i, r_all, r_one)
        assert torch.equal(ps[i].detach(), alone[0].detach()), i
        assert not torch.equal(ps[i].detach().cpu(), ws[i])


# ----------------------------------------------------------------------------- update vs the fp64 contract
@functools.lru_cache(maxsize=None)
def _reference(name, bf16_grads):
    ws, grads = _inputs()
    if bf16_grads:
        grads = [[g.bfloat16().float() for g in gs] for gs in grads]
    return _oracle(name)(ws, grads, **_kw(name))[0]


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_update_matches_fp64_contract(name, grad_dtype):
    ws, grads = _inputs()
    ps = _params(ws, channels_last=True)
    _run(name, ps, grads, grad_dtype)
    for p, r, w in zip(ps, _reference(name, grad_dtype == torch.bfloat16), ws):
        torch.testing.assert_close(p.detach().cpu(), r.float(), **TOL)
        assert (p.detach().cpu() - w).abs().max() > 1e-3  # and the steps were not negligible


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_nesterov_and_plain_groups(name):
    """LARS with nesterov, and both optimizers with an adapt=False group next to an adapted one."""
    ws, grads = _inputs()
    kw = dict(nesterov=True) if name == "lars" else {}
    ps = _params(ws)
    two, one = [p for p in ps if p.dim() >= 2], [p for p in ps if p.dim() < 2]
    groups = [dict(params=two), dict(params=one, adapt=False, weight_decay=0.0, lr=0.1 if name == "lars" else 1e-2)]
    opt = _cls(name)(groups, **{**_kw(name), **kw})
    for gs in grads:
        _set_grads(ps, gs)
        opt.step()
    okw = {**_kw(name), **kw}
    i2 = [i for i, p in enumerate(ps) if p.dim() >= 2]
    i1 = [i for i, p in enumerate(ps) if p.dim() < 2]
    ref2 = _oracle(name)([ws[i] for i in i2], [[gs[i] for i in i2] for gs in grads], **okw)[0]
    okw.update(adapt=False, weight_decay=0.0, lr=0.1 if name == "lars" else 1e-2)
    ref1 = _oracle(name)([ws[i] for i in i1], [[gs[i] for i in i1] for gs in grads], **okw)[0]
    for i, r in list(zip(i2, ref2)) + list(zip(i1, ref1)):
        torch.testing.assert_close(ps[i].detach().cpu(), r.float(), **TOL)


# ----------------------------------------------------------------------------- bf16 + master weights
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_bf16_master_weights(name):
    ws, grads = _inputs()
    ws = [w.bfloat16().float() for w in ws]
    grads = [[g.bfloat16().float() for g in gs] for gs in grads]
    ps = _params(ws, torch.bfloat16)
    opt = _run(name, ps, grads)
    ref = _params(ws)
    _run(name, ref, grads)
    for p, r in zip(ps, ref):
        m = opt.state[p]["master_param"]
        assert m.dtype == torch.float32
        assert torch.equal(p.detach(), m.to(torch.bfloat16))
        torch.testing.assert_close(m, r.detach(), rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_norms_come_from_the_master(name):
    """Scale one master copy by 1 + 2^-11: below bf16 resolution (2^-9 between neighbours), so the bf16
    parameter could not carry it. Without decay both ratios are proportional to ||w||, so the ratio must
    move by that factor."""
    ws, grads = _inputs()
    ws, grads = [ws[2].bfloat16().float()], [[gs[2].bfloat16().float()] for gs in grads]
    out = []
    for scale in (1.0, 1.0 + 2.0 ** -11):
        ps = _params(ws, torch.bfloat16)
        opt = _cls(name)(ps, **{**_kw(name), "weight_decay": 0.0, "lr": 0.0})
        _set_grads(ps, grads[0])
        opt.step()  # lr 0: creates the master copy and the states, moves nothing
        opt.state[ps[0]]["master_param"].mul_(scale)
        _set_grads(ps, grads[1])
        opt.step()
        out.append(float(opt.trust_ratios()[ps[0]]))
    rel = out[1] / out[0] - 1.0
    assert out[0] != out[1] and abs(rel - 2.0 ** -11) < 0.1 * 2.0 ** -11, (out, rel)


# ----------------------------------------------------------------------------- AMP
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_amp_power_of_two_scale_is_exact(name):
    ws, grads = _inputs(3)
    a = _params(ws)
    _run(name, a, grads[:2])
    b = _params(ws)
    opt = _cls(name)(b, **_kw(name))
    inv, found = torch.full((1,), 0.25, device=DEV), torch.zeros(1, device=DEV)
    for gs in grads[:2]:
        _set_grads(b, gs, scale=4.0)
        opt.step(inv_scale=inv, found_inf=found)
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_amp_found_inf_skips_everything(name):
    ws, grads = _inputs(3)
    ps = _params(ws)
    opt = _cls(name)(ps, **_kw(name))
    inv, found = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    _set_grads(ps, grads[0])
    opt.step(inv_scale=inv, found_inf=found)
    w0, s0 = [p.detach().clone() for p in ps], _state(opt, ps)
    assert s0
    _set_grads(ps, grads[1])
    ps[2].grad[3, 3] = float("inf")
    ps[4].grad[70000] = float("nan")
    found.fill_(1.0)
    opt.step(inv_scale=inv, found_inf=found)
    torch.cuda.synchronize()
    for x, y in zip(w0 + s0, [p.detach() for p in ps] + _state(opt, ps)):
        assert torch.equal(x, y)
    if name == "lamb":
        assert float(opt.state[ps[0]]["step"]) == 1.0
    # the run goes on as if the skipped step had not happened
    found.zero_()
    _set_grads(ps, grads[2])
    opt.step(inv_scale=inv, found_inf=found)
    ref = _params(ws)
    _run(name, ref, [grads[0], grads[2]])
    for x, y in zip(ps, ref):
        assert torch.isfinite(x).all() and torch.equal(x.detach(), y.detach())


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_two_runs_are_bit_equal(name):
    ws, grads = _inputs()
    runs = []
    for _ in range(2):
        ps = _params(ws, channels_last=True)
        opt = _run(name, ps, grads)
        runs.append([p.detach().clone() for p in ps] + _state(opt, ps) + list(opt.trust_ratios().values()))
    assert len(runs[0]) == len(runs[1]) > 2 * len(ws)
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- hipGraph capture
@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_captured_step_replays_like_eager(name):
    g = torch.Generator().manual_seed(11)
    shapes = [(48, 16, 3, 3), (48,), (300, 130), (CHUNK + 3,), (7,)]
    ws = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(6)]

    def make():
        ps = _params(ws)
        groups = [dict(params=[p for p in ps if p.dim() >= 2]),
                  dict(params=[p for p in ps if p.dim() < 2], adapt=False, weight_decay=0.0)]
        return ps, _cls(name)(groups, **{**_kw(name), "lr": 0.5 if name == "lars" else 1e-2})

    def eager(halve):
        ps, opt = make()
        for i, gs in enumerate(grads):
            if halve and i == 5:
                for grp in opt.param_groups:
                    grp["lr"] *= 0.5
            _set_grads(ps, gs)
            opt.step()
        torch.cuda.synchronize()
        return [p.detach().clone() for p in ps] + _state(opt, ps)

    ref, ref_same_lr = eager(True), eager(False)
    ps, opt = make()
    for p in ps:
        p.grad = torch.zeros_like(p)  # static gradient buffers
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for gs in grads[:3]:  # eager warm-up: states, scratch and device scalars exist before the capture
            for p, gg in zip(ps, gs):
                p.grad.copy_(gg)
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step()
    for i, gs in enumerate(grads[3:]):
        if i == 2:
            for grp in opt.param_groups:
                grp["lr"] *= 0.5
            opt.sync_lr()
        for p, gg in zip(ps, gs):
            p.grad.copy_(gg)
        graph.replay()
    torch.cuda.synchronize()
    got = [p.detach() for p in ps] + _state(opt, ps)
    assert len(got) == len(ref)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(got[:len(ps)], ref_same_lr[:len(ps)]))  # the new lr counted
    del graph


# ----------------------------------------------------------------------------- model level
def _train5(make_model, make_opt, batch, loss_fn):
    torch.manual_seed(0)
    model = make_model()
    opt = make_opt(model)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model, *batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in model.parameters()]


def _check_model(make_model, make_opt, batch, loss_fn):
    la, pa = _train5(make_model, make_opt, batch, loss_fn)
    lb, pb = _train5(make_model, make_opt, batch, loss_fn)
    print("losses", la)
    assert all(np.isfinite(la)) and la[4] < la[0], la
    assert la == lb
    bad = [i for i, (x, y) in enumerate(zip(pa, pb)) if not torch.equal(x, y)]
    assert not bad, f"{len(bad)} of {len(pa)} parameters differ between two runs (first: {bad[:5]})"


def test_resnet18_lars_trains_and_repeats():
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    from pytorch_distributed_training_example_amd.ops.cross_entropy import cross_entropy
    base = [None]

    def make_model():
        if base[0] is None:
            torch.manual_seed(0)
            base[0] = to_bf16_mixed(get_model("resnet18", num_classes=16).cuda().to(memory_format=torch.channels_last))
        return copy.deepcopy(base[0])

    def make_opt(m):
        o = _optim()
        return o.FusedLARS(o.layerwise_param_groups(m, 5e-5), lr=0.1, momentum=0.9, trust_coefficient=0.1)

    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(8, 3, 32, 32, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 16, (8,), device=DEV, generator=g)
    _check_model(make_model, make_opt, (x, y), lambda m, x, y: cross_entropy(m(x), y))


def test_gpt2_lamb_trains_and_repeats():
    from pytorch_distributed_training_example_amd.models.gpt2 import GPT, GPTConfig
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    base = [None]

    def make_model():
        if base[0] is None:
            torch.manual_seed(0)
            base[0] = to_bf16_mixed(GPT(GPTConfig(n_layer=2, n_head=2, n_embd=128, block_size=64, vocab_size=512)).cuda())
        return copy.deepcopy(base[0])

    def make_opt(m):
        o = _optim()
        return o.FusedLAMB(o.layerwise_param_groups(m, 0.01), lr=1e-2)

    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randint(0, 512, (4, 64), device=DEV, generator=g)
    y = torch.randint(0, 512, (4, 64), device=DEV, generator=g)
    _check_model(make_model, make_opt, (x, y), lambda m, x, y: m(x, y))


# ----------------------------------------------------------------------------- the training step around them
def _amp_step(name, clip):
    from pytorch_distributed_training_example_amd.engine.amp import GradScaler
    from pytorch_distributed_training_example_amd.engine.trainer import StepConfig, TrainStep, make_loss_fn
    from pytorch_distributed_training_example_amd.models import get_model
    torch.manual_seed(0)
    m = get_model("vit_tiny", image_size=32, num_classes=10).cuda()
    torch.nn.init.normal_(m.heads.head.weight, std=0.02)
    sc = GradScaler(init_scale=2.0 ** 12, growth_interval=2, device="cuda")
    o = _optim()
    groups = o.layerwise_param_groups(m, 1e-4)
    opt = (o.FusedLARS(groups, lr=0.1, momentum=0.9, trust_coefficient=0.02) if name == "lars"
           else o.FusedLAMB(groups, lr=1e-3))
    cfg = StepConfig(precision="amp_fp16", reducer="none", clip_grad=clip)
    return m, sc, opt, TrainStep(m, opt, make_loss_fn("cross_entropy"), cfg, scaler=sc, raw_model=m)


def _amp_batches(bad):
    g = torch.Generator(device="cuda").manual_seed(5)
    xs = [torch.randn(8, 3, 32, 32, device="cuda", generator=g) for _ in range(6)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(6)]
    xs[bad] = xs[bad] * 1e6  # overflows fp16 in the forward
    return xs, ys


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_amp_fp16_graph_captured_step(name):
    """--precision amp_fp16 --hipgraph: the whole step (autocast forward, scaled backward, unscale + inf check,
    the layer-wise optimizer with its on-device skip, scale update) captured once and replayed equals eager step
    for step, through an overflowing input that skips the update and backs the scale off on device."""
    bad = 2
    xs, ys = _amp_batches(bad)
    me, se, oe, te = _amp_step(name, 0.0)
    mg, sg, og, tg = _amp_step(name, 0.0)
    tg.enable_graph(warmup=2)
    for _ in range(2):  # StaticStep's two eager warm-up steps
        te(xs[0], ys[0])
    for i in range(len(xs)):
        before, scale = [p.detach().clone() for p in mg.parameters()], sg.get_scale()
        te(xs[i], ys[i])
        tg(xs[i], ys[i])
        assert se.get_scale() == sg.get_scale(), i
        worst = max((((a - b).abs() / (TOL["atol"] + TOL["rtol"] * b.abs())).max().item(), n)
                    for (n, a), b in zip(me.named_parameters(), mg.parameters()))
        print(f"{name} replay {i}: scale {sg.get_scale()}, worst eager-vs-graph difference {worst[0]:.3e} of the "
              f"tolerance ({worst[1]})")
        for a, b in zip(me.parameters(), mg.parameters()):
            torch.testing.assert_close(a, b, msg=lambda m: f"replay {i}: {m}", **TOL)
        moved = any(not torch.equal(a, b.detach()) for a, b in zip(before, mg.parameters()))
        skipped = sg.get_scale() < scale  # the scaler backs off exactly when the step found a non-finite gradient
        assert moved == (not skipped) and (skipped or i != bad), (i, moved, skipped)
    assert tg._graphs and all(r.graph is not None for r in tg._graphs.values())
    assert all(torch.isfinite(p).all() for p in mg.parameters())


@pytest.mark.parametrize("name", ["lars", "lamb"])
def test_amp_fp16_clip_graph_and_checkpoint(name, tmp_path):
    """... and with --clip-grad and --checkpoint / --resume. The clip norm still ends in float atomics (README,
    known leftover), fp16 autocast amplifies its last-bit differences from step to step, and both optimizers
    turn the rounding-noise gradient of ViT's key biases into full-size steps, so two clipped runs are not
    compared over several steps. Checked instead: the captured clipped step replays, clips, skips on overflow
    and stays finite; and a checkpoint restores model, optimizer and scaler so that ONE further step from the
    identical state agrees (one step differs by the last bit of the clip coefficient only)."""
    from pytorch_distributed_training_example_amd.engine.checkpoint import load_checkpoint, save_checkpoint
    bad = 2
    xs, ys = _amp_batches(bad)
    mg, sg, og, tg = _amp_step(name, 1.0)
    tg.enable_graph(warmup=2)
    for i in range(len(xs)):
        before, scale = [p.detach().clone() for p in mg.parameters()], sg.get_scale()
        tg(xs[i], ys[i])
        moved = any(not torch.equal(a, b.detach()) for a, b in zip(before, mg.parameters()))
        skipped = sg.get_scale() < scale
        assert moved == (not skipped) and (skipped or i != bad), (i, moved, skipped)
        if not skipped:  # the static gradient buffers hold the unscaled, clipped gradients of this replay
            norm = float(torch.sqrt(sum(p.grad.float().pow(2).sum() for p in mg.parameters() if p.grad is not None)))
            assert norm <= 1.0 + 1e-3, (i, norm)
    assert tg._graphs and all(r.graph is not None for r in tg._graphs.values())
    assert all(torch.isfinite(p).all() for p in mg.parameters())

    me, se, oe, te = _amp_step(name, 1.0)
    for i in (0, 1, 3):
        te(xs[i], ys[i])
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, me, oe, None, se, epoch=1)
    m2, s2, o2, t2 = _amp_step(name, 1.0)
    assert load_checkpoint(path, m2, o2, None, s2, map_location="cuda")["epoch"] == 1
    for a, b in zip(me.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    te(xs[4], ys[4])
    t2(xs[4], ys[4])
    assert se.get_scale() == s2.get_scale()
    for a, b in zip(me.parameters(), m2.parameters()):
        torch.testing.assert_close(a, b, **TOL)
