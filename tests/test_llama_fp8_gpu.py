"""fp8 for the Llama decoder on one MI355X: the fp8-emitting RMSNorm (rmsnorm.hip rms_fwd_fp8_kernel) and
SwiGLU casts (fp8.hip fp8_swiglu_cast_kernel) against their unfused chains (bf16 kernel, then
fp8_cast_transpose) bit for bit and against the float64 oracle's e4m3 envelope (tests/llama_fp8_oracle.py);
striped state rows; the fused model path against the per-Linear fp8 path; fp8 against bf16; training; a
captured step; the command line."""
import copy
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import llama_oracle as LO
from llama_fp8_oracle import fp8_worst_ratio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
V, B, T = 512, 4, 64


def _C():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _st(scale):
    st = torch.zeros(3 + 4, device="cuda")
    st[1], st[2] = scale, 1.0 / scale
    return st


def _u8(t):
    return t.view(torch.uint8)


# ----------------------------------------------------------------------------- 1. / 3. rms_fwd_fp8
RMS_SCALE = 80.0


def _rms_case(n, d, fused):
    x, _, h, _, w = LO.rms_inputs(n, d, BF16, fused=fused)
    x[1, 5] = 300.0  # this row's y reaches sqrt(D) |w| at that column: saturates at 448 after scaling
    return x, h, w


@pytest.mark.parametrize("n,d,fused", [(16, 256, True), (48, 512, True), (48, 1280, True), (48, 1536, True),
                                       (8208, 1024, True), (48, 768, False)])
def test_rms_fwd_fp8_bit_identical_to_rms_then_cast(n, d, fused):
    """add + RMSNorm emitting e4m3 (+ transpose) == the bf16 add + RMSNorm kernel followed by the cast-transpose
    pass: the same bytes, rstd, residual sum and amax; and every unsaturated element inside the float64
    oracle's e4m3 envelope, which does not rest on the bf16 kernel."""
    C = _C()
    x, h, w = _rms_case(n, d, fused)
    xg, wg, hg = x.cuda(), w.cuda(), (h.cuda() if fused else None)
    st_ref, st = _st(RMS_SCALE), _st(RMS_SCALE)
    y, rstd_r, s_r = C.rms_fwd(xg, wg, LO.EPS, hg)
    q_ref, qt_ref = C.fp8_cast_transpose(y, st_ref, True)
    q, qt, rstd, s = C.rms_fwd_fp8(xg, wg, LO.EPS, hg, st)
    assert q.shape == (n, d) and qt.shape == (d, n) and q.dtype == torch.float8_e4m3fn
    assert torch.equal(rstd, rstd_r)
    assert (s is None and s_r is None) if not fused else torch.equal(s, s_r)
    assert torch.equal(_u8(q), _u8(q_ref))
    assert torch.equal(_u8(qt), _u8(qt_ref))
    assert st[0].item() == st_ref[0].item() == y.float().abs().max().item()
    assert (y.float().abs() * RMS_SCALE > 448).any() and (_u8(q) & 0x7f).max().item() == 0x7e  # it saturated
    ref, env = LO.rmsnorm_oracle(x, w, LO.EPS, h=h)
    for name, got, r, e in (("yq", q, ref["y"], env["y"]), ("yqt", qt, ref["y"].t(), env["y"].t())):
        worst, bad, cnt = fp8_worst_ratio(got.cpu(), RMS_SCALE, r, e, LO.RMS_C)
        print(f"rms_fwd_fp8 {n}x{d} {name}: worst error / envelope {worst:.3f} over {cnt} unsaturated elements")
        assert bad == 0 and cnt > 0.9 * n * d, (name, worst, bad)
    if fused:
        assert torch.equal(s.cpu(), ref["s"])


@pytest.mark.parametrize("n,d", [(48, 2048), (24, 512), (48, 384)])
def test_rms_fwd_fp8_refuses_unserved_shapes(n, d):
    x = torch.randn(n, d, device="cuda").bfloat16()
    with pytest.raises(RuntimeError, match="rms_fwd_fp8"):
        _C().rms_fwd_fp8(x, torch.ones(d, device="cuda"), LO.EPS, torch.zeros_like(x), _st(1.0))


def test_rms_fp8_ok_falls_back_in_python():
    """The Python gate in front of the kernel: D = 2048 (K = 8) and N % 16 != 0 keep the bf16 kernel + cast."""
    from pytorch_distributed_training_example_amd.ops.fp8 import rms_fp8_ok
    from pytorch_distributed_training_example_amd.ops.rmsnorm import RMSNorm
    for (n, d), want in (((48, 256), True), ((48, 1536), True), ((48, 2048), False), ((24, 512), False)):
        x = torch.zeros(n, d, device="cuda", dtype=BF16)
        assert rms_fp8_ok(x, x, RMSNorm(d).cuda()) is want, (n, d)


# ----------------------------------------------------------------------------- 2. / 3. fp8_swiglu_cast
SWIGLU_SCALE = 32.0
SWIGLU_SHAPES = [(16, 64), (48, 192), (144, 128), (3088, 2816)]


def _swiglu_case(m, f):
    gu, dy = LO.swiglu_inputs(m, f, BF16)
    gu[0, :8] = torch.tensor([25.0, -25.0, 60.0, -95.0, 21.0, -21.0, 88.0, -88.0])  # both tails of the gate
    gu[m - 1, f - 4:f] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    return gu, dy


@pytest.mark.parametrize("m,f", SWIGLU_SHAPES)
def test_swiglu_cast_fwd_bit_identical_to_unfused(m, f):
    """fp8(silu(g) u) and its transpose in one pass == swiglu_fwd then cast-transpose, and inside the oracle's
    e4m3 envelope."""
    C = _C()
    gu, _ = _swiglu_case(m, f)
    gug = gu.cuda()
    st_ref, st = _st(SWIGLU_SCALE), _st(SWIGLU_SCALE)
    a = C.swiglu_fwd(gug)
    q_ref, qt_ref = C.fp8_cast_transpose(a, st_ref, True)
    q, qt = C.fp8_swiglu_cast(gug, None, st)
    assert q.shape == (m, f) and qt.shape == (f, m)
    assert torch.equal(_u8(q), _u8(q_ref))
    assert torch.equal(_u8(qt), _u8(qt_ref))
    assert st[0].item() == st_ref[0].item() == a.float().abs().max().item()
    ref, env = LO.swiglu_oracle(gu)
    for name, got, r, e in (("aq", q, ref["y"], env["y"]), ("aqt", qt, ref["y"].t(), env["y"].t())):
        worst, bad, cnt = fp8_worst_ratio(got.cpu(), SWIGLU_SCALE, r, e, LO.SWIGLU_C)
        print(f"fp8_swiglu_cast fwd {m}x{f} {name}: worst error / envelope {worst:.3f} over {cnt} unsaturated")
        assert bad == 0 and cnt > 0.9 * m * f, (name, worst, bad)


@pytest.mark.parametrize("m,f", SWIGLU_SHAPES)
def test_swiglu_cast_bwd_bit_identical_to_unfused(m, f):
    """fp8([dg | du]) and its transpose from (dy, gu) == swiglu_bwd then cast-transpose: one scale and one amax
    over both halves; and inside the oracle's e4m3 envelope."""
    C = _C()
    gu, dy = _swiglu_case(m, f)
    gug, dyg = gu.cuda(), dy.cuda()
    st_ref, st = _st(SWIGLU_SCALE), _st(SWIGLU_SCALE)
    dgu = C.swiglu_bwd(dyg, gug)
    q_ref, qt_ref = C.fp8_cast_transpose(dgu, st_ref, True)
    q, qt = C.fp8_swiglu_cast(gug, dyg, st)
    assert q.shape == (m, 2 * f) and qt.shape == (2 * f, m)
    assert torch.equal(_u8(q), _u8(q_ref))
    assert torch.equal(_u8(qt), _u8(qt_ref))
    assert st[0].item() == st_ref[0].item() == dgu.float().abs().max().item()
    ref, env = LO.swiglu_oracle(gu, dy)
    r, e = torch.cat([ref["dg"], ref["du"]], -1), torch.cat([env["dg"], env["du"]], -1)
    for name, got, rr, ee in (("dguq", q, r, e), ("dguqt", qt, r.t(), e.t())):
        worst, bad, cnt = fp8_worst_ratio(got.cpu(), SWIGLU_SCALE, rr, ee, LO.SWIGLU_C)
        print(f"fp8_swiglu_cast bwd {m}x{f} {name}: worst error / envelope {worst:.3f} over {cnt} unsaturated")
        assert bad == 0 and cnt > 0.9 * 2 * m * f, (name, worst, bad)


@pytest.mark.parametrize("m,f", [(16, 72), (24, 64)])
@pytest.mark.parametrize("bwd", [False, True])
def test_swiglu_cast_refuses_unserved_shapes(m, f, bwd):
    gu = torch.randn(m, 2 * f, device="cuda").bfloat16()
    dy = torch.randn(m, f, device="cuda").bfloat16() if bwd else None
    with pytest.raises(RuntimeError, match="fp8_swiglu_cast"):
        _C().fp8_swiglu_cast(gu, dy, _st(1.0))


# ----------------------------------------------------------------------------- 4. striped rows
@pytest.mark.parametrize("kind", ["rms", "swiglu_fwd", "swiglu_bwd"])
def test_striped_amax_rows(kind):
    """The new producers writing into a striped state row (Fp8State): after update() the newest history entry
    is the unstriped run's amax, the stripes are cleared, and the bytes equal the unstriped run's."""
    from pytorch_distributed_training_example_amd.ops.fp8 import Fp8State
    C = _C()
    torch.manual_seed(9)
    st = Fp8State(1, history=4).cuda()
    st.state[0, 1], st.state[0, 2] = 8.0, 0.125
    ref = _st(8.0)
    if kind == "rms":
        x, h = torch.randn(4112, 1024, device="cuda").bfloat16(), torch.randn(4112, 1024, device="cuda").bfloat16()
        w = torch.rand(1024, device="cuda") + 0.5
        got, want = C.rms_fwd_fp8(x, w, LO.EPS, h, st.state[0])[:2], C.rms_fwd_fp8(x, w, LO.EPS, h, ref)[:2]
    else:
        gu = (torch.randn(1040, 2 * 1024, device="cuda") * 2).bfloat16()
        dy = torch.randn(1040, 1024, device="cuda").bfloat16() if kind == "swiglu_bwd" else None
        got, want = C.fp8_swiglu_cast(gu, dy, st.state[0]), C.fp8_swiglu_cast(gu, dy, ref)
    for a, b in zip(got, want):
        assert torch.equal(_u8(a), _u8(b))
    assert st.state[0, 0].item() == 0.0  # the stripes took every workgroup's maximum
    assert (st.state[0, 4:Fp8State.STRIPED] > 0).sum().item() == 16  # every stripe was written
    st.update()
    assert st.state[0, Fp8State.STRIPED].item() == ref[0].item() > 0
    assert (st.state[0, 4:Fp8State.STRIPED] == 0).all()


# ----------------------------------------------------------------------------- 5. model level
@pytest.mark.parametrize("heads,kv_heads", [(8, 8), (8, 2)])
def test_llama_blocks_fused_fp8_matches_per_linear_path(heads, kv_heads):
    """Two LlamaBlocks + the final RMSNorm, fp8: the e4m3-emitting add+RMSNorm and SwiGLU casts (PDT_FP8_LN,
    PDT_FP8_SWIGLU) against the per-Linear path (bf16 RMSNorm / SwiGLU, then a cast pass) — bit-identical
    output, input gradient, parameter gradients and folded state; multi-head and grouped-query."""
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models.llama import LlamaBlock, LlamaConfig, run_llama_blocks
    from pytorch_distributed_training_example_amd.ops.fp8 import enable_fp8
    from pytorch_distributed_training_example_amd.ops.rmsnorm import RMSNorm
    from pytorch_distributed_training_example_amd.ops.rope import RotaryTable
    torch.manual_seed(7)
    cfg = LlamaConfig(n_layer=2, n_head=heads, n_embd=512, ffn=1024, block_size=48, n_kv_head=kv_heads)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = torch.nn.ModuleList([LlamaBlock(cfg) for _ in range(2)])
            self.ln_f = RMSNorm(512, eps=cfg.eps)
            self.rope = RotaryTable(48, cfg.rope_base, 64)

        def forward(self, x):
            return run_llama_blocks(self.blocks, x, self.ln_f, self.rope)
    net = Net().cuda()
    for m in net.modules():  # bf16 weights, fp32 RMSNorm parameters and RoPE table (models/precision.py)
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.normal_(m.weight, 0.0, 0.03)
            m.to(BF16)
    x0 = torch.randn(4, 48, 512, device="cuda").bfloat16()
    g = torch.randn(4, 48, 512, device="cuda").bfloat16()
    res, fns = {}, {}
    saved = (SW.fp8_ln, SW.fp8_swiglu)
    try:
        for on in (False, True):
            SW.fp8_ln = SW.fp8_swiglu = on
            st = enable_fp8(net, history=4)
            assert st.state.shape[0] == 3 * 4 * 2
            for _ in range(3):  # two calibration passes, then the compared one
                net.zero_grad(set_to_none=True)
                x = x0.clone().requires_grad_(True)
                y = net(x)
                y.backward(g)
            st.update()  # folds the amax stripes (which workgroup wrote which stripe differs by path)
            res[on] = [y, x.grad, st.state.clone()] + [p.grad.clone() for p in net.parameters()]
            names, todo, seen = set(), [y.grad_fn], set()
            while todo:
                fn = todo.pop()
                if fn is None or fn in seen:
                    continue
                seen.add(fn)
                names.add(type(fn).__name__)
                todo.extend(f for f, _ in fn.next_functions)
            fns[on] = names
            net._fp8_hook.remove()
    finally:
        SW.fp8_ln, SW.fp8_swiglu = saved
    fused = {n for n in fns[True] if n.startswith(("_AddRMSFp8Fn", "_Fp8SwigluMlpFn"))}
    assert len(fused) == 2 and not {n for n in fns[False] if n.startswith(("_AddRMSFp8Fn", "_Fp8SwigluMlpFn"))}
    assert any(n.startswith("_SwiGLUFn") for n in fns[False]) and any(n.startswith("_Fp8LinearFn") for n in fns[False])
    assert all(torch.isfinite(t.float()).all() for t in res[True]) and res[True][0].float().abs().max() > 0
    for i, (a, b) in enumerate(zip(res[False], res[True])):
        assert torch.equal(a, b), i


# ----------------------------------------------------------------------------- 6. / 7. fp8 against bf16
# Measured on an MI355X and recorded in profiles/r17/llama_fp8_numerics.txt; every bound below is twice the
# measured figure (no bound is known in advance for two whole blocks).
FP8_VS_BF16 = {
    "logits": 6.3290e-02,
    "transformer.wte.weight": 7.8690e-02,
    "transformer.h.0.ln_1.weight": 9.5185e-02,
    "transformer.h.0.attn.c_attn.weight": 8.6155e-02,
    "transformer.h.0.attn.c_proj.weight": 8.1571e-02,
    "transformer.h.0.ln_2.weight": 8.4021e-02,
    "transformer.h.0.mlp.c_fc.weight": 9.0451e-02,
    "transformer.h.0.mlp.c_proj.weight": 8.9387e-02,
    "transformer.h.1.ln_1.weight": 8.4790e-02,
    "transformer.h.1.attn.c_attn.weight": 7.6229e-02,
    "transformer.h.1.attn.c_proj.weight": 7.9631e-02,
    "transformer.h.1.ln_2.weight": 1.0696e-01,
    "transformer.h.1.mlp.c_fc.weight": 1.0171e-01,
    "transformer.h.1.mlp.c_proj.weight": 1.0165e-01,
    "transformer.ln_f.weight": 5.9177e-02,
    "lm_head.weight": 6.3361e-02,
}
FP8_TRAIN_GAP = 1.6175e-05  # |last fp8 loss - last bf16 loss| after 30 steps


def _batch(seed, b=B):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (b, T), generator=g).cuda(), torch.randint(0, V, (b, T), generator=g).cuda()


def _pair():
    """llama_tiny in fp8 and in bf16 from the same weights."""
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    torch.manual_seed(0)
    base = get_model("llama_tiny").cuda()
    return apply_precision(copy.deepcopy(base), "fp8"), apply_precision(copy.deepcopy(base), "bf16")


def fp8_vs_bf16_ratios():
    """|fp8 - bf16| / |bf16| as norm ratios, for the logits and every parameter gradient, after two
    calibration passes of the delayed scales."""
    m8, m16 = _pair()
    x, y = _batch(0)
    for _ in range(3):
        m8.zero_grad(set_to_none=True)
        m8(x, y).backward()
    m16(x, y).backward()
    with torch.no_grad():
        m8.train()
        l8, l16 = m8(x).float(), m16(x).float()
    out = {"logits": ((l8 - l16).norm() / l16.norm()).item()}
    g16 = dict(m16.named_parameters())
    for n, p in m8.named_parameters():
        out[n] = ((p.grad.float() - g16[n].grad.float()).norm() / g16[n].grad.float().norm()).item()
    return out


def test_fp8_close_to_bf16():
    got = fp8_vs_bf16_ratios()
    for n, r in got.items():
        print(f"fp8 vs bf16 {n}: {r:.4e}")
    assert set(got) == set(FP8_VS_BF16), sorted(set(got) ^ set(FP8_VS_BF16))
    for n, r in got.items():
        assert math.isfinite(r) and r <= 2 * FP8_VS_BF16[n], (n, r, FP8_VS_BF16[n])


def train_losses(precision, steps=30):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    from pytorch_distributed_training_example_amd.optim import FusedAdamW
    torch.manual_seed(0)
    m = apply_precision(get_model("llama_tiny").cuda(), precision)
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    x, y = _batch(1)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = m(x, y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).float().cpu()


def test_llama_tiny_fp8_trains():
    l8, l16 = train_losses("fp8"), train_losses("bf16")
    gap = abs(l8[-1].item() - l16[-1].item())
    print(f"fp8 losses first {l8[0].item():.4f} last {l8[-1].item():.4f}; bf16 last {l16[-1].item():.4f}; gap {gap:.4e}")
    assert torch.isfinite(l8).all(), l8
    assert l8[-1] < l8[0], l8
    assert gap <= 2 * FP8_TRAIN_GAP, (gap, FP8_TRAIN_GAP)


# ----------------------------------------------------------------------------- 8. capture
def _train(base, mode, steps=3, lr=1e-3):
    """``steps`` AdamW steps on fresh batches after the warm-up steps (tests/test_llama_gpu.py _train); the
    losses, the final parameters and the fp8 state."""
    from pytorch_distributed_training_example_amd.engine.graph import StaticStep
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    from pytorch_distributed_training_example_amd.optim import FusedAdamW
    m = apply_precision(copy.deepcopy(base), "fp8")
    opt = FusedAdamW(m.parameters(), lr=lr, weight_decay=0.01)

    def step(x, y):
        opt.zero_grad(set_to_none=True)
        loss = m(x, y)
        loss.backward()
        opt.step()
        return loss.detach()

    data = [_batch(10 + i) for i in range(steps + 1)]
    out = []
    if mode == "eager":
        for _ in range(3):
            step(*data[0])
        for x, y in data[1:]:
            out.append(float(step(x, y)))
    else:
        runner = StaticStep(step, list(data[0]), warmup=3)
        runner.capture()
        for x, y in data[1:]:
            out.append(float(runner(x, y)))
    torch.cuda.synchronize()
    return torch.tensor(out), [p.detach().float().clone() for p in m.parameters()], m.fp8_state.state.clone()


def test_graph_fp8_step_matches_eager_step():
    """Three replays of a StaticStep-captured fp8 step equal the three eager steps bit for bit: losses, final
    parameters and the Fp8State buffer (the delayed scales advance on replay)."""
    from pytorch_distributed_training_example_amd.models import get_model
    torch.manual_seed(0)
    base = get_model("llama_tiny").cuda()
    le, pe, se = _train(base, "eager")
    lg, pg, sg = _train(base, "graph")
    assert torch.equal(lg, le), (lg, le)
    bad = [i for i, (a, b) in enumerate(zip(pg, pe)) if not torch.equal(a, b)]
    assert not bad, f"{len(bad)} of {len(pe)} parameters differ after the replayed steps (first: {bad[:5]})"
    assert torch.equal(sg, se)
    hist = se[:, 260:]  # six forwards: the first update pushed an empty amax, the other five a step's each
    assert (hist[:, :5] > 0).all() and (hist[:, 5:] == 0).all() and se.shape[0] == 3 * 4 * 2


# ----------------------------------------------------------------------------- 9. command line
CLI_ARGS = ["--precision", "fp8", "--steps-per-epoch", "2", "--epochs", "1", "--batch-size", "4", "--seq-len", "32",
            "--world-size", "1", "--no-eval"]


def test_cli_accepts_fp8_for_llama_on_the_gpu(tmp_path, monkeypatch):
    from pytorch_distributed_training_example_amd import cli
    monkeypatch.chdir(tmp_path)
    assert cli.main(["--model", "llama_tiny"] + CLI_ARGS) == 0


def test_train_cli_llama_tiny_gqa_fp8_two_steps(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--model", "llama_tiny_gqa"] + CLI_ARGS,
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Loss: ([-+0-9.eE]+|nan|inf)", r.stdout)]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
