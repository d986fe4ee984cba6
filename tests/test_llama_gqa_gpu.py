"""``llama_tiny_gqa`` (4 query heads on 2 K/V heads) end to end on one MI355X: the four tests of
tests/test_llama_gpu.py with its method, helpers and slack constants, on the grouped-query model: the HIP
path against the stock path, both against an fp32 oracle; run-to-run determinism; a hipGraph-captured step
against the eager step; a 2-rank DDP step."""
import copy
import os

import pytest
import torch

from dist_utils import run_ranks
from test_llama_gpu import _batch, _grads, _train

pytestmark = pytest.mark.gpu
NAME = "llama_tiny_gqa"


def _model(seed=0):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(seed)
    return to_bf16_mixed(get_model(NAME).cuda())


def test_llama_gqa_native_matches_reference(slack=1.3):
    """The native bf16 path must be as accurate as the stock bf16 path (PDT_DISABLE_NATIVE=1: SDPA on K/V
    expanded with repeat_interleave), both measured against the fp32 oracle."""
    from pytorch_distributed_training_example_amd.config import SW
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    base = get_model(NAME).cuda()
    assert base.transformer.h[0].attn.c_attn.weight.shape == ((4 + 2 * 2) * 64, 256)
    x, y = _batch(0)
    os.environ["PDT_DISABLE_NATIVE"] = "1"
    SW.reload()
    try:
        l32, g32 = _grads(copy.deepcopy(base), x, y)
        l_ref, g_ref = _grads(to_bf16_mixed(copy.deepcopy(base)), x, y)
    finally:
        os.environ.pop("PDT_DISABLE_NATIVE")
        SW.reload()
    nat = to_bf16_mixed(copy.deepcopy(base))
    l_nat, g_nat = _grads(nat, x, y)
    # the native step really ran the grouped-query kernels
    names = set()
    loss = nat(x, y)
    todo, seen = [loss.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    for want in ("_RMSFn", "_AddRMSFn", "_RopeQKVFn", "_SwiGLUFn", "_FlashGQAFn"):
        assert any(n.startswith(want) for n in names), (want, sorted(names))
    assert not any(n.startswith("_FlashQKVFn") for n in names), sorted(names)
    assert set(g_nat) == set(g32) == set(n for n, _ in base.named_parameters())
    assert abs(l_nat - l32) <= slack * abs(l_ref - l32) + 0.02 * max(1.0, abs(l32)), (l_nat, l_ref, l32)
    e = lambda a, b: ((a - b).norm() / (b.norm() + 1e-9)).item()  # noqa: E731
    e_nat = torch.tensor([e(g_nat[n], g32[n]) for n in g32])
    e_ref = torch.tensor([e(g_ref[n], g32[n]) for n in g32])
    print(f"{NAME}: native median {e_nat.median():.3e} max {e_nat.max():.3e}; stock median {e_ref.median():.3e} "
          f"max {e_ref.max():.3e}")
    assert e_nat.median() <= slack * e_ref.median() + 0.02, (e_nat.median(), e_ref.median())
    assert e_nat.max() <= slack * e_ref.max() + 0.05, (e_nat.max(), e_ref.max())


def test_two_eager_runs_are_bit_identical():
    base = _model()
    la, pa = _train(base, "eager", steps=2)
    lb, pb = _train(base, "eager", steps=2)
    assert torch.equal(la, lb), (la, lb)
    bad = [i for i, (a, b) in enumerate(zip(pa, pb)) if not torch.equal(a, b)]
    assert not bad, f"{len(bad)} of {len(pa)} parameters differ between two runs from the same seed (first: {bad[:5]})"
    assert max(float((a - p0.detach().float()).norm()) for a, p0 in zip(pa, base.parameters())) > 0  # it trained


def test_graph_step_matches_eager_step():
    """Three replays of a StaticStep-captured step equal the three eager steps bit for bit (losses and final
    parameters)."""
    base = _model()
    le, pe = _train(base, "eager", steps=3)
    lg, pg = _train(base, "graph", steps=3)
    assert torch.equal(lg, le), (lg, le)
    bad = [i for i, (a, b) in enumerate(zip(pg, pe)) if not torch.equal(a, b)]
    assert not bad, f"{len(bad)} of {len(pe)} parameters differ after the replayed steps (first: {bad[:5]})"


def _ddp_worker(rank, world):
    from pytorch_distributed_training_example_amd.optim import FusedAdamW
    from pytorch_distributed_training_example_amd.parallel import DistributedDataParallel
    from pytorch_distributed_training_example_amd.parallel.debug import check_replicas_in_sync
    model = _model()
    ref = copy.deepcopy(model)
    ddp = DistributedDataParallel(model, bucket_cap_mb=1, broadcast_buffers=False)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    x, y = _batch(20 + rank, b=2)
    losses, got = [], None
    for it in range(2):
        opt.zero_grad(set_to_none=True)
        loss = ddp(x, y)
        loss.backward()
        if it == 0:
            got = [p.grad.float().cpu() for p in model.parameters()]
        opt.step()
        losses.append(float(loss.detach()))
    check_replicas_in_sync(list(model.parameters()))
    # reference: every rank's gradient on the initial weights, averaged in fp32
    want = None
    for r in range(world):
        ref.zero_grad(set_to_none=True)
        ref(*_batch(20 + r, b=2)).backward()
        g = [p.grad.float().cpu() for p in ref.parameters()]
        want = g if want is None else [a + b for a, b in zip(want, g)]
    want = [a / world for a in want]
    return losses, got, want, [p.detach().float().cpu() for p in model.parameters()], len(ddp._buckets)


def test_ddp_two_ranks_train_in_sync():
    (l0, g0, want, p0, nb), (l1, g1, _, p1, _) = run_ranks(_ddp_worker, 2, use_gpu=True)
    assert nb > 1
    assert l0 != l1  # the ranks saw different batches
    for a, b in zip(g0, g1):
        assert torch.equal(a, b), "replicas must hold identical averaged gradients"
    for a, b in zip(p0, p1):
        assert torch.equal(a, b), "replicas must hold identical parameters after two steps"
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-6)).item()  # noqa: E731
    errs = torch.tensor([rel(a, b) for a, b in zip(g0, want)])
    # a rank's local gradient is the reference's (deterministic kernels); the bucket average rounds to bf16
    assert errs.max() < 1e-2, (errs.median(), errs.max(), int(errs.argmax()))
    init = [p.detach().float().cpu() for p in _model().parameters()]
    assert max(float((a - b).norm()) for a, b in zip(p0, init)) > 0  # it trained
