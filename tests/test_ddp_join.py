"""DistributedDataParallel.join(): uneven per-rank step counts on CPU/gloo, against torch DDP's own join()."""
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from dist_utils import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
ATOL = 1e-6  # ours vs torch DDP, the bound of test_ddp.py::test_ddp_matches_torch_ddp


def _model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.ReLU(), nn.Linear(8, 4))


def _batches(rank, n, seed=100):
    g = torch.Generator().manual_seed(seed + rank)
    return [(torch.randn(4, 8, generator=g), torch.randn(4, 4, generator=g)) for _ in range(n)]


def _ours(**kw):
    from pytorch_distributed_training_example_amd.parallel import DistributedDataParallel
    return DistributedDataParallel(_model(), **kw)


def _torch_ddp():
    return torch.nn.parallel.DistributedDataParallel(_model())


def _state(ddp):
    return {k: v.detach().clone() for k, v in ddp.module.state_dict().items()}


def _steps(ddp, opt, batches):
    for x, y in batches:
        opt.zero_grad()
        nn.functional.mse_loss(ddp(x), y).backward()
        opt.step()


def _run_join(ddp, batches, join_kw, micro=False):
    """Train ``ddp`` over ``batches`` inside join(); ``micro``: two micro-batches per step, the first no_sync."""
    opt = torch.optim.SGD(ddp.parameters(), lr=0.1)
    with ddp.join(**join_kw):
        if not micro:
            _steps(ddp, opt, batches)
        else:
            for (x1, y1), (x2, y2) in zip(batches[0::2], batches[1::2]):
                opt.zero_grad()
                with ddp.no_sync():
                    nn.functional.mse_loss(ddp(x1), y1).backward()
                nn.functional.mse_loss(ddp(x2), y2).backward()
                opt.step()
    return _state(ddp)


def _assert_same(a, b, exact=False):
    assert list(a) == list(b)
    for k in a:
        if exact:
            assert torch.equal(a[k], b[k]), k
        else:
            torch.testing.assert_close(a[k], b[k], rtol=0, atol=ATOL, msg=lambda m, k=k: f"{k}: {m}")


def _assert_ranks_equal(states):
    for s in states[1:]:
        _assert_same(states[0], s, exact=True)


# ---------------------------------------------------------------- 1. against torch's join
def _vs_torch(rank, world, counts, divide, ours_kw, micro):
    kw = dict(divide_by_initial_world_size=divide)
    n = counts[rank] * (2 if micro else 1)
    ours = _ours(**ours_kw)
    mine = _run_join(ours, _batches(rank, n), kw, micro)
    ref = _run_join(_torch_ddp(), _batches(rank, n), kw, micro)
    return mine, ref, [(list(s.indices), list(s.offsets)) for s in ours.bucket_specs()], ours._rebuilt


@pytest.mark.parametrize("divide", [True, False])
@pytest.mark.parametrize("counts", [(3, 1), (1, 3), (2, 0), (3, 1, 2)])
def test_join_matches_torch_join(counts, divide):
    res = run_ranks(_vs_torch, world=len(counts), args=(counts, divide, {}, False))
    for mine, ref, _, _ in res:
        _assert_same(mine, ref)
    _assert_ranks_equal([r[0] for r in res])
    assert int(res[0][0]["1.num_batches_tracked"]) == max(counts)  # the model that took every step


# ---------------------------------------------------------------- 2. bucket rebuild inside join
@pytest.mark.parametrize("divide", [True, False])
def test_join_bucket_rebuild_in_shadowed_iteration(divide):
    kw = dict(rebuild_buckets=True, bucket_cap_mb=1e-6, first_bucket_mb=1e-6)
    res = run_ranks(_vs_torch, world=2, args=((3, 1), divide, kw, False))
    for mine, ref, specs, rebuilt in res:
        _assert_same(mine, ref)
        assert rebuilt and len(specs) == 6  # one bucket per tensor; the rebuild ran on the shadowing rank too
        assert specs == res[0][2]
    _assert_ranks_equal([r[0] for r in res])


# ---------------------------------------------------------------- 3. no_sync inside join
@pytest.mark.parametrize("divide", [True, False])
def test_join_with_no_sync_micro_batches(divide):
    """Parameters against torch DDP run the same way. The BatchNorm running statistics are NOT compared with
    torch's: torch skips the buffer broadcast in the forward that follows a no_sync forward (its
    ``require_forward_param_sync`` flag), our wrapper broadcasts buffers in every forward, inside join() and
    outside it, so rank 0's running statistics after micro-batch 1 are overwritten by rank 1's here and kept
    there (measured: running_mean differs by up to 0.07). Training-mode BatchNorm does not read them, so
    the parameters are unaffected. The buffers must still be the last joiner's on every rank."""
    res = run_ranks(_vs_torch, world=2, args=((2, 1), divide, {}, True))
    for mine, ref, _, _ in res:
        params = [k for k in mine if "running" not in k]
        assert len(params) == 7
        _assert_same({k: mine[k] for k in params}, {k: ref[k] for k in params})
    _assert_ranks_equal([r[0] for r in res])
    assert int(res[0][0]["1.num_batches_tracked"]) == 4


# ---------------------------------------------------------------- 4. comm hook
def _hook(rank, world, counts, divide):
    from pytorch_distributed_training_example_amd.parallel import comm_hooks
    kw = dict(divide_by_initial_world_size=divide)
    plain = _run_join(_ours(), _batches(rank, counts[rank]), kw)
    hooked = _ours()
    hooked.register_comm_hook(None, comm_hooks.allreduce_hook)
    return plain, _run_join(hooked, _batches(rank, counts[rank]), kw)


@pytest.mark.parametrize("divide", [True, False])
def test_join_comm_hook_same_result(divide):
    """World 2: the hook's SUM / 2 (x 2 / active) and the plain SUM / 2 (SUM x 1 / active) scale by powers of
    two only, so the results are the same bits."""
    res = run_ranks(_hook, world=2, args=((3, 1), divide))
    for plain, hooked in res:
        _assert_same(plain, hooked, exact=True)
    _assert_ranks_equal([r[1] for r in res])


# ---------------------------------------------------------------- 5. debug mode
def _debug(rank, world, counts, divide):
    ddp = _ours(debug=True, bucket_cap_mb=1e-6, first_bucket_mb=1e-6)
    out = _run_join(ddp, _batches(rank, counts[rank]), dict(divide_by_initial_world_size=divide))
    return out, ddp._debug.step


@pytest.mark.parametrize("divide", [True, False])
def test_join_debug_mode_no_desync(divide):
    res = run_ranks(_debug, world=2, args=((3, 1), divide))
    assert [r[1] for r in res] == [3, 3]  # the shadowing rank went through every post-backward check
    _assert_ranks_equal([r[0] for r in res])


# ---------------------------------------------------------------- 6. throw_on_early_termination
def _throw(rank, world, counts):
    ddp = _ours()
    try:
        _run_join(ddp, _batches(rank, counts[rank]), dict(throw_on_early_termination=True))
    except RuntimeError as e:
        return str(e), ddp._join is None
    return None, ddp._join is None


def test_join_throw_on_early_termination():
    res = run_ranks(_throw, world=2, args=((3, 1),))
    assert res[0][0] == "Detected at least one rank that exhausted inputs. Throwing across all ranks."
    assert res[1][0] == "Rank 1 exhausted all inputs."
    assert res[0][1] and res[1][1]


# ---------------------------------------------------------------- 7. re-entry
def _twice(rank, world):
    ddp = _ours()
    a = _run_join(ddp, _batches(rank, (2, 1)[rank]), {})
    b = _run_join(ddp, _batches(rank, (1, 2)[rank], seed=200), {})
    return a, b


def test_join_two_consecutive_contexts():
    res = run_ranks(_twice, world=2)
    _assert_ranks_equal([r[0] for r in res])
    _assert_ranks_equal([r[1] for r in res])
    assert int(res[0][1]["1.num_batches_tracked"]) == 4  # 2 steps, then 2 more on the other rank
    assert not torch.equal(res[0][0]["0.weight"], res[0][1]["0.weight"])


# ---------------------------------------------------------------- 8. enable=False, world 1, no group
def _noop(rank, world, join_kw):
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(t.numel()), real(t, *a, **k))[1]
    try:
        inside = _run_join(_ours(), _batches(rank, 3), join_kw)
    finally:
        dist.all_reduce = real
    plain = _ours()
    _steps(plain, torch.optim.SGD(plain.parameters(), lr=0.1), _batches(rank, 3))
    return inside, _state(plain), calls


@pytest.mark.parametrize("world,kw", [(2, dict(enable=False)), (1, {})])
def test_join_disabled_or_single_rank_is_a_noop(world, kw):
    for inside, plain, calls in run_ranks(_noop, world=world, args=(kw,)):
        _assert_same(inside, plain, exact=True)
        assert world + 1 not in calls  # no notify


def test_join_without_process_group_is_a_noop():
    inside = _run_join(_ours(), _batches(0, 3), {})
    plain = _ours()
    _steps(plain, torch.optim.SGD(plain.parameters(), lr=0.1), _batches(0, 3))
    _assert_same(inside, _state(plain), exact=True)


# ---------------------------------------------------------------- 9. SyncBatchNorm is refused
def _syncbn(rank, world):
    from pytorch_distributed_training_example_amd.parallel import DistributedDataParallel, convert_sync_batchnorm
    torch.manual_seed(0)
    m = convert_sync_batchnorm(nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4)))
    ddp = DistributedDataParallel(m)
    try:
        with ddp.join():
            raise AssertionError("join() entered")
    except RuntimeError as e:
        return str(e)


def test_join_refuses_sync_batchnorm():
    for msg in run_ranks(_syncbn, world=2):
        assert "SyncBatchNorm" in msg and "join()" in msg


# ---------------------------------------------------------------- 10. outside join nothing changes
_COLLECTIVES = ("all_reduce", "broadcast", "broadcast_object_list", "all_gather", "all_gather_object",
                "all_gather_into_tensor", "reduce", "reduce_scatter", "barrier", "all_to_all", "gather", "scatter")


class _Recorder:
    """Wraps torch.distributed's collective entry points; ``log`` holds (collective, numel, dtype)."""

    def __init__(self):
        self.log = []
        self._real = {}

    def __enter__(self):
        for name in _COLLECTIVES:
            real = getattr(dist, name)
            self._real[name] = real

            def wrapped(*a, _name=name, _real=real, **k):
                t = a[0] if a else None
                if torch.is_tensor(t):
                    self.log.append((_name, t.numel(), str(t.dtype)))
                elif isinstance(t, (list, tuple)):
                    self.log.append((_name, len(t), None))
                else:
                    self.log.append((_name, 0, None))
                return _real(*a, **k)
            setattr(dist, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, real in self._real.items():
            setattr(dist, name, real)


def _record_steps(ddp, batches):
    opt = torch.optim.SGD(ddp.parameters(), lr=0.1)
    per_step = []
    for b in batches:
        with _Recorder() as rec:
            _steps(ddp, opt, [b])
        per_step.append(rec.log)
    return per_step


def _unchanged(rank, world):
    batches = _batches(rank, 4)
    base = _record_steps(_ours(), batches)  # the ``join`` attribute never touched
    ddp = _ours()
    if hasattr(type(ddp), "join"):  # a wrapper that has been through a join() context and left it
        opt = torch.optim.SGD(ddp.parameters(), lr=0.1)
        with ddp.join():
            _steps(ddp, opt, batches[:1])
    else:
        _record_steps(ddp, batches[:1])
    return base, _record_steps(ddp, batches[1:])


def test_collectives_outside_join_unchanged():
    """Three even steps outside join(): the same (collective, numel, dtype) per step as a wrapper whose ``join``
    was never touched (its steps 2-4: step 2 carries the bucket-rebuild broadcast in both), no notify."""
    for base, after in run_ranks(_unchanged, world=2):
        assert len(after) == 3 and after == base[1:]
        assert ("broadcast_object_list", 1, None) in base[1]  # the recorder sees the rebuild
        for step in base + after:
            assert any(c[0] == "all_reduce" for c in step)
            assert not any(c[0] == "all_reduce" and c[1] == 3 for c in step)  # world + 1


# ---------------------------------------------------------------- 11. trainer and CLI
REPRO = ["--no-cuda", "--world-size", "2", "--train-samples", "1001", "--batch-size", "1000", "--epochs", "1",
         "--synthetic", "yes", "--no-eval"]


def test_cli_repro_uneven_shards_trains_to_completion(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + REPRO + ["--save-model"],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Train Epoch: 1 [0/501 (0%)]\tLoss: " in r.stdout
    sd = torch.load(tmp_path / "mnist_cnn.pt", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values())


def _cli_spy(rank, world, samples, extra):
    from pytorch_distributed_training_example_amd import cli
    from pytorch_distributed_training_example_amd.parallel import DistributedDataParallel
    args = cli.build_parser().parse_args([a if a != "1001" else str(samples) for a in REPRO] + list(extra))
    entered = []
    real = DistributedDataParallel.join

    def spy(self, *a, **k):
        entered.append(1)
        return real(self, *a, **k)
    DistributedDataParallel.join = spy
    try:
        cli.run(rank, world, args)
    except RuntimeError as e:
        return len(entered), str(e)
    finally:
        DistributedDataParallel.join = real
    return len(entered), None


def test_cli_even_split_issues_no_join():
    assert run_ranks(_cli_spy, world=2, args=(2000, ())) == [(0, None), (0, None)]


def test_cli_uneven_split_trains_inside_one_join():
    assert run_ranks(_cli_spy, world=2, args=(1001, ())) == [(1, None), (1, None)]


def _assert_refusal(msg, what):
    assert msg is not None and what in msg
    assert "[2, 1]" in msg and "--sharding sampler" in msg and "divisible by world" in msg


def test_cli_reducer_reference_uneven_raises():
    for entered, msg in run_ranks(_cli_spy, world=2, args=(1001, ("--reducer", "reference"))):
        assert entered == 0
        _assert_refusal(msg, "--reducer reference")


def _graph_uneven(rank, world):
    from pytorch_distributed_training_example_amd.engine.trainer import StepConfig, TrainStep, train_epoch
    ddp = _ours()
    step = TrainStep(ddp, torch.optim.SGD(ddp.parameters(), lr=0.1), nn.functional.mse_loss, StepConfig(),
                     raw_model=ddp.module)
    step.enable_graph()
    before = _state(ddp)
    try:
        train_epoch(step, _batches(rank, (2, 1)[rank]), torch.device("cpu"), 1, rank=rank)
    except RuntimeError as e:
        return str(e), before, _state(ddp)
    return None, before, _state(ddp)


def test_train_step_graph_uneven_raises_before_first_step():
    for msg, before, after in run_ranks(_graph_uneven, world=2):
        _assert_refusal(msg, "hipGraph")
        _assert_same(before, after, exact=True)
