"""SyncBatchNorm on the CPU tier (two gloo ranks, the fp32 reference path of ops/sync_batchnorm.py): two
ranks with uneven shards must compute what one process computes on the concatenated batch; conversion keeps
parameters, buffers and checkpoints; one rank / eval mode is plain BatchNorm2d without any collective."""
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

from dist_utils import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1")

SHARDS, C, H, W = (3, 5), 64, 5, 7
EPS, MOM = 1e-5, 0.1
TOL = dict(rtol=1e-5, atol=1e-5)  # fp32 path against the fp64 reference (torch.testing's fp32 defaults are tighter)


def _shard(r, n=None, c=C, h=H, w=W):
    """Rank r's (x, residual, g): data shifted by (-1)^r, std 2; loss = sum(y * g)."""
    gen = torch.Generator().manual_seed(100 + r)
    n = SHARDS[r] if n is None else n
    x = torch.randn(n, c, h, w, generator=gen) * 2.0 + (-1.0) ** r
    res = torch.randn(n, c, h, w, generator=gen)
    g = torch.randn(n, c, h, w, generator=gen)
    return x, res, g


def _affine(c=C):
    gen = torch.Generator().manual_seed(7)
    return torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)


def full_batch_reference(xs, ress, gs, weight, bias):
    """fp64 F.batch_norm + residual + ReLU over the concatenated batch: y, dx, dgamma, dbeta, running stats."""
    x = torch.cat(xs).double().requires_grad_()
    res = torch.cat(ress).double()
    g = torch.cat(gs).double()
    w = weight.double().requires_grad_()
    b = bias.double().requires_grad_()
    rm, rv = torch.zeros(x.shape[1], dtype=torch.float64), torch.ones(x.shape[1], dtype=torch.float64)
    y = F.relu(F.batch_norm(x, rm, rv, w, b, True, MOM, EPS) + res)
    (y * g).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dg=w.grad, db=b.grad, rm=rm, rv=rv)


def _sync_worker(rank, world):
    from pytorch_distributed_training_example_amd.ops.batchnorm import batch_norm_act
    from pytorch_distributed_training_example_amd.ops.sync_batchnorm import sync_batch_norm_act
    x, res, g = _shard(rank)
    weight, bias = _affine()
    out = {}
    for name in ("sync", "local"):
        xr = x.clone().requires_grad_()
        w, b = weight.clone().requires_grad_(), bias.clone().requires_grad_()
        rm, rv = torch.zeros(C), torch.ones(C)
        if name == "sync":
            y, mean, invstd = sync_batch_norm_act(xr, res, w, b, rm, rv, True, MOM, EPS, True, None,
                                                  _return_stats=True)
            out["mean"], out["invstd"] = mean, invstd
        else:
            y = batch_norm_act(xr, res, w, b, rm, rv, True, MOM, EPS, True)
        (y * g).sum().backward()
        out[name] = dict(y=y.detach(), dx=xr.grad, dg=w.grad, db=b.grad, rm=rm, rv=rv)
    return out


def test_two_uneven_ranks_equal_the_full_batch():
    outs = run_ranks(_sync_worker, 2)
    shards = [_shard(r) for r in range(2)]
    weight, bias = _affine()
    ref = full_batch_reference(*zip(*shards), weight, bias)
    off = 0
    for r, o in enumerate(outs):
        n = SHARDS[r]
        s = o["sync"]
        torch.testing.assert_close(s["y"].double(), ref["y"][off:off + n], **TOL)
        torch.testing.assert_close(s["dx"].double(), ref["dx"][off:off + n], **TOL)
        # running statistics of the full batch (unbiased with N = 8 * 35)
        torch.testing.assert_close(s["rm"].double(), ref["rm"], **TOL)
        torch.testing.assert_close(s["rv"].double(), ref["rv"], **TOL)
        off += n
    # the weight / bias gradients stay local: their sum over the ranks is the full-batch one
    torch.testing.assert_close((outs[0]["sync"]["dg"] + outs[1]["sync"]["dg"]).double(), ref["dg"], **TOL)
    torch.testing.assert_close((outs[0]["sync"]["db"] + outs[1]["sync"]["db"]).double(), ref["db"], **TOL)
    for k in ("mean", "invstd"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    for k in ("rm", "rv"):
        assert torch.equal(outs[0]["sync"][k], outs[1]["sync"][k]), k
    # power: per-rank statistics (the unsynced BatchNorm) miss the full-batch output almost everywhere
    off = 0
    for r, o in enumerate(outs):
        n = SHARDS[r]
        want = ref["y"][off:off + n]
        miss = (o["local"]["y"].double() - want).abs() > TOL["atol"] + TOL["rtol"] * want.abs()
        assert miss.float().mean() > 0.5, (r, miss.float().mean())
        off += n


def test_convert_sync_batchnorm_resnet18():
    from torch import nn
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.ops.batchnorm import BatchNorm2d
    from pytorch_distributed_training_example_amd.parallel import SyncBatchNorm, convert_sync_batchnorm
    torch.manual_seed(0)
    model = get_model("resnet18", num_classes=10)
    for m in model.modules():  # make the buffers and parameters distinguishable
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_()
            m.weight.data.uniform_(0.5, 1.5)
    nbn = sum(isinstance(m, nn.BatchNorm2d) for m in model.modules())
    relu_flags = {n: m.fused_relu for n, m in model.named_modules() if isinstance(m, BatchNorm2d)}
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = {n: p for n, p in model.named_parameters()}
    model.train()
    conv = convert_sync_batchnorm(model)
    assert conv is model
    bns = {n: m for n, m in conv.named_modules() if isinstance(m, nn.BatchNorm2d)}
    assert len(bns) == nbn == 20 and all(type(m) is SyncBatchNorm for m in bns.values())
    assert not any(isinstance(m, BatchNorm2d) for m in conv.modules())
    assert {n: m.fused_relu for n, m in bns.items()} == relu_flags and any(relu_flags.values())
    assert all(m.training for m in bns.values())
    after = conv.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    # the same Parameter objects: an optimizer / DDP wrapper built before the conversion still sees them
    now = {n: p for n, p in conv.named_parameters()}
    assert list(now) == list(params) and all(now[n] is params[n] for n in params)
    # a checkpoint of the converted model loads into an unconverted one
    plain = get_model("resnet18", num_classes=10)
    plain.load_state_dict(after, strict=True)
    for k, v in plain.state_dict().items():
        assert torch.equal(v, before[k]), k
    # and torch's own BatchNorm2d is converted as well, eval flag kept
    seq = nn.Sequential(nn.Conv2d(3, 8, 1), nn.BatchNorm2d(8, eps=1e-3, momentum=0.2)).eval()
    seq = convert_sync_batchnorm(seq)
    assert type(seq[1]) is SyncBatchNorm and not seq[1].training and seq[1].eps == 1e-3 and seq[1].momentum == 0.2
    assert seq[1].fused_relu is False


def _count_all_reduce(monkeypatch):
    import torch.distributed as dist
    calls = []
    real = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(dist, "all_reduce", counted)
    return calls


def _fallback_worker(rank, world):
    """World size 1 WITH an initialised group: no collective, the local BatchNorm's bits."""
    import torch.distributed as dist
    from pytorch_distributed_training_example_amd.ops.batchnorm import BatchNorm2d
    from pytorch_distributed_training_example_amd.parallel import SyncBatchNorm
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        x, res, _ = _shard(0)
        a, b = BatchNorm2d(C, fused_relu=True), SyncBatchNorm(C, fused_relu=True)
        ya, yb = a(x, residual=res), b(x, residual=res)
    finally:
        dist.all_reduce = real
    return torch.equal(ya, yb), torch.equal(a.running_var, b.running_var), len(calls)


def test_world_one_and_eval_are_plain_batchnorm(monkeypatch):
    from pytorch_distributed_training_example_amd.ops.batchnorm import BatchNorm2d
    from pytorch_distributed_training_example_amd.parallel import SyncBatchNorm
    (same_y, same_rv, ncalls), = run_ranks(_fallback_worker, 1)
    assert same_y and same_rv and ncalls == 0
    # no process group at all, train and eval
    calls = _count_all_reduce(monkeypatch)
    x, res, _ = _shard(0)
    a, b = BatchNorm2d(C, fused_relu=True), SyncBatchNorm(C, fused_relu=True)
    for mode in (True, False):
        a.train(mode), b.train(mode)
        assert torch.equal(a(x, residual=res), b(x, residual=res))
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    assert not calls


def _eval_worker(rank, world):
    """Eval mode on two ranks: running statistics, no collective."""
    import torch.distributed as dist
    from pytorch_distributed_training_example_amd.ops.batchnorm import BatchNorm2d
    from pytorch_distributed_training_example_amd.parallel import SyncBatchNorm
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        x, res, _ = _shard(rank)
        a, b = BatchNorm2d(C).eval(), SyncBatchNorm(C).eval()
        same = torch.equal(a(x, residual=res, relu=True), b(x, residual=res, relu=True))
    finally:
        dist.all_reduce = real
    return same, len(calls)


def test_eval_mode_two_ranks_issues_no_collective():
    for same, ncalls in run_ranks(_eval_worker, 2):
        assert same and ncalls == 0


def _cli(args, cwd, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--no-cuda", "--world-size", "2", "--model", "resnet18",
           "--sync-bn", "--synthetic", "yes"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=str(cwd), env=ENV)


def test_cli_sync_bn_two_ranks(tmp_path):
    r = _cli(["--steps-per-epoch", "2", "--epochs", "1", "--no-eval", "--check-sync", "--batch-size", "4",
              "--image-size", "32"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "--sync-bn: 20 BatchNorm2d converted to SyncBatchNorm" in r.stdout


def test_cli_sync_bn_rejects_hipgraph_on_two_ranks(tmp_path):
    from pytorch_distributed_training_example_amd.cli import SYNC_BN_HIPGRAPH_MSG
    r = _cli(["--hipgraph", "--steps-per-epoch", "1", "--epochs", "1"], tmp_path, timeout=120)
    assert r.returncode != 0
    assert SYNC_BN_HIPGRAPH_MSG in r.stderr
