"""bench.py driver contract, rehearsed on CPU/gloo: the launch line the driver uses
(torch.distributed.run, 127.0.0.1, one rank per device), one JSON line from rank 0 with the
whole-job aggregate, the BASELINE.json metric and the dp<N> parallelism tag."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
        "scaling", "vs_baseline", "dtype", "data", "config"}


def _run(nproc, port, extra=(), self_launch=False):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--steps", "2", "--warmup", "1", "--image-size", "32", *extra]
    if not any(a in ("--batch-size", "--global-batch") for a in extra):
        args += ["--batch-size", "2"]
    if nproc == 1 or self_launch:
        cmd = [sys.executable, "bench.py", "--gpus", str(nproc), *args]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", f"--master-port={port}", "bench.py", "--gpus", str(nproc), *args]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    return json.loads(lines[0])


@pytest.mark.parametrize("nproc,port", [(1, 0), (4, 29671)])
def test_bench_json_contract(nproc, port):
    r = _run(nproc, port)
    assert KEYS <= set(r)
    baseline = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert r["metric"] == baseline["metric"]
    assert r["n_gpus"] == nproc and r["steps"] == 2 and r["warmup"] == 1
    assert r["config"]["model"] == "resnet50" and r["config"]["parallelism"] == f"dp{nproc}"
    assert r["config"]["global_batch"] == 2 * nproc
    assert r["scaling"] == "weak" and r["higher_is_better"] is True and r["dtype"] == "bf16"
    # value is the whole-job aggregate derived from the (max over ranks) step time
    assert r["value"] == pytest.approx(2 * nproc / (r["ms_per_step"] / 1e3), rel=1e-2)


def test_bench_gpus_flag_self_launches():
    """``python bench.py --gpus 4`` (no launcher) must run 4 ranks itself, like the reference's one
    command that uses every GPU (train.py:138,147)."""
    r = _run(4, 0, self_launch=True)
    assert r["n_gpus"] == 4 and r["config"]["parallelism"] == "dp4"
    assert r["config"]["global_batch"] == 8


def test_bench_world_size_mismatch_refused():
    env = dict(os.environ, OMP_NUM_THREADS="2", WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_bench_global_batch_strong_scaling():
    """--global-batch G: per-rank ceil(G/N) (train.py:82), reported as strong scaling."""
    r = _run(2, 0, extra=("--global-batch", "5"), self_launch=True)
    assert r["scaling"] == "strong" and r["config"]["per_gpu_batch"] == 3
    assert r["config"]["global_batch"] == 6 and r["n_gpus"] == 2


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs DIR: the last timed step's loss, logits, updated parameters and gradients as
    float32 .npy (at most 64 MB in all); same arguments -> same inputs, so on CPU (deterministic
    kernels) two runs write identical arrays. --full is accepted and recorded."""
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    ra = _run(1, 0, extra=("--model", "lenet", "--dump-outputs", str(a), "--full"))
    rb = _run(1, 0, extra=("--model", "lenet", "--dump-outputs", str(b)))
    assert ra["config"]["full"] is True and rb["config"]["full"] is False
    assert ra["steps"] == 2 and ra["ms_per_step"] > 0
    assert sorted(p.name for p in a.iterdir()) == ["grads.npy", "logits.npy", "loss.npy", "params.npy"]
    assert sum(p.stat().st_size for p in a.iterdir()) <= 64 * 10 ** 6
    for p in a.iterdir():
        x, y = np.load(p), np.load(b / p.name)
        assert x.dtype == np.float32 and x.shape == y.shape and np.isfinite(x).all()
        if ra["config"]["rank_devices"] == [-1]:  # CPU: bit-identical
            assert np.array_equal(x, y), p.name
        else:  # on a GPU the reduction order may differ between runs: fp32 LeNet, two steps
            np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-6, err_msg=p.name)
    assert np.load(a / "logits.npy").shape == (2, 10)
    assert np.load(a / "params.npy").shape == (61706,)
    assert float(np.load(a / "loss.npy")[0]) == pytest.approx(ra["config"]["final_loss"], abs=1e-4)
    assert np.abs(np.load(a / "grads.npy")).max() > 0


def test_bench_dump_samples_large_arrays_at_fixed_positions(tmp_path):
    """An array above DUMP_MAX_ELEMS elements (ResNet-50's 25.6M parameters) is written as a sample of
    that many, at positions that depend on nothing but the array's size; bf16 comes out as float32."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_MAX_ELEMS + 12345
    pos = torch.arange(n, dtype=torch.float32)  # value = position (exact in float32 below 2^24)
    info = bench.dump_outputs(str(tmp_path), {"big": pos.reshape(1, n), "again": pos + 0.0,
                                             "small": torch.ones(3, 5, dtype=torch.bfloat16)})
    big, again, small = (np.load(tmp_path / f"{k}.npy") for k in ("big", "again", "small"))
    assert info["big"] == {"shape": [1, n], "sampled": True} and info["small"] == {"shape": [3, 5], "sampled": False}
    assert big.dtype == small.dtype == np.float32
    assert big.shape == (bench.DUMP_MAX_ELEMS,) and small.shape == (3, 5)
    assert np.array_equal(big, again) and big.min() >= 0 and big.max() < n
    assert len(np.unique(big)) > bench.DUMP_MAX_ELEMS // 2  # spread over the array, not one region
    assert 4 * (3 * bench.DUMP_MAX_ELEMS) + (1 << 20) <= 64 * 10 ** 6  # loss + logits + params + grads


def test_bench_fails_on_non_finite_loss():
    """A run whose loss ends NaN is not a measurement: bench.py exits 3 (round 6: a graphed run looked
    faster while training to NaN, profiles/r6/graph_colsum_bwd.txt)."""
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", "--model", "lenet", "--steps", "3", "--warmup", "2",
                        "--lr", "1e30"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert "not valid" in p.stderr
