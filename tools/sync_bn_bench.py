"""SyncBatchNorm's split path at W = 1 against the local BatchNorm: forward + backward of one BatchNorm + ReLU at
[32, 256, 56, 56] bf16 channels_last (ResNet-50 layer 1), HIP-event time, median of RUNS alternating runs.
What the difference buys nothing for at W = 1 is what it costs: the zero-filled exchange buffers, the two
merge launches, and reduce / finalize / apply as separate entry points (BASELINE.md "SyncBatchNorm").
Also counts how many channels' invstd differ in the last bit between the two paths (mean never does)."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from pytorch_distributed_training_example_amd.ops._native import native  # noqa: E402
from pytorch_distributed_training_example_amd.ops.batchnorm import batch_norm_act  # noqa: E402
from pytorch_distributed_training_example_amd.ops.sync_batchnorm import sync_batch_norm_act  # noqa: E402

N, C, H, W = 32, 256, 56, 56
WARMUP, RUNS = 10, 30


def main():
    torch.manual_seed(0)
    x = (torch.randn(N, C, H, W, device="cuda") * 2 + 0.5).bfloat16().contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    w = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(C, device="cuda").requires_grad_(True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    g = torch.randn(N, C, H, W, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)

    def local():
        batch_norm_act(x, None, w, b, rm, rv, True, 0.1, 1e-5, True).backward(g)

    def sync():
        sync_batch_norm_act(x, None, w, b, rm, rv, True, 0.1, 1e-5, True, None, _force_sync=True).backward(g)

    def once(fn):
        x.grad = w.grad = b.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    for _ in range(WARMUP):
        once(local), once(sync)
    times = {"local": [], "sync": []}
    for _ in range(RUNS):  # alternating: both see the same neighbours on the machine
        times["local"].append(once(local))
        times["sync"].append(once(sync))
    for k, v in times.items():
        v.sort()
        print(f"{k:>5}: median {statistics.median(v):8.1f} us  (min {v[0]:.1f}, max {v[-1]:.1f}, {RUNS} runs)")
    _, mean, invstd = sync_batch_norm_act(x.detach(), None, w, b, rm.clone(), rv.clone(), True, 0.1, 1e-5, True, None,
                                          _force_sync=True, _return_stats=True)
    _, _, lmean, linvstd = native().bn_fwd_train(x.detach(), None, w, b, rm.clone(), rv.clone(), 0.1, 1e-5, True)
    print(f"channels whose mean differs from the local path: {(mean != lmean).sum().item()} / {C}; "
          f"invstd: {(invstd != linvstd).sum().item()} / {C}")


if __name__ == "__main__":
    main()
