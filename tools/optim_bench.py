"""Cost of the optimizer step alone on the real parameter sets, one GPU, one process.

Builds resnet50 and gpt2_medium as bench.py does (bf16 parameters with fp32 master copies, BatchNorm /
LayerNorm parameters as the precision policy leaves them), gives every parameter a random gradient of
its own dtype (what a DDP bucket view holds) and times ``optimizer.step()`` only:

  resnet50      sgd      FusedSGD(momentum 0.9, weight_decay 5e-5)            (what bench.py runs)
                lars     FusedLARS on layerwise_param_groups (1-D tensors: plain SGD step, no norms)
                lars_all FusedLARS with every tensor adapted (--layer-adapt-1d)
  gpt2_medium   adamw    FusedAdamW(weight_decay 0.1)                          (what bench.py runs)
                lamb     FusedLAMB on layerwise_param_groups
                lamb_all FusedLAMB with every tensor adapted

Each entry is warmed up, then ``--steps`` steps are timed with device events; the entries of a model are
alternated in one process and the order is repeated ``--rounds`` times, so drift shows. Besides the time
the table gives the bytes the step has to move (from the dtypes of each bucket), the rate that
implies, and our kernel launches per step (batches of up to 36 tensors x kernels per batch).

usage: python tools/optim_bench.py [--models resnet50,gpt2_medium] [--steps 50] [--warmup 10] [--rounds 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_TENSORS = 36  # PDT_MT_MAX_TENSORS


def entries(model_name):
    from pytorch_distributed_training_example_amd.optim import (FusedAdamW, FusedLAMB, FusedLARS, FusedSGD,
                                                                layerwise_param_groups)
    if model_name.startswith("resnet"):
        return [("sgd", lambda m: FusedSGD(m.parameters(), lr=1e-6, momentum=0.9, weight_decay=5e-5)),
                ("lars", lambda m: FusedLARS(layerwise_param_groups(m, 5e-5), lr=1e-6, momentum=0.9)),
                ("lars_all", lambda m: FusedLARS(layerwise_param_groups(m, 5e-5, skip_1d=False), lr=1e-6,
                                                 momentum=0.9))]
    return [("adamw", lambda m: FusedAdamW(m.parameters(), lr=1e-6, weight_decay=0.1)),
            ("lamb", lambda m: FusedLAMB(layerwise_param_groups(m, 0.1), lr=1e-6)),
            ("lamb_all", lambda m: FusedLAMB(layerwise_param_groups(m, 0.1, skip_1d=False), lr=1e-6))]


def traffic(opt):
    """(bytes moved per step, our kernel launches per step) from the optimizer's buckets."""
    from pytorch_distributed_training_example_amd.optim import FusedAdam, FusedLAMB, FusedLARS
    total, launches = 0, 0
    for group in opt.param_groups:
        adapt = bool(group.get("adapt", False))
        for key, ps in opt._buckets(group).items():
            n = sum(p.numel() for p in ps)
            w = 4 if key[0] == torch.float32 else 2  # the tensor the kernel updates (master or parameter)
            g = 4 if key[1] == torch.float32 else 2
            copy = 2 if key[2] else 0
            batches = -(-len(ps) // MAX_TENSORS)
            if isinstance(opt, FusedLAMB):
                # adapted: norm pass w, g, m, v in, m, v out; update w, m, v in, w (+ copy) out
                per = (w + g + 16) + (w + 8 + w + copy) if adapt else (2 * w + g + 16 + copy)
            elif isinstance(opt, FusedAdam):
                per = 2 * w + g + 16 + copy
            else:  # SGD / LARS with momentum: w, buf in and out, g in; adapted LARS reads w, g once more
                per = 2 * w + g + 8 + copy + ((w + g) if adapt and isinstance(opt, FusedLARS) else 0)
            total += per * n
            launches += batches * (3 if adapt else 1)
    return total, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet50,gpt2_medium")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU (a CPU timing says nothing about the kernels)")
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    dev = torch.device("cuda:0")
    for name in a.models.split(","):
        runs = {}
        for tag, make in entries(name):
            torch.manual_seed(1234)
            model = get_model(name).to(dev)
            if name.startswith("resnet"):
                model = model.to(memory_format=torch.channels_last)
            model = apply_precision(model, "bf16")
            gen = torch.Generator(device=dev).manual_seed(100)
            for p in model.parameters():
                p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 1e-2).to(p.dtype)
                if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
                    p.grad = p.grad.contiguous(memory_format=torch.channels_last)
            opt = make(model)
            for _ in range(a.warmup):
                opt.step()
            runs[tag] = (model, opt)
        torch.cuda.synchronize()
        nparam = sum(p.numel() for p in runs[next(iter(runs))][0].parameters())
        ntens = len(list(runs[next(iter(runs))][0].parameters()))
        print(f"# {name}: {ntens} tensors, {nparam / 1e6:.1f} M parameters, {a.steps} timed steps per entry, "
              f"order repeated {a.rounds}x", flush=True)
        best = {}
        for r in range(a.rounds):
            for tag, (model, opt) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    opt.step()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / a.steps * 1e3
                nbytes, launches = traffic(opt)
                best[tag] = min(best.get(tag, us), us)
                print(f"{name:12s} round {r} {tag:9s} {us:10.1f} us/step  {nbytes / nparam:5.1f} B/param  "
                      f"{nbytes / us / 1e3:7.1f} GB/s  {launches:3d} launches", flush=True)
        base = best[next(iter(best))]
        for tag, us in best.items():
            print(f"{name:12s} best    {tag:9s} {us:10.1f} us/step  {us / base:5.2f}x {next(iter(best))}", flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
