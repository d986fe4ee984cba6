"""Whole-step cost of dropout on the transformer workloads, one GPU.

Builds gpt2_medium and vit_b16 as bench.py does (same per-GPU batch, sequence / image size, bf16
precision, fused AdamW, our DDP wrapper, measured GEMM table) in three configurations:
  p0      dropout = 0                         (what bench.py measures)
  fused   dropout = 0.1, counter-generated masks inside our kernels (PDT_DROPOUT_FUSED=1)
  aten    dropout = 0.1 from F.dropout + SDPA's dropout           (PDT_DROPOUT_FUSED=0)
and times ``--steps`` steps of each with device events after a warm-up. The three are alternated
in one process (p0, fused, aten) and the order is repeated ``--rounds`` times, so drift shows.

usage: python tools/dropout_bench.py [--models gpt2_medium,vit_b16] [--steps 20] [--rounds 2]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (WORKLOADS, setup: the benchmark's own environment and process group)
from pytorch_distributed_training_example_amd.config import SW  # noqa: E402

CONFIGS = [("p0", 0.0, True), ("fused", 0.1, True), ("aten", 0.1, False)]


def build(model_name, p, ctx):
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import apply_precision
    from pytorch_distributed_training_example_amd.optim import FusedAdamW
    from pytorch_distributed_training_example_amd.parallel import DistributedDataParallel
    torch.manual_seed(1234)
    model = apply_precision(get_model(model_name, dropout=p).to(ctx.device), "bf16")
    ddp = DistributedDataParallel(model, bucket_cap_mb="auto", broadcast_buffers=False, gradient_as_bucket_view=True,
                                  reduce_single_rank=True)
    return ddp, FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gpt2_medium,vit_b16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    from pytorch_distributed_training_example_amd.ops.cross_entropy import cross_entropy
    ctx = None
    for name in a.models.split(","):
        args = bench.parse(["--model", name])
        if ctx is None:
            ctx = bench.setup(args)
        B = bench.WORKLOADS[name][2]
        g = torch.Generator(device=ctx.device).manual_seed(100)
        if name.startswith("gpt"):
            x = torch.randint(0, 50257, (B, args.seq_len), device=ctx.device, generator=g)
            y = torch.randint(0, 50257, (B, args.seq_len), device=ctx.device, generator=g)
        else:
            x = torch.randn(B, 3, args.image_size, args.image_size, device=ctx.device, generator=g).bfloat16()
            y = torch.randint(0, 1000, (B,), device=ctx.device, generator=g)
        runs = {}
        for tag, p, fused in CONFIGS:
            ddp, opt = build(name, p, ctx)

            def step(ddp=ddp, opt=opt, fused=fused):
                SW.dropout_fused = fused
                opt.zero_grad(set_to_none=True)
                out = ddp(x)
                loss = cross_entropy(out.reshape(-1, out.shape[-1]), y.reshape(-1))
                loss.backward()
                opt.step()
                return loss
            for _ in range(a.warmup):
                step()
            runs[tag] = step
        torch.cuda.synchronize()
        unit = B * (args.seq_len if name.startswith("gpt") else 1)
        print(f"# {name}: batch {B}, {a.steps} timed steps per entry, order repeated {a.rounds}x", flush=True)
        for r in range(a.rounds):
            for tag, _, _ in CONFIGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    loss = runs[tag]()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.steps
                print(f"{name:12s} round {r} {tag:6s} {ms:9.3f} ms/step {unit / ms * 1e3:12.0f} "
                      f"{bench.WORKLOADS[name][1]}  loss {float(loss):.4f}", flush=True)
        del runs
        torch.cuda.empty_cache()
    SW.reload()
    from pytorch_distributed_training_example_amd.parallel import launcher
    launcher.destroy()


if __name__ == "__main__":
    main()
