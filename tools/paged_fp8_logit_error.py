"""Worst logit error of Llama generation on the e4m3 paged cache over the bf16 paged cache's, both against the fp32
full forward, on the PyTorch reference path with CPU tensors: the figure tests/test_llama_paged_fp8_gpu.py takes its
bound R from (twice the largest ratio printed here). Inputs as in that test: bf16-valued weights of seed 0, tokens
of seed 1, prompts of LENS right-padded to 70 tokens, 8 teacher-forced decode steps. No GPU is used.

Usage: python tools/paged_fp8_logit_error.py
"""
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_distributed_training_example_amd.models import get_model  # noqa: E402
from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed  # noqa: E402

LENS, STEPS = (5, 60, 70), 8


def run(model, idx, kv_dtype):
    cache = model.new_paged_cache(3, 9, kv_dtype=kv_dtype)
    for s in range(3):
        cache.admit(s)
    cache.reserve(70)
    out = [model.prefill(idx[:3, :70], cache, prompt_lens=LENS)]
    for i in range(STEPS):
        cache.reserve(1)
        out.append(model.decode_step(torch.stack([idx[s, LENS[s] + i] for s in range(3)]), cache))
    return torch.stack(out, 1).float()


def main():
    for name in ("llama_tiny", "llama_tiny_gqa"):
        torch.manual_seed(0)
        model = to_bf16_mixed(get_model(name, block_size=192)).eval()
        idx = torch.randint(0, model.cfg.vocab_size, (4, 96), generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            want = copy.deepcopy(model).float()(idx)
            err = {}
            for kv in (None, "fp8"):
                got = run(model, idx, kv)
                err[kv] = max((got[b] - want[b, LENS[b] - 1:LENS[b] + STEPS]).abs().max().item() for b in range(3))
        print(f"{name}: e_b = {err[None]:.4g} (bf16 paged cache), e_q = {err['fp8']:.4g} (e4m3 paged cache), "
              f"e_q / e_b = {err['fp8'] / err[None]:.3f}")


if __name__ == "__main__":
    main()
