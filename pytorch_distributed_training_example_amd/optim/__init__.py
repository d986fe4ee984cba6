"""Fused multi-tensor optimizers and LR schedules."""
from .fused import (FusedAdadelta, FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, FusedSGD, build_optimizer,
                    layerwise_param_groups)
from .schedules import build_scheduler, warmup_cosine

__all__ = ["FusedAdadelta", "FusedAdam", "FusedAdamW", "FusedLAMB", "FusedLARS", "FusedSGD", "build_optimizer",
           "build_scheduler", "layerwise_param_groups", "warmup_cosine"]
