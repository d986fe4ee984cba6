"""Temperature / top-k / top-p token sampling with per-row parameters: one HIP launch per call on the GPU
(csrc/kernels/sampling.hip), the same semantics in plain torch on the CPU.

Semantics, per row of ``logits [B, V]`` (fp32 or bf16, ``V <= 131072``):
  1. NaN counts as -inf, +inf as the dtype's largest finite value. If no logit is above -inf the token is 0
     and the ``probs`` row is zero.
  2. ``M`` = the row maximum. ``temperature == 0``: the lowest index with ``l == M`` (``probs``: one-hot).
  3. Top-k acts on the raw logits: ``t_k`` = the k-th largest value counted with multiplicity,
     ``K = {l >= t_k}``; ties at the threshold are all kept. ``k == 0`` or ``k >= V`` keeps everything.
  4. Weights ``e = exp((l - M) / T)`` in fp32, masses ``q = floor(e * 2^32)`` as 64-bit integers: every sum
     of masses is an integer sum, so the GPU result does not depend on the order of its additions.
  5. Top-p: ``t_p`` = the largest value ``t`` with ``mass{K, l >= t} >= p * mass(K)`` (the two sides compared
     as fp64), ``P = {i in K : l >= t_p}``; ties again kept whole.
  6. ``r = floor(u * mass(P))`` (fp64); the token is the lowest index of ``P`` whose inclusive prefix mass in
     index order exceeds ``r``.
  7. ``probs = q / mass(P)`` on ``P`` (fp64 quotient, stored fp32), 0 elsewhere.
Device-side parameter values are clamped, not read: ``k < 0`` is 0, ``p`` goes into (0, 1] (NaN: the smallest).

The uniform ``u [B]`` is given, or drawn from a ``SamplerState``: a device ``(key, step)`` counter like
``DropoutState`` (the same ``dropout_begin`` kernel hands out the ticket and advances the step, also under
hipGraph replay), with ``u[b] = (philox4x32_10((b, 0, stream, step), key)[0] >> 8) * 2^-24``. The CPU path
computes the same ``u`` with ``ops/dropout.py:philox4x32_10``; its ``exp`` is torch's, so CPU and GPU agree
except where a mass comparison is within an ulp of a tie.

Not here: min-p, typical sampling, repetition / presence penalties, logit bias, beam search.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._native import native
from .dropout import DropoutState, philox4x32_10, ticket_values

MAX_VOCAB = 131072
_TINY = 1.17549435e-38  # the smallest p the kernel clamps to


class SamplerState(DropoutState):
    """Host seed + device ``(key, step)`` counter of the sampler's draws; ``ticket`` advances the step."""

    def ticket(self, device) -> torch.Tensor:
        st = self._device_state(device)
        if st.is_cuda:
            return native().dropout_begin(st)
        t = st.clone()
        st[1] += 1
        return t


def uniforms(key: int, step: int, rows: int, stream: int = 0) -> torch.Tensor:
    """The fp32 uniforms in [0, 1) that rows 0..rows-1 draw from ticket ``(key, step)``."""
    w0 = philox4x32_10((np.arange(rows, dtype=np.uint32), np.uint32(0), np.uint32(stream & 0xFFFFFFFF),
                        np.uint32(step & 0xFFFFFFFF)), (key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF))[0]
    return torch.from_numpy((w0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))


_PARAMS: dict = {}


def _param(name: str, value, rows: int, dtype, device, lo_ok) -> torch.Tensor:
    """A scalar (validated on the host, broadcast into a cached device tensor) or a [B] tensor as ``dtype``."""
    if isinstance(value, torch.Tensor):
        if value.shape != (rows,):
            raise ValueError(f"sample: {name} must be a scalar or a [{rows}] tensor, got shape {tuple(value.shape)}")
        if value.device != device:
            raise ValueError(f"sample: {name} is on {value.device}, the logits on {device}")
        return value.to(dtype).contiguous()
    if not lo_ok(value):
        raise ValueError(f"sample: {name} = {value!r} is out of range (temperature >= 0, top_k >= 1, 0 < top_p <= 1)")
    key = (name, value, rows, device)
    t = _PARAMS.get(key)
    if t is None:
        t = _PARAMS[key] = torch.full((rows,), value, dtype=dtype, device=device)
    return t


def sample_cpu(logits, temperature, top_k, top_p, u, return_probs=False):
    """The semantics above in torch, for [B] parameter tensors: tokens int64 [B] (and probs fp32 [B, V])."""
    B, V = logits.shape
    ninf = float("-inf")
    l = logits.float()
    l = torch.where(l.isnan(), torch.full_like(l, ninf), l).clamp(max=torch.finfo(logits.dtype).max) + 0.0
    M = l.max(-1, keepdim=True).values
    dead, greedy = ~(M[:, 0] > ninf), ~(temperature > 0)
    T = torch.where(greedy, torch.ones_like(temperature), temperature)[:, None]
    e = torch.where(l > ninf, torch.exp((l - M) / T), torch.zeros_like(l))
    q = (e.double() * 4294967296.0).floor().long()
    # top-k: a prefix of the descending order, cut after the k-th value's ties
    s, order = l.sort(-1, descending=True)
    k = top_k.long().clamp(min=0)
    t_k = torch.where(((k > 0) & (k < V))[:, None], s.gather(1, (k.clamp(1, V) - 1)[:, None]), torch.full_like(M, ninf))
    keep = l >= t_k
    # top-p: mass{l >= s_j} is the running mass at the end of s_j's tie group
    cum = (q * keep).gather(1, order).cumsum(-1)
    last = torch.ones_like(keep)
    last[:, :-1] = s[:, :-1] != s[:, 1:]
    big = torch.iinfo(torch.int64).max
    ge = torch.where(last, cum, torch.full_like(cum, big)).flip(-1).cummin(-1).values.flip(-1)
    p = torch.where(top_p > 0, top_p, torch.full_like(top_p, _TINY)).clamp(max=1.0)
    need = p.double()[:, None] * cum[:, -1:].double()
    t_p = s.gather(1, (ge.double() >= need).int().argmax(-1, keepdim=True))
    keep = keep & ((l >= t_p) | (p >= 1.0)[:, None])
    qp = q * keep
    mass = qp.sum(-1)
    r = (u.double().clamp(0.0, 1.0) * mass.double()).floor().long().clamp(max=mass - 1)
    tok = (qp.cumsum(-1) > r[:, None]).int().argmax(-1)
    first_max = (l == M).int().argmax(-1)
    tok = torch.where(dead, torch.zeros_like(tok), torch.where(greedy, first_max, tok))
    if not return_probs:
        return tok
    probs = (qp.double() / mass.clamp(min=1).double()[:, None]).float()
    onehot = torch.zeros_like(probs).scatter_(1, first_max[:, None], 1.0)
    probs = torch.where(greedy[:, None], onehot, probs)
    return tok, torch.where(dead[:, None], torch.zeros_like(probs), probs)


def sample(logits: torch.Tensor, temperature=1.0, top_k=None, top_p=None, state: Optional[SamplerState] = None,
           u: Optional[torch.Tensor] = None, return_probs: bool = False):
    """One token id per row of ``logits [B, V]`` (int64 [B]); with ``return_probs`` also the distribution
    ``[B, V]`` fp32 each was drawn from. ``temperature`` / ``top_k`` / ``top_p``: scalars (``None`` = off) or
    ``[B]`` tensors on the logits' device. Exactly one of ``state`` (a ``SamplerState``) and ``u`` (fp32 [B]
    uniforms in [0, 1)). GPU tensors take the HIP kernel, and a call with tensors or cached scalars launches
    without a host read, so it can be captured in a hipGraph; CPU tensors take ``sample_cpu``."""
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"sample: logits must be fp32 / bf16 [B, V], got {logits.dtype} {tuple(logits.shape)}")
    B, V = logits.shape
    if not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"sample: V = {V} outside 1..{MAX_VOCAB}")
    if (state is None) == (u is None):
        raise ValueError("sample: exactly one of state and u must be given")
    dev = logits.device
    t = _param("temperature", temperature, B, torch.float32, dev, lambda v: v >= 0)
    k = _param("top_k", 0 if top_k is None else top_k, B, torch.int32, dev, lambda v: top_k is None or v >= 1)
    p = _param("top_p", 1.0 if top_p is None else top_p, B, torch.float32, dev, lambda v: 0 < v <= 1)
    if logits.is_cuda:
        probs = torch.empty(B, V, dtype=torch.float32, device=dev) if return_probs else None
        tok = native().sample_logits(logits, t, k, p, u=u, ticket=None if state is None else state.ticket(dev),
                                     stream=0, probs=probs)
        return (tok, probs) if return_probs else tok
    if u is None:
        u = uniforms(*ticket_values(state.ticket(dev)), B)
    return sample_cpu(logits, t, k, p, u.float(), return_probs)
