"""fp64 oracles, condition envelopes and one elementwise comparator for the transformer kernels
(attention.hip, layernorm.hip, softmax_ce.hip). A helper module imported by plain name, like
dist_utils.py; tests/test_oracle_envelope_cpu.py proves on the CPU that it is sharp.

Method. The oracle is the operation in float64 on the kernel's own (bf16 / fp32) inputs, so the
reference error is ~1e-16 and plays no part. The *envelope* of an output element is an a-priori bound
on what a correct kernel's roundings can do to it, built from the same fp64 quantities: a unit
roundoff times a sum of ABSOLUTE values of the terms the kernel adds up (a condition number times
u). ``assert_within`` then asks ``|actual - ref| <= c * (env + floor)`` for every element; ``c`` is a
small constant fixed from the analysis (below), never fitted to what the kernels give. A whole-tensor
norm appears nowhere: one wrong element fails the test. ``floor`` is FLOOR, the smallest normal number
(results below it may be flushed to zero), or 0.

Attention (P exact probabilities, u = 2^-8 the bf16 unit roundoff). The kernels round P to bf16
before P V and P^T dO, dS to bf16 before dS K and dS^T Q, every output to bf16, and form
delta = sum_j dO_j O_j from the bf16 O:
    E_O  = P |V|                      E_dV = P^T |dO|
    E_dS = |dS| + P o sum_j |dO_j O_j|   (second term: delta inherits O's rounding)
    E_dQ = scale E_dS |K|             E_dK = scale E_dS^T |Q|
Operand rounding plus output rounding bound every result by 2 u E (fp32 accumulation is 2^-16 of
that). ATTN_C = 3 is that ceiling plus 50 % for what the bound does not model: MFMA accumulation
order, the raw 2^x instruction, the LSE carried in log2 units. With dropout the same formulas hold
with P o keep * keep_scale wherever the kernels use the dropped probabilities.

LayerNorm (u = 2^-24, fp32 arithmetic on a row held in registers; n_s = D/64 + 7 counts the fp32
roundings on the path of a row sum: D/64 sequential adds per lane, 6 wave-reduction levels, one
multiply by 1/D). With xh the exact normalised row and kappa = rstd * mean_j|x_j|:
    mean:   |d mu| <= n_s u mean|x|.  A two-pass variance sees it only at second order (sum_j d_j = 0),
            so rstd carries (n_s/2 + 5) u relative (summation, the subtraction, rsqrt).
    xh:     e_xh = u ((n_s/2 + 8) |xh| + n_s kappa)      (kappa ~ 1 for centred rows, |mean|/std else)
    y:      |w| e_xh + u (2 |xh w| + |y|) + u_out |y|
    dx:     u (n_s + 8) E_dx + rstd (e_xh a2 + |xh| mean_j(|g w| e_xh)) + u_out |dx|  (+ u |dx| for + ds)
            with E_dx = rstd (|g w| + mean|g w| + |xh| a2), a2 = mean|g w xh|
    dgamma: (N + 16) u sum_r |g xh| + sum_r |g| e_xh     dbeta: (N + 16) u sum_r |g|
(N + 16) u E is the worst case of ANY summation order of N fp32 terms (+16: the products and the
fixed partial/finalize tree), so LN_C_SUM = 1; y and dx use LN_C = 2 (rsqrt's own error and FMA
contraction are not itemised). One row left out of dgamma moves an entry by |g xh| ~ 1, i.e. by
~1e5 bounds.

Cross-entropy (u = 2^-24; one 256-thread workgroup per row, n = ceil(V/256) + 32 roundings on the
path of the sum of exponentials; exp(x) is 2^(x log2 e), whose argument rounding costs u |x| relative):
    lse:      u (8 max(|x|_max, |lse|) + n)
    row loss: + 4 u (|lse| + |x_t|) + eps u (|lse| + n mean|x|)
    dlogits:  |g| (p (u (|x - lse| + 4) + tol_lse) + 4 u |p - y|) + u_out |dlogits|
CE_C = 2.
"""
from __future__ import annotations

import math

import torch

U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24
ATTN_C = 3.0
LN_C = 2.0
LN_C_SUM = 1.0
CE_C = 2.0
# LSE (fp32) absolute tolerances by input amplitude
LSE_TOL_SMOOTH = 1e-4   # amplitude <= 1.5
LSE_TOL_PEAKED = 2e-4   # amplitude 4 / planted peaks
# Absolute floor added to every envelope: the smallest normal fp32 / bf16 number. The kernels' fast
# exponentials and bf16 conversions may flush anything below it to zero.
FLOOR = 2.0 ** -126


def u_of(dtype) -> float:
    return {torch.bfloat16: U_BF16, torch.float32: U_FP32}[dtype]


# ----------------------------------------------------------------------------- comparator
def worst_ratio(actual, ref, env, floor=0.0):
    """(max over elements of |actual - ref| / (env + floor), its flat index); NaN/inf in actual count as inf."""
    a, r, e = actual.double(), ref.double(), env.double()
    err = (a - r).abs()
    err = torch.where(torch.isfinite(a), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (e + floor))  # 0/0 -> 0, x/0 -> inf
    flat = ratio.reshape(-1)
    i = int(flat.argmax())
    return float(flat[i]), i


def assert_within(actual, ref, env, c, floor=0.0, name="", record=None):
    """Elementwise ``|actual - ref| <= c * (env + floor)``. Returns the worst ratio err / (env + floor);
    on failure reports the worst index, its ratio and how many elements fail. ``record``: a dict that
    collects the worst ratio per ``name`` (the figures kept in profiles/r9/tx_oracle_ratios.txt)."""
    assert actual.shape == ref.shape == env.shape, (name, actual.shape, ref.shape, env.shape)
    ratio, i = worst_ratio(actual, ref, env, floor)
    if record is not None:
        record[name] = max(record.get(name, 0.0), ratio)
    if not ratio <= c:  # also catches NaN
        a, r, e = actual.double(), ref.double(), env.double()
        bad = ~((a - r).abs() <= c * (e + floor))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), actual.shape)) if actual.dim() else ()
        raise AssertionError(
            f"{name}: {int(bad.sum())} of {bad.numel()} elements outside {c} x envelope; worst at {idx}: "
            f"got {a.reshape(-1)[i].item():.9g}, want {r.reshape(-1)[i].item():.9g}, "
            f"envelope {e.reshape(-1)[i].item():.3g}, ratio {ratio:.3g}")
    return ratio


def assert_abs(actual, ref, tol, name="", record=None):
    """Elementwise absolute bound (the fp32 LSE). Same report as ``assert_within``."""
    return assert_within(actual, ref, torch.full_like(ref.double(), tol), 1.0, name=name, record=record)


# ----------------------------------------------------------------------------- attention
def attention_oracle(q, k, v, do=None, causal=False, scale=None, keep=None, keep_scale=1.0):
    """q, k, v, do: [..., T, Dh] (any float dtype, promoted to double). Returns (ref, env): ref has O, LSE
    (of the undropped scores) and, with ``do``, dQ, dK, dV; env the matching u * E tensors (LSE has none:
    it takes an absolute tolerance). ``keep`` [..., T, T] bool and ``keep_scale``: dropout of P."""
    Q, K, V = q.double(), k.double(), v.double()
    T, Dh = Q.shape[-2], Q.shape[-1]
    scale = 1.0 / math.sqrt(Dh) if scale is None else float(scale)
    S = (Q @ K.transpose(-1, -2)) * scale
    if causal:
        allowed = torch.ones(T, T, dtype=torch.bool, device=Q.device).tril()
        S = S.masked_fill(~allowed, float("-inf"))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    Pd = P if keep is None else P * keep.to(P.dtype) * keep_scale
    O = Pd @ V
    ref = {"O": O, "LSE": lse}
    env = {"O": U_BF16 * (Pd @ V.abs())}
    if do is not None:
        DO = do.double()
        dP = DO @ V.transpose(-1, -2)
        if keep is not None:
            dP = dP * keep.to(P.dtype) * keep_scale
        dS = P * (dP - (DO * O).sum(-1, keepdim=True))
        E_dS = dS.abs() + P * (DO * O).abs().sum(-1, keepdim=True)
        ref.update(dV=Pd.transpose(-1, -2) @ DO, dQ=scale * (dS @ K), dK=scale * (dS.transpose(-1, -2) @ Q))
        env.update(dV=U_BF16 * (Pd.transpose(-1, -2) @ DO.abs()), dQ=U_BF16 * scale * (E_dS @ K.abs()),
                   dK=U_BF16 * scale * (E_dS.transpose(-1, -2) @ Q.abs()))
    return ref, env


# ----------------------------------------------------------------------------- LayerNorm
def layernorm_oracle(x, w, b, eps, dy=None, h=None, ds=None):
    """x, dy (, h, ds): [N, D] in the storage dtype (fp32 / bf16); w, b fp32 [D]. Plain LayerNorm, or
    with ``h`` the fused (s, y) = (x + h, LN(x + h)) whose backward is dx = dh = LN'(dy) + ds.
    ``s`` is the sum as the storage dtype holds it (one correctly rounded add: compared bit for bit);
    everything after it is float64 on that s. Returns (ref, env) with y (, s) and, with ``dy``, dx, dw, db."""
    u, u_out = U_FP32, u_of(x.dtype)
    if h is not None:
        s = (x.float() + h.float()).to(x.dtype)
    else:
        s = x
    X, W, Bv = s.double(), w.double(), b.double()
    N, D = X.shape
    n_s = D / 64 + 7
    mu = X.mean(-1, keepdim=True)
    d = X - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    y = xh * W + Bv
    kappa = rstd * X.abs().mean(-1, keepdim=True)
    e_xh = u * ((n_s / 2 + 8) * xh.abs() + n_s * kappa)
    ref = {"y": y}
    env = {"y": W.abs() * e_xh + u * (2 * (xh * W).abs() + y.abs()) + u_out * y.abs()}
    if h is not None:
        ref["s"] = s
    if dy is not None:
        G = dy.double()
        gw = G * W
        s1 = gw.mean(-1, keepdim=True)
        s2 = (gw * xh).mean(-1, keepdim=True)
        a1 = gw.abs().mean(-1, keepdim=True)
        a2 = (gw * xh).abs().mean(-1, keepdim=True)
        dx = rstd * (gw - s1 - xh * s2)
        e_dx = u * (n_s + 8) * rstd * (gw.abs() + a1 + xh.abs() * a2) \
            + rstd * (e_xh * a2 + xh.abs() * (gw.abs() * e_xh).mean(-1, keepdim=True))
        if ds is not None:
            dx = dx + ds.double()
            e_dx = e_dx + u * dx.abs()
        ref.update(dx=dx, dw=(G * xh).sum(0), db=G.sum(0))
        env.update(dx=e_dx + u_out * dx.abs(),
                   dw=(N + 16) * u * (G * xh).abs().sum(0) + (G.abs() * e_xh).sum(0),
                   db=(N + 16) * u * G.abs().sum(0))
    return ref, env


# ----------------------------------------------------------------------------- cross-entropy
def cross_entropy_oracle(logits, target, smoothing=0.0, ignore_index=-100, reduction="mean", dloss=None):
    """logits [N, V] (fp32 / bf16), target int64 [N]. ``dloss``: the upstream gradient ([N] for "none", a
    scalar otherwise; default ones). Returns (ref, env) with row (per-row loss, 0 on ignored rows), loss
    (reduced as asked) and dlogits. -inf logits are allowed off the target column when smoothing == 0.
    All rows ignored under "mean" gives loss 0 / dlogits 0 here (count clamped to 1), as the op does;
    torch returns NaN there."""
    u, u_out = U_FP32, u_of(logits.dtype)
    X = logits.double()
    N, V = X.shape
    valid = target != ignore_index
    t = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(X, -1)
    xt = X.gather(1, t[:, None])[:, 0]
    Xf = torch.where(torch.isfinite(X), X, torch.zeros_like(X))
    amax = torch.maximum(Xf.abs().amax(-1), lse.abs())
    n = math.ceil(V / 256) + 32
    tol_lse = u * (8 * amax + n)
    row = lse - xt
    tol_row = tol_lse + 4 * u * (lse.abs() + xt.abs())
    if smoothing > 0:
        row = (1 - smoothing) * row + smoothing * (lse - X.mean(-1))
        tol_row = tol_row + smoothing * u * (lse.abs() + n * Xf.abs().mean(-1))
    zero = torch.zeros_like(row)
    row, tol_row = torch.where(valid, row, zero), torch.where(valid, tol_row, zero)
    count = valid.sum().clamp_min(1).double()
    if dloss is None:
        dloss = torch.ones(N if reduction == "none" else (), dtype=torch.float64, device=X.device)
    g = dloss.double()
    tol_sum = tol_row.sum() + (N + 2) * u * row.abs().sum()
    if reduction == "none":
        loss, tol_loss = row, tol_row
    elif reduction == "sum":
        loss, tol_loss, g = row.sum(), tol_sum, g.expand(N)
    else:
        loss, g = row.sum() / count, (g / count).expand(N)
        tol_loss = tol_sum / count + u * loss.abs()
    g = torch.where(valid, g, zero)
    p = torch.exp(X - lse[:, None])
    Y = torch.full_like(X, smoothing / V)
    Y.scatter_add_(1, t[:, None], torch.full_like(X[:, :1], 1 - smoothing))
    dl = (p - Y) * g[:, None]
    dist = torch.where(p > 0, (X - lse[:, None]).abs(), torch.zeros_like(X))
    e_dl = g.abs()[:, None] * (p * (u * (dist + 4) + tol_lse[:, None]) + 4 * u * (p - Y).abs()) + u_out * dl.abs()
    return {"row": row, "loss": loss, "dlogits": dl, "lse": lse}, {"row": tol_row, "loss": tol_loss, "dlogits": e_dl}
