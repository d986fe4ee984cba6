"""Flash attention (csrc/kernels/attention.hip) against the fp64 oracle, elementwise inside the condition
envelopes of tests/oracle_envelope.py (c = 3, LSE absolute 1e-4 / 2e-4), at the tile edges of its three
MFMA kernels: 64-key tile, 128-query block, 32-query wave, 16-row subtile. Three input regimes
(tests/test_oracle_envelope_cpu.py shows why each is needed): smooth (amplitude 0.5), peaked (4) and
probe (dO zero off a few boundary rows). Every comparison prints its worst ratio; the measured ones are
kept in profiles/r9/tx_oracle_ratios.txt."""
import functools
import math

import pytest
import torch

import oracle_envelope as oe

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, DH = 2, 3, 64
SEED = 5
SENTINEL = 0x5A5A  # int16 pattern of untouched output rows (bf16 1.4977e16: finite, never a result)
PROBE = (0, 15, 16, 31, 32, 63, 64, 127, 128)


def _ops():
    from pytorch_distributed_training_example_amd.ops import attention, dropout
    from pytorch_distributed_training_example_amd.ops._native import native
    return attention, dropout, native()


@functools.lru_cache(maxsize=None)
def _inputs(T, amp, seed=0):
    """qkv [B, T, 3, H, 64] bf16 (q, k at ``amp``, v at 1) and a dense dO [B, T, H, 64]; shared, never modified."""
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + T)
    qkv = torch.randn(B, T, 3, H, DH, generator=g)
    qkv[:, :, :2] *= amp
    do = torch.randn(B, T, H, DH, generator=g)
    return qkv.bfloat16().to(DEV), do.bfloat16().to(DEV)


def _probe(do, T):
    rows = sorted({r for r in PROBE + (T - 1,) if r < T})
    z = torch.zeros_like(do)
    z[:, rows] = do[:, rows]
    return z


def _bhtd(x5, i=None):
    """[B, T, (3,) H, 64] -> [B, H, T, 64] view."""
    return (x5 if i is None else x5[:, :, i]).permute(0, 2, 1, 3)


def _kernel(qkv, do, causal, scale=None, p=0.0, ticket=None, stream=None):
    """Forward + backward through attention_qkv; every result as [B, H, T, 64] (LSE [B, H, T])."""
    A, _, _ = _ops()
    Bq, T = qkv.shape[:2]
    x = qkv.reshape(Bq, T, 3 * H * DH).clone().requires_grad_()
    y = A.attention_qkv(x, H, causal=causal, scale=scale, dropout_p=p, ticket=ticket, stream=stream)
    lse = y.grad_fn.saved_tensors[2]
    y.backward(do.reshape(Bq, T, H * DH))
    g5 = x.grad.view(Bq, T, 3, H, DH)
    return {"O": _bhtd(y.detach().view(Bq, T, H, DH)), "LSE": lse, "dQ": _bhtd(g5, 0), "dK": _bhtd(g5, 1),
            "dV": _bhtd(g5, 2)}


def _oracle(qkv, do, causal, scale=None, keep=None, keep_scale=1.0):
    return oe.attention_oracle(_bhtd(qkv, 0), _bhtd(qkv, 1), _bhtd(qkv, 2), _bhtd(do), causal=causal, scale=scale,
                               keep=keep, keep_scale=keep_scale)


def _compare(got, ref, env, lse_tol, tag):
    """All five outputs through the comparator; prints every ratio, then raises the failures together."""
    errors = []
    for name in ("O", "LSE", "dQ", "dK", "dV"):
        try:
            if name == "LSE":
                r = oe.assert_abs(got[name], ref[name], lse_tol, name=f"{tag} LSE")
            else:
                r = oe.assert_within(got[name], ref[name], env[name], oe.ATTN_C, oe.FLOOR, name=f"{tag} {name}")
            print(f"ratio {tag} {name} {r:.4g}")
        except AssertionError as e:
            errors.append(str(e))
            print(f"FAIL {e}")
    assert not errors, "\n".join(errors)


def _lse_tol(amp):
    return oe.LSE_TOL_PEAKED if amp > 1.5 else oe.LSE_TOL_SMOOTH


# ----------------------------------------------------------------------------- edge sweep
EDGE_T = (1, 31, 64, 65, 127, 128, 129, 197, 257, 385)
SWEEP = [(T, 0.5) for T in EDGE_T] + [(129, 4.0), (385, 4.0)]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T,amp", SWEEP)
def test_edge_sweep(T, amp, causal):
    qkv, do = _inputs(T, amp)
    ref, env = _oracle(qkv, do, causal)
    _compare(_kernel(qkv, do, causal), ref, env, _lse_tol(amp), f"sweep T={T} amp={amp} causal={int(causal)}")


@pytest.mark.parametrize("causal", [False, True])
def test_scale_other_than_default(causal):
    qkv, do = _inputs(197, 0.5)
    ref, env = _oracle(qkv, do, causal, scale=0.2)
    _compare(_kernel(qkv, do, causal, scale=0.2), ref, env, oe.LSE_TOL_SMOOTH, f"scale0.2 T=197 causal={int(causal)}")


# ----------------------------------------------------------------------------- probe backward
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [65, 129, 197, 385])
def test_probe_backward(T, causal):
    """dO lives on the rows next to every subtile / wave / tile / block boundary and on the last row: the
    envelopes of dK, dV shrink to those rows' weight, so one omitted (row, key) product is an O(1) error."""
    qkv, do = _inputs(T, 0.5)
    do = _probe(do, T)
    ref, env = _oracle(qkv, do, causal)
    _compare(_kernel(qkv, do, causal), ref, env, oe.LSE_TOL_SMOOTH, f"probe T={T} causal={int(causal)}")


# ----------------------------------------------------------------------------- peak placement
PEAK_T = 385
PEAK_QUERIES = (3, 45, 80, 120, 131, 170, 200, 250, 260, 300, 340, 384)  # every wave of every query block


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("where,key", [("first_tile", 2), ("last_tile", PEAK_T - 1), ("key63", 63), ("key64", 64)])
def test_peak_placement(where, key, causal):
    """One key with score ~ +30 for one query per wave (the others stay within a few units): planted in
    the first tile every later tile takes the alpha == 1 skip of the online softmax; planted in the
    last tile (a tile of one row here) the whole accumulator is rescaled by ~e^-20 at the end; keys 63
    and 64 put it on either side of the first tile boundary."""
    qkv, do = _inputs(PEAK_T, 0.5)
    qkv = qkv.clone()
    kvec = qkv[:, key, 1].float()  # [B, H, 64]
    qnew = kvec * (30.0 / (0.125 * (kvec * kvec).sum(-1, keepdim=True)))
    for qi in PEAK_QUERIES:
        qkv[:, qi, 0] = qnew.bfloat16()
    ref, env = _oracle(qkv, do, causal)
    planted = ref["LSE"][:, :, [q for q in PEAK_QUERIES if not causal or q >= key]]
    assert planted.numel() == 0 or (planted.min() > 25 and planted.max() < 35), planted
    _compare(_kernel(qkv, do, causal), ref, env, oe.LSE_TOL_PEAKED, f"peak {where} causal={int(causal)}")


# ----------------------------------------------------------------------------- padding
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [100, 197])
def test_padding_rows_are_neither_read_nor_written(T, causal):
    """q/k/v/dO are the first T rows of buffers 67 rows longer whose tail is NaN (a kernel that consumed a
    row >= T, e.g. through an unmasked tile load, would turn results NaN: the buffer-resource zero fill
    and the key >= T masks are what prevent it); o/dq/dk/dv are views of sentinel-filled buffers whose
    tail rows must keep the sentinel bit for bit."""
    _, _, C = _ops()
    qkv, do = _inputs(T, 0.5)
    TP = T + 67
    qkv_buf = torch.full((B, TP, 3, H, DH), float("nan"), device=DEV, dtype=torch.bfloat16)
    do_buf = torch.full((B, TP, H, DH), float("nan"), device=DEV, dtype=torch.bfloat16)
    qkv_buf[:, :T], do_buf[:, :T] = qkv, do
    o_buf = torch.empty(B, TP, H, DH, device=DEV, dtype=torch.bfloat16)
    g_buf = torch.empty(B, TP, 3, H, DH, device=DEV, dtype=torch.bfloat16)
    o_buf.view(torch.int16).fill_(SENTINEL)
    g_buf.view(torch.int16).fill_(SENTINEL)
    lse = torch.empty(B, H, T, device=DEV, dtype=torch.float32)
    q, k, v = (_bhtd(qkv_buf[:, :T], i) for i in range(3))
    o, dov = _bhtd(o_buf[:, :T]), _bhtd(do_buf[:, :T])
    dq, dk, dv = (_bhtd(g_buf[:, :T], i) for i in range(3))
    scale = 1.0 / math.sqrt(DH)
    C.attn_fwd_out(q, k, v, o, lse, causal, scale)
    C.attn_bwd_out(dov, q, k, v, o, lse, dq, dk, dv, causal, scale)
    got = {"O": o, "LSE": lse, "dQ": dq, "dK": dk, "dV": dv}
    for name, t in got.items():
        assert torch.isfinite(t.float()).all(), name
    ref, env = _oracle(qkv, do, causal)
    _compare(got, ref, env, oe.LSE_TOL_SMOOTH, f"padding T={T} causal={int(causal)}")
    assert bool((o_buf[:, T:].view(torch.int16) == SENTINEL).all()), "o tail overwritten"
    assert bool((g_buf[:, T:].view(torch.int16) == SENTINEL).all()), "dq/dk/dv tail overwritten"
    assert bool(torch.isnan(qkv_buf[:, T:].float()).all() and torch.isnan(do_buf[:, T:].float()).all())


# ----------------------------------------------------------------------------- causal independence
def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("j", [64, 65, 128, 150])
def test_causal_independence(j):
    """Under the causal mask query i sees keys <= i only: rows < j of O and LSE do not depend on rows >= j
    of Q, K, V, and dK, dV of keys >= j do not depend on rows < j of dO — bit for bit (the replaced
    values are large but finite: a masked product is 0 * finite = 0)."""
    T = 197
    qkv, do = _inputs(T, 0.5)
    base = _kernel(qkv, do, True)
    qkv2 = qkv.clone()
    qkv2[:, j:] = (torch.randn_like(qkv2[:, j:].float()) * 50).bfloat16()
    fwd = _kernel(qkv2, do, True)
    assert torch.equal(_bits(fwd["O"][:, :, :j]), _bits(base["O"][:, :, :j]))
    assert torch.equal(fwd["LSE"][:, :, :j], base["LSE"][:, :, :j])
    do2 = do.clone()
    do2[:, :j] = (torch.randn_like(do2[:, :j].float()) * 50).bfloat16()
    bwd = _kernel(qkv, do2, True)
    assert torch.equal(_bits(bwd["dK"][:, :, j:]), _bits(base["dK"][:, :, j:]))
    assert torch.equal(_bits(bwd["dV"][:, :, j:]), _bits(base["dV"][:, :, j:]))


@pytest.mark.parametrize("causal", [False, True])
def test_forward_backward_deterministic(causal):
    qkv, do = _inputs(385, 1.5)
    a, b = _kernel(qkv, do, causal), _kernel(qkv, do, causal)
    for name in a:
        assert torch.equal(a[name].contiguous().view(-1).view(torch.int16), b[name].contiguous().view(-1).view(torch.int16)), name


# ----------------------------------------------------------------------------- DROP instantiations
def _ticket(step):
    _, D, _ = _ops()
    st = D.DropoutState(SEED)
    st.set_state(SEED, step)
    return st.begin_forward(DEV)


@functools.lru_cache(maxsize=None)
def _keep(T, p):
    _, D, _ = _ops()
    return D.reference_mask(SEED, 21, 4, (B, H, T, T), p, "attn").to(DEV)


@pytest.mark.parametrize("probe", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [65, 197, 257])
def test_dropout_instantiations(T, causal, p, probe):
    """The DROP kernels with the CPU reference mask in the oracle: O, dQ, dK, dV carry keep and
    1 / (1 - p_eff) in value and envelope; the LSE is that of the undropped probabilities."""
    _, D, _ = _ops()
    qkv, do = _inputs(T, 0.5)
    if probe:
        do = _probe(do, T)
    ref, env = _oracle(qkv, do, causal, keep=_keep(T, p), keep_scale=D.scale_of(D.threshold(p)))
    got = _kernel(qkv, do, causal, p=p, ticket=_ticket(21), stream=4)
    _compare(got, ref, env, oe.LSE_TOL_SMOOTH, f"drop T={T} causal={int(causal)} p={p}{' probe' if probe else ''}")
