"""The fused top-k / top-p sampler (csrc/kernels/sampling.hip) on the MI355X against an fp64 statement of its
semantics (ops/sampling.py lists them): kept set and probabilities, the draw, greedy and the guards, the
ticket path under hipGraph replay, the binding's refusals, and Llama.generate(sampler="fused").

Tolerance on probs: |got - ref| <= RTOL * ref + 1 / mass(P). RTOL is 4x the worst relative error of the fp32
torch form of the same formula (exp in fp32, floor to 2^-32, integer sums) against the fp64 one on these very
inputs, taken over entries of at least 2^20 quanta, where the floor no longer shows: 9.8e-7, measured on the
CPU and recorded in profiles/r27/sampler.txt. The 1 / mass(P) is one 2^-32 quantum of the fixed-point mass: an
exp that is off by an ulp may floor to the neighbouring integer, whatever the size of the entry."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = [1, 37, 4099, 32000, 131072]
DTYPES = [torch.bfloat16, torch.float32]
RTOL = 4 * 9.8e-7
TEMP, TOPK = [1.5, 0.7, 0.7, 0.7], [0, 1, 50, 50]  # no filter (flat enough that no mass floors to 0); k = 1; k = 50; k = 50 and p


def ref_row(l, T, k, p):
    """fp64 from the semantics text: (kept mask, integer masses q on the kept set, mass(K))."""
    l = torch.where(l.isnan(), torch.full_like(l, float("-inf")), l).double()
    T = torch.tensor(T, dtype=torch.float32).double()
    q = torch.floor(torch.exp((l - l.max()) / T) * 2.0 ** 32)
    keep = torch.ones_like(l, dtype=torch.bool)
    if 0 < k < l.numel():
        keep = l >= l.sort(descending=True).values[k - 1]
    mass_k = q[keep].sum()
    if p < 1:
        vals = l[keep].unique().flip(0)  # descending
        ge = torch.stack([q[keep & (l >= v)].sum() for v in vals])
        keep = keep & (l >= vals[int((ge >= p * mass_k).nonzero()[0])])
    return keep, q * keep, mass_k


@functools.lru_cache(None)
def case(V):
    """Logits [4, V] (bf16-representable, with the k-th value of rows 2 and 3 planted twice), p of row 3, and the
    reference (keep, q) per row."""
    l = (3 * torch.randn(4, V, generator=torch.Generator().manual_seed(V))).bfloat16().float()
    for b in (2, 3):
        if V > 50:
            s, o = l[b].sort(descending=True)
            l[b, o[50]] = s[49]  # the threshold value twice: both copies must be kept
    # p: the midpoint of two consecutive cumulative masses (0 included) of row 3 that lie at least 1e-3 apart
    _, qk, mass_k = ref_row(l[3], TEMP[3], TOPK[3], 1.0)
    vals = l[3][qk > 0].unique().flip(0)
    cum = torch.cat([torch.zeros(1).double(), torch.stack([qk[l[3] >= v].sum() for v in vals])]) / mass_k
    j = [i for i in range(len(cum) - 1) if cum[i + 1] - cum[i] >= 1e-3]
    assert j, "no gap of 1e-3 between consecutive cumulative masses"
    j = min(j, key=lambda i: abs(float(cum[i]) - 0.6))
    p = float((cum[j] + cum[j + 1]) / 2)
    ps = [1.0, 1.0, 1.0, p]
    refs = [ref_row(l[b], TEMP[b], TOPK[b], ps[b])[:2] for b in range(4)]
    if V > 50:
        assert int(refs[2][0].sum()) >= 51  # the planted tie is in the reference set
    return l, ps, refs


def run(V, dtype, u, probs=True):
    from pytorch_distributed_training_example_amd.ops.sampling import sample
    l, ps, _ = case(V)
    dev = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)  # noqa: E731
    return sample(l.to(DEV, dtype), dev(TEMP, torch.float32), dev(TOPK, torch.int32), dev(ps, torch.float32),
                  u=dev(u, torch.float32), return_probs=probs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_kept_set_and_probabilities(V, dtype):
    _, _, refs = case(V)
    tok, probs = run(V, dtype, [0.5] * 4)
    probs = probs.cpu().double()
    for b, (keep, q) in enumerate(refs):
        assert torch.equal(probs[b] > 0, q > 0), f"row {b}: kept set"
        want = q / q.sum()
        err = (probs[b] - want).abs()
        print(f"V={V} row {b}: kept {int(keep.sum())}, worst rel err {(err / want.clamp(min=1e-300))[q >= 2 ** 20].max():.3g}, "
              f"worst err in quanta {(err * q.sum()).max():.3g}")
        assert bool((err <= RTOL * want + 1 / q.sum()).all()), f"row {b}: probs"
        assert q[tok[b]] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_draw(V, dtype):
    """u at the midpoint of a token's fp64 CDF interval (first / middle / last kept token of probability >= 1e-3 in
    index order) gives that token; u = 0 the first kept index; u = 1 - 2^-24 the reference's inverse CDF there
    (the last kept index wherever that token weighs more than 2^-24 of the mass)."""
    _, _, refs = case(V)
    picks, us = [], []
    for keep, q in refs:
        cdf = q.cumsum(0) / q.sum()
        big = (q / q.sum() >= 1e-3).nonzero()[:, 0]
        assert len(big), "no kept token of probability 1e-3"
        t = [int(big[0]), int(big[len(big) // 2]), int(big[-1])]
        picks.append(t)
        us.append([float((cdf[i] + (cdf[i - 1] if i else 0)) / 2) for i in t])
    for n in range(3):
        tok = run(V, dtype, [u[n] for u in us], probs=False).tolist()
        assert tok == [t[n] for t in picks]
    assert run(V, dtype, [0.0] * 4, probs=False).tolist() == [int((q > 0).nonzero()[0]) for _, q in refs]
    hi = 1 - 2.0 ** -24
    want = []
    for _, q in refs:
        r = torch.floor(hi * q.sum())
        t = int((q.cumsum(0) > r).nonzero()[0])
        assert float(q[t + 1:].sum()) * 1.001 < float(q.sum() - r) < float(q[t:].sum()) * 0.999  # not at an edge
        want.append(t)
    assert want[1:] == [int((q > 0).nonzero()[-1]) for _, q in refs[1:]]
    assert run(V, dtype, [hi] * 4, probs=False).tolist() == want


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_greedy_and_guards(dtype):
    from pytorch_distributed_training_example_amd.ops._native import native
    V = 4099
    l = case(V)[0].clone()
    l[0, [77, 3001]] = 40.0  # a tied maximum: the lower index
    l[1] = float("-inf")  # nothing to draw from: token 0, zero probs
    l[2, int(l[2].argmax())] = float("nan")  # a NaN where the maximum was: the runner-up wins
    second = int(l[2].nan_to_num(nan=float("-inf")).argmax())
    l[3, 4098] = 45.0
    buf = torch.full((6, V), 7.0, device=DEV)
    par = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)  # noqa: E731
    args = (par([0.0, 1.0, 0.0, 0.0], torch.float32), par([0, 0, 5, 0], torch.int32), par([1.0, 0.9, 1.0, 0.5], torch.float32))
    tok = native().sample_logits(l.to(DEV, dtype), *args, u=par([0.3] * 4, torch.float32), probs=buf[1:5])
    assert tok.tolist() == [77, 0, second, 4098] and tok.dtype == torch.int64
    assert bool((buf[0] == 7).all()) and bool((buf[5] == 7).all())  # the rows around probs
    want = torch.zeros(4, V)
    want[0, 77] = want[2, second] = want[3, 4098] = 1.0
    assert torch.equal(buf[1:5].cpu(), want)
    with pytest.raises(RuntimeError, match="contiguous"):
        native().sample_logits(l.to(DEV, dtype)[:, ::2], *args, u=par([0.3] * 4, torch.float32))


def test_ticket_path_and_graph_replay():
    from pytorch_distributed_training_example_amd.ops.sampling import SamplerState, sample, uniforms
    l = case(4099)[0].to(DEV)
    kw = dict(temperature=1.0, top_k=40, top_p=0.95)
    st = SamplerState(seed=1234, rank=1)
    eager = [sample(l, state=st, **kw) for _ in range(3)]
    for step, tok in enumerate(eager):
        assert torch.equal(tok, sample(l, u=uniforms(st.key, step, 4).to(DEV), **kw))
    assert not (torch.equal(eager[0], eager[1]) and torch.equal(eager[1], eager[2]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample(l, state=st, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tok = sample(l, state=st, **kw)
    st.set_state(1234, 0)
    for want in eager:
        graph.replay()
        assert torch.equal(tok, want)


BAD = {
    "fp32 or bf16": lambda a: a.update(logits=a["logits"].half()),
    "outside 1..131072": lambda a: a.update(logits=torch.zeros(1, 131073, device=DEV)),
    "outside 1..65535": lambda a: a.update(logits=torch.zeros(65536, 1, device=DEV)),
    "contiguous": lambda a: a.update(logits=a["logits"].t().contiguous().t()),
    "misaligned": lambda a: a.update(logits=torch.zeros(4 * 64 + 1, device=DEV)[1:].view(4, 64)),
    "temperature must be": lambda a: a.update(temperature=a["temperature"].double()),
    "top_k must be": lambda a: a.update(top_k=a["top_k"].long()),
    "top_p must be": lambda a: a.update(top_p=a["top_p"][:3]),
    "u must be": lambda a: a.update(u=a["u"].cpu()),
    "exactly one of u and ticket": lambda a: a.update(u=None),
    "exactly one of u and ticket ": lambda a: a.update(ticket=torch.zeros(2, dtype=torch.int64, device=DEV)),
    "probs must be": lambda a: a.update(probs=torch.zeros(4, 63, device=DEV)),
    "probs must be ": lambda a: a.update(probs=torch.zeros(4, 64, device=DEV, dtype=torch.bfloat16)),
}


@pytest.mark.parametrize("msg", list(BAD))
def test_refusals(msg):
    from pytorch_distributed_training_example_amd.ops._native import native
    a = dict(logits=torch.zeros(4, 64, device=DEV), temperature=torch.ones(4, device=DEV),
             top_k=torch.zeros(4, dtype=torch.int32, device=DEV), top_p=torch.ones(4, device=DEV), u=torch.zeros(4, device=DEV))
    BAD[msg](a)
    with pytest.raises(RuntimeError, match=msg.strip()):
        native().sample_logits(**a)


def test_generate_with_the_fused_sampler():
    from pytorch_distributed_training_example_amd.models import get_model
    from pytorch_distributed_training_example_amd.models.precision import to_bf16_mixed
    torch.manual_seed(0)
    model = to_bf16_mixed(get_model("llama_tiny_gqa")).to(DEV).eval()
    idx = torch.randint(0, model.cfg.vocab_size, (3, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(3)  # noqa: E731
    tok, logits = model.generate(idx, 6, sampler="fused", return_logits=True)
    assert torch.equal(logits.gather(2, tok[..., None])[..., 0], logits.max(-1).values)  # greedy, whatever the ties
    kw = dict(temperature=0.8, top_k=20, top_p=0.9, generator=gen(), sampler="fused")
    tok, logits = model.generate(idx, 6, return_logits=True, **kw)
    for b in range(3):
        for t in range(6):
            assert bool(ref_row(logits[b, t].float().cpu(), 0.8, 20, 0.9)[0][tok[b, t]])
    kw["generator"] = gen()
    assert torch.equal(tok, model.generate(idx, 6, **kw))
    per_row = dict(kw, generator=gen(), temperature=torch.full((3,), 0.8, device=DEV),
                   top_k=torch.full((3,), 20, device=DEV), top_p=torch.full((3,), 0.9, device=DEV))
    assert torch.equal(tok, model.generate(idx, 6, **per_row))
    a = model.generate(idx, 6, temperature=0.8, top_k=20, generator=gen())
    assert torch.equal(a, model.generate(idx, 6, temperature=0.8, top_k=20, generator=gen(), sampler="torch"))
    with pytest.raises(ValueError, match="top_p needs sampler='fused'"):
        model.generate(idx, 6, temperature=0.8, top_p=0.9)
