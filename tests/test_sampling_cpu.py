"""ops/sampling.py without a GPU: the CPU implementation against the usual sort-and-cumsum formulation of top-k /
top-p, the Philox uniform against philox.h's known answer, the scalar checks, and the two CLI flags."""
import pytest
import torch

from pytorch_distributed_training_example_amd import cli
from pytorch_distributed_training_example_amd.ops.sampling import SamplerState, sample, uniforms


def hf_filter(l, T, k, p):
    """fp64, the formulation of the common libraries: top-k by the k-th value, then remove the ascending tail whose
    cumulative probability is at most 1 - p. Returns the renormalised probabilities."""
    z = l.double() / T
    if k:
        z = z.masked_fill(z < z.topk(k).values[-1], float("-inf"))
    s, o = z.sort()
    drop = torch.softmax(s, 0).cumsum(0) <= 1 - p
    z[o[drop]] = float("-inf")
    return torch.softmax(z, 0)


@pytest.mark.parametrize("V,k", [(37, None), (1000, None), (1000, 20)])
def test_cpu_sampler_against_sort_and_cumsum(V, k):
    l = 3 * torch.randn(2, V, generator=torch.Generator().manual_seed(V))
    T = 0.8
    ps = []
    for b in range(2):  # p in the middle of a gap of at least 1e-3 between consecutive cumulative masses
        cum = hf_filter(l[b], T, k, 1.0).sort(descending=True).values.cumsum(0)
        j = [i for i in range(len(cum) - 1) if cum[i + 1] - cum[i] >= 1e-3 and cum[i] > 0.3]
        assert j
        ps.append(float((cum[j[0]] + cum[j[0] + 1]) / 2))
    want = torch.stack([hf_filter(l[b], T, k, ps[b]) for b in range(2)])
    u = torch.tensor([0.25, 0.75])
    tok, probs = sample(l, T, k, torch.tensor(ps), u=u, return_probs=True)
    assert torch.equal(probs > 0, want > 0)
    assert torch.allclose(probs.double(), want, rtol=1e-5, atol=2.0 ** -31)
    cdf = want.cumsum(1)
    assert tok.tolist() == [int((cdf[b] > u[b]).nonzero()[0]) for b in range(2)]
    # greedy rows and scalar parameters; a draw from a state is the draw from its uniforms
    assert torch.equal(sample(l, 0.0, u=u), l.argmax(-1))
    st = SamplerState(seed=7)
    a = sample(l, T, k, ps[0], state=st)
    assert torch.equal(a, sample(l, T, k, ps[0], u=uniforms(7, 0, 2))) and st.get_state()["step"] == 1


def test_philox_uniform_known_answer():
    # philox.h: counter (0, 0, 0, 0), key (0, 0) -> 6627e8d5 ...: row 0 of ticket (0, 0), stream 0
    assert float(uniforms(0, 0, 3)[0]) == (0x6627E8D5 >> 8) * 2.0 ** -24
    assert len(set(uniforms(0, 0, 3).tolist() + uniforms(0, 1, 3).tolist() + uniforms(1, 0, 3).tolist())) == 9


@pytest.mark.parametrize("kw", [dict(temperature=-0.1), dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5), dict(u=None),
                                dict(state=SamplerState()), dict(temperature=torch.ones(3))])
def test_scalar_validation(kw):
    with pytest.raises(ValueError):
        sample(torch.zeros(2, 8), **{"u": torch.zeros(2), **kw})


@pytest.mark.parametrize("flags,err", [
    (["--sample-sampler", "fused", "--sample-top-p", "0.9"], None),
    (["--sample-sampler", "fused"], None),
    (["--sample-top-p", "0.9"], "--sample-sampler fused"),
    (["--sample-sampler", "fused", "--sample-top-p", "0"], "(0, 1]"),
    (["--sample-sampler", "fused", "--sample-top-p", "1.01"], "(0, 1]"),
])
def test_cli_flags(flags, err):
    args = cli.build_parser().parse_args(["--model", "llama_tiny", "--sample-tokens", "4", "--sample-temperature", "0.8"] + flags)
    msg = cli.sample_args_error(args)
    assert msg is None if err is None else err in msg
    assert cli.build_parser().parse_args([]).sample_sampler == "torch"
