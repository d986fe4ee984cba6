"""The e4m3 paged append and decode attention kernels (csrc/kernels/attn_paged_fp8.hip): the append bit for bit
against quantize_rows_e4m3 of what the bf16 paged append stores, the decode inside the unchanged envelope of
decode_oracle.py run on the dequantised rows, a one-hot probe bit for bit, and the binding's refusals. Pages
nobody wrote hold 0x7F bytes (an e4m3 NaN) and NaN scales throughout."""
import pytest
import torch

import decode_oracle as do
import oracle_envelope as oe

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
B = 12  # 11 slots at the seams and one inactive slot
SPLITS = [1, 2, None]


def _native():
    from pytorch_distributed_training_example_amd.ops._native import native
    return native()


def _geo(Hkv, MP, splits, G):
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_geo
    return attention_decode_geo(B, Hkv, 64 * MP, splits, G)


def _seams(H, Hkv, MP):
    """lens of the 11 active slots: either side of the 16-key, page and chunk boundaries of every split, the last key."""
    cap = 64 * MP
    s = {0, 15, 16, 63, 64, 65, cap - 1}
    for splits in SPLITS:
        C = _geo(Hkv, MP, splits, H // Hkv)[1]
        s |= {C - 1, C}
    s = sorted(x for x in s if x < cap)
    assert len(s) <= B - 1
    return s + [0] * (B - 1 - len(s))


def _pools(kq, ks, vq, vs, lens, MP, seed=0):
    """The logical caches (bytes uint8 [B-1, Hkv, cap, 64], scales [B-1, Hkv, cap]) scattered over shuffled pages; the
    inactive last slot's table row is -1. Rows past lens, unnamed pages: 0x7F bytes, NaN scales."""
    n, Hkv = kq.shape[0], kq.shape[1]
    NP = B * MP + 3
    perm = torch.randperm(NP, generator=torch.Generator().manual_seed(seed))
    table = torch.full((B, MP), -1, dtype=torch.long)
    table[:n] = perm[:n * MP].view(n, MP)
    table[:n][torch.arange(MP)[None, :] > (lens[:n].long()[:, None] >> 6)] = -1
    ok = table[:n] >= 0
    past = torch.arange(64 * MP)[None, :] > lens[:n, None]  # [n, cap]
    out = []
    for q, s in ((kq, ks), (vq, vs)):
        q = torch.where(past[:, None, :, None], torch.tensor(0x7F, dtype=torch.uint8), q)
        s = torch.where(past[:, None, :], torch.tensor(float("nan")), s)
        pool = torch.full((NP, Hkv, 64, 64), 0x7F, dtype=torch.uint8)
        sp = torch.full((NP, Hkv, 64), float("nan"))
        pool[table[:n][ok]] = q.view(n, Hkv, MP, 64, 64).permute(0, 2, 1, 3, 4)[ok]
        sp[table[:n][ok]] = s.view(n, Hkv, MP, 64).permute(0, 2, 1, 3)[ok]
        out += [pool.view(FP8).to(DEV), sp.to(DEV)]
    return out[0], out[2], out[1], out[3], table.to(torch.int32).to(DEV)


def _quantised(c):
    from pytorch_distributed_training_example_amd.ops.linear import quantize_rows_e4m3
    q, s = quantize_rows_e4m3(c.reshape(-1, 64))
    return q.view(torch.uint8).view(c.shape), s.view(c.shape[:-1])


def _run(q, pools, lens, H, Hkv, splits):
    """attention_decode_paged_fp8 on the B slots (the inactive one gets a zero query). O [B, H, 64], LSE [B, H] cpu."""
    from pytorch_distributed_training_example_amd.ops import attention as A
    kp, vp, ks, vs, table = pools
    qq = torch.zeros(B, H, 64, dtype=torch.bfloat16)
    qq[:q.shape[0]] = q
    ll = torch.zeros(B, dtype=torch.int32)
    ll[:q.shape[0]] = lens
    n0 = A.PAGED_FP8_STATS["native_calls"]
    O, lse = A.attention_decode_paged_fp8(do.pack_q(qq, Hkv).to(DEV), kp, vp, ks, vs, table, ll.to(DEV), H, Hkv, 0.125,
                                          splits, return_lse=True)
    assert A.PAGED_FP8_STATS["native_calls"] == n0 + 1
    return O.view(B, H, 64).cpu(), lse.cpu()


_CASES = {}


def _case(H, Hkv, MP, amplitude):
    """Inputs, pools and the fp64 reference on K^, V^: once per shape, shared by the splits."""
    key = (H, Hkv, MP, amplitude)
    if key not in _CASES:
        lens = _seams(H, Hkv, MP)
        q, k, v, lens_t = do.decode_inputs(B - 1, H, Hkv, 64 * MP, lens, amplitude, seed=7 * H + Hkv + MP, stale="zero")
        (kq, ks), (vq, vs) = _quantised(k), _quantised(v)
        ref, env = do.decode_oracle(q, kq.view(FP8).float() * ks[..., None], vq.view(FP8).float() * vs[..., None], lens_t)
        _CASES[key] = (q, lens_t, _pools(kq, ks, vq, vs, lens_t, MP), ref, env)
    return _CASES[key]


@pytest.mark.parametrize("amplitude", [1.0, 4.0])
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("MP", [4, 8])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2), (2, 2), (20, 1)])  # (20, 1): the second pass of G > 16
def test_envelope_at_every_seam(H, Hkv, MP, splits, amplitude):
    q, lens, pools, ref, env = _case(H, Hkv, MP, amplitude)
    O, lse = _run(q, pools, lens, H, Hkv, splits)
    name = f"H{H} Hkv{Hkv} MP{MP} geo{_geo(Hkv, MP, splits, H // Hkv)} lens{lens.tolist()} a{amplitude}"
    assert not torch.isnan(O.float()).any(), f"a stale row, a stale scale or an unused page reached O ({name})"
    assert bool((O[B - 1] == 0).all()), f"the inactive slot's O is not zero ({name})"
    worst = oe.assert_within(O[:B - 1], ref["O"], env["O"], oe.ATTN_C, oe.FLOOR, name="O " + name)
    oe.assert_abs(lse[:B - 1], ref["LSE"], oe.LSE_TOL_SMOOTH if amplitude <= 1.5 else oe.LSE_TOL_PEAKED, name="LSE " + name)
    print(f"{name}: worst O ratio {worst:.3f} of {oe.ATTN_C}")


@pytest.mark.parametrize("splits", SPLITS)
def test_equal_bits_across_launches_and_a_captured_replay(splits):
    from pytorch_distributed_training_example_amd.ops.attention import attention_decode_paged_fp8
    H, Hkv, MP = 4, 2, 8
    q, lens, (kp, vp, ks, vs, table), _, _ = _case(H, Hkv, MP, 4.0)
    qkv = do.pack_q(torch.cat([q, q[:1]]), Hkv).to(DEV)
    ll = torch.cat([lens, lens[:1] * 0]).to(DEV)
    run = lambda: attention_decode_paged_fp8(qkv, kp, vp, ks, vs, table, ll, H, Hkv, 0.125, splits, return_lse=True)
    a, la = run()
    b, lb = run()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(la, lb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c, lc = run()
    for i in range(3):
        c.fill_(7.0)
        graph.replay()
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)) and torch.equal(la, lc), f"replay {i}"


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("MP", [4, 8])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (20, 1)])
def test_onehot_probe_bit_for_bit(H, Hkv, MP, splits):
    """K bytes: dim 0 = -32 but +32 at the hot key, scale 1; q dim 0 = 32, scale 1/8: scores -128 and +128, every
    other probability is exactly 0. V bytes are integer codes e4m3 holds exactly (the key in base 8 on the even
    columns, the column on the odd ones); V scales are powers of two that differ by key and by head. O must be the
    row V^[hot] bit for bit."""
    cap, n = 64 * MP, B - 1
    lens = torch.tensor(_seams(H, Hkv, MP), dtype=torch.int32)
    C = _geo(Hkv, MP, splits, H // Hkv)[1]
    j = torch.arange(cap)
    d = torch.arange(64)
    digit = (j[:, None] // torch.pow(8, d[None, :] % 6 // 2)) % 8  # the key's base-8 digits on columns 0, 2, 4, 6, ...
    code = torch.where(d[None, :] % 2 == 1, (d[None, :] // 2 % 16).expand(cap, 64), digit).float()
    vq = code.to(FP8).view(torch.uint8)[None, None].expand(n, Hkv, cap, 64).contiguous()
    assert torch.equal(vq.view(FP8).float()[0, 0], code)
    vs = torch.pow(2.0, -(1.0 + torch.arange(Hkv)[:, None] + (j[None, :] % 3))).expand(n, Hkv, cap).contiguous()
    ks = torch.ones(n, Hkv, cap)
    q = torch.zeros(n, H, 64)
    q[:, :, 0] = 32.0
    for which in ("last", "middle"):
        hot = lens.long() if which == "last" else lens.long() // 2
        k = torch.zeros(n, Hkv, cap, 64)
        k[:, :, :, 0] = -32.0
        k[torch.arange(n), :, hot, 0] = 32.0
        pools = _pools(k.to(FP8).view(torch.uint8), ks, vq, vs, lens, MP, seed=1)
        O, _ = _run(q.to(torch.bfloat16), pools, lens, H, Hkv, splits)
        want = (code[hot][:, None, :] * vs[torch.arange(n)[:, None], torch.arange(Hkv)[None, :], hot[:, None]][..., None])
        want = want.repeat_interleave(H // Hkv, dim=1).to(torch.bfloat16)  # [n, H, 64], exact
        for b, h in (O[:n].float() != want.float()).any(-1).nonzero().tolist():
            key = int(hot[b])
            page = int(pools[4][b, key >> 6])
            pytest.fail(f"one-hot probe ({which}): slot {b} (lens {int(lens[b])}), head {h}, hot key {key} in page {page} "
                        f"(table entry {key >> 6}, chunk {key // C} of C = {C}), subtile {(key & 63) >> 4}: O = "
                        f"{O[b, h].tolist()}, V^ row = {want[b, h].tolist()}")


def _guarded(shape, dtype, fill):
    """A tensor of ``shape`` inside a flat buffer with 256 sentinel elements either side. Returns (view, buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + 512, dtype=dtype, device=DEV)
    buf.view(torch.uint8 if dtype == FP8 else dtype).fill_(fill)
    return buf[256:256 + n].view(shape), buf


@pytest.mark.parametrize("L", [0, 62])
@pytest.mark.parametrize("Tn", [1, 3, 70])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (4, 1)])
def test_append_stores_quantize_rows_of_the_bf16_rows(H, Hkv, Tn, L):
    """Two slots at lens L on a shuffled table; slot 1 has no second page (-1), so its rows at positions 64 .. 127 are
    rotated in qkv and stored nowhere."""
    from pytorch_distributed_training_example_amd.ops import rope as R
    NP, MP = 8, 3
    qkv = torch.randn(2, Tn, (H + 2 * Hkv) * 64, generator=torch.Generator().manual_seed(Tn + L)).to(torch.bfloat16).to(DEV)
    cos, sin = (t.to(DEV) for t in R.rope_table(192))
    table = torch.tensor([[5, 2, 7], [0, -1, 3]], dtype=torch.int32, device=DEV)
    lens = torch.tensor([L, L], dtype=torch.int32, device=DEV)
    kb, vb = (torch.full((NP, Hkv, 64, 64), 7.0, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    want = R.rope_append_paged_(qkv.clone(), cos, sin, H, Hkv, kb, vb, table, lens)
    (kq, kqb), (vq, vqb) = (_guarded((NP, Hkv, 64, 64), FP8, 0x7F) for _ in range(2))
    (ks, ksb), (vs, vsb) = (_guarded((NP, Hkv, 64), torch.float32, float("nan")) for _ in range(2))
    n0 = R.APPEND_PAGED_FP8_STATS["native_calls"]
    got = R.rope_append_paged_fp8_(qkv.clone(), cos, sin, H, Hkv, kq, vq, ks, vs, table, lens)
    torch.cuda.synchronize()
    assert R.APPEND_PAGED_FP8_STATS["native_calls"] == n0 + 1
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "qkv differs from the bf16 kernel's"
    stored = sum(int(table[b, (L + t) >> 6]) >= 0 for b in range(2) for t in range(Tn))  # slot 1 skips positions 64 .. 127
    for pb, pq, ps, qb, sb in ((kb, kq, ks, kqb, ksb), (vb, vq, vs, vqb, vsb)):
        written = ~(pb == 7.0).all(-1)  # [NP, Hkv, 64]: the rows the bf16 kernel stored
        assert int(written.sum()) == Hkv * stored
        q, s = _quantised(pb[written])
        assert torch.equal(pq.view(torch.uint8)[written], q), "stored bytes are not quantize_rows_e4m3's"
        assert torch.equal(ps[written], s), "stored scales are not quantize_rows_e4m3's"
        assert bool((pq.view(torch.uint8)[~written] == 0x7F).all()) and bool(ps[~written].isnan().all()), "a row nobody owns was written"
        for buf in (qb.view(torch.uint8), sb):
            guard = torch.cat([buf[:256], buf[-256:]])
            assert bool(((guard == 0x7F) if guard.dtype == torch.uint8 else guard.isnan()).all()), "a guard band was written"


@pytest.mark.parametrize("what,match", [("bf16 pools with scales", "float8_e4m3fn"), ("scale shape", "scale pools must be"),
                                        ("scale dtype", "fp32"), ("pool sizes", "equal sizes"),
                                        ("non-contiguous pool", "contiguous and 16-byte aligned"),
                                        ("misaligned pool", "contiguous and 16-byte aligned"),
                                        ("head dim", "head dim must be 64")])
def test_binding_refusals(what, match):
    H, Hkv, NP, MP = 4, 2, 6, 2
    qkv = torch.zeros(2, 1, (H + 2 * Hkv) * (32 if what == "head dim" else 64), device=DEV, dtype=torch.bfloat16)
    kp = torch.zeros(NP, Hkv, 64, 64, device=DEV, dtype=torch.uint8).view(FP8)
    vp = kp.clone()
    ks = torch.ones(NP, Hkv, 64, device=DEV)
    vs = ks.clone()
    if what == "bf16 pools with scales":
        kp = vp = torch.zeros(NP, Hkv, 64, 64, device=DEV, dtype=torch.bfloat16)
    if what == "scale shape":
        vs = torch.ones(NP, Hkv, 32, device=DEV)
    if what == "scale dtype":
        ks = ks.to(torch.bfloat16)
    if what == "pool sizes":
        vp = torch.zeros(NP + 1, Hkv, 64, 64, device=DEV, dtype=torch.uint8).view(FP8)
    if what == "non-contiguous pool":
        kp = torch.zeros(NP, Hkv, 64, 128, device=DEV, dtype=torch.uint8).view(FP8)[..., ::2]
    if what == "misaligned pool":
        kp = torch.zeros(NP * Hkv * 4096 + 16, device=DEV, dtype=torch.uint8)[8:-8].view(NP, Hkv, 64, 64).view(FP8)
    table = torch.full((2, MP), -1, device=DEV, dtype=torch.int32)
    lens = torch.zeros(2, device=DEV, dtype=torch.int32)
    out = torch.empty(2, 1, H * 64, device=DEV, dtype=torch.bfloat16)
    cos = torch.zeros(128, 32, device=DEV)
    with pytest.raises(RuntimeError, match=match):
        _native().attn_decode_paged_fp8(qkv, kp, vp, ks, vs, table, lens, H, Hkv, 0.125, 1, out)
    with pytest.raises(RuntimeError, match=match):
        _native().rope_kv_append_paged_fp8(qkv, cos, cos, H, Hkv, kp, vp, ks, vs, table, lens)
