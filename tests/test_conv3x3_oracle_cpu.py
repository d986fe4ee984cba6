"""tests/conv_oracle.py is sharp, shown without a GPU:
  * its reference equals float64 ``F.conv2d`` and autograd's gradients at both strides and at odd sizes;
  * a torch emulation of a correct kernel (``Emu``: fp32 accumulation per 32-channel chunk and tap, per weight-
    gradient tile and split, the shifted statistics of tile_stats.h, one bf16 rounding at the store) passes every
    check of every case of tests/test_conv3x3_oracle_gpu.py, whose test functions run here against it;
  * ten planted faults each fail the exact check and each fail the envelope check, and the single-pixel ones pass
    the criterion the earlier tests used (||a - b|| / ||b|| < 1e-2): the gap the oracle closes;
  * Python replicas of the host halo bounds (conv3x3.hip halo_rows_bound, conv3x3_wgrad.hip halo_rows) are never
    below what the tiles need by the kernels' own formulas, for H, W in 1..70 at both strides.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co
import test_conv3x3_oracle_gpu as tg

CL = torch.channels_last


# ----------------------------------------------------------------------------- the emulated extension
def _unpack(mask, shape):
    return ((mask[:, None].to(torch.int32) >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(shape)


class Emu:
    """The bindings tests/test_conv3x3_oracle_gpu.py calls, emulated in torch on the CPU. ``fault`` plants one
    of FAULTS."""

    def __init__(self, fault=None):
        self.opt, self.tune, self.fault = 41, (0, 0), fault

    # host-only queries and switches
    def conv3x3_opt(self, v):
        old, self.opt = self.opt, (41 if v < 0 else v)
        return old

    def conv3x3_wgrad_tune(self, target_wgs, co_tile):
        self.tune = (target_wgs if target_wgs >= 0 else self.tune[0], co_tile if co_tile >= 0 else self.tune[1])

    def conv3x3s1_variant(self, N, H, W, Ci, Co):
        if Ci % 32 or Co % 64 or min(N, H, W) < 1:
            raise RuntimeError("conv3x3s1_variant: shape not taken by conv3x3s1_fwd")
        return co.s1_variant(N, H, W, Ci, Co, self.opt)

    def conv3x3_wgrad_geo(self, N, H, W, Ci, Co, stride):
        return co.wgrad_geo(N, H, W, Ci, Co, stride, *self.tune)

    # forward (and the stride-1 data gradient: the same launch on flipped weights)
    def _fwd_acc(self, x, w, stride):
        N, H, W, Ci = x.shape
        Ho, Wo = co.out_size(H, stride), co.out_size(W, stride)
        x, w = x.float(), w.float()
        if self.fault == "s2_odd_edge" and stride == 2 and H % 2:   # the last row of an odd input taken for padding
            x = x.clone()
            x[:, H - 1] = 0
        xp = co.pad(x)
        acc = torch.zeros(N, Ho, Wo, w.shape[0])
        for c0 in range(0, Ci, co.CHUNK):
            for t in range(9):
                acc += co.shift(xp, t, Ho, Wo, stride)[..., c0:c0 + co.CHUNK] @ w[:, t, c0:c0 + co.CHUNK].t()
        if self.fault == "pad_corner":      # (0, 1, 0) tap (1, 0): the pad column reads the previous row's last pixel
            acc[0, 1, 0] += x[0, 0, W - 1] @ w[:, 3].t()
        if self.fault == "tap_dropped":     # the centre tap of the last row of tile 0
            m = min(co.BM, N * H * W) - 1
            acc[m // (H * W), m // W % H, m % W] -= x[m // (H * W), m // W % H, m % W] @ w[:, 4].t()
        if self.fault == "wrong_image":     # row 0 of image 1 takes its kh = 0 halo row from image 0's last row
            row = F.pad(x[0, H - 1], (0, 0, 1, 1))
            for kw in range(3):
                acc[1, 0] += row[kw:kw + W] @ w[:, kw].t()
        return acc

    def _fwd(self, x4, w4, stride):
        acc = self._fwd_acc(x4.permute(0, 2, 3, 1), co.from_w_nchw(w4), stride)
        return co.nchw(acc.to(torch.bfloat16))

    def conv3x3s1_fwd(self, x4, w4):
        return self._fwd(x4, w4, 1)

    def conv3x3_flip(self, w4):
        wf = co.flip_ref(w4).contiguous(memory_format=CL)
        if self.fault == "flip_tap":        # tap 1 takes t for 8 - t
            wf[:, :, 0, 1] = w4[:, :, 0, 1].t()
        return wf

    def _stats(self, y, rows):
        """tile_stats.h rs8_*: S = sum (y - K), Q = sum (y - K)^2 in fp32, K the tile's first row; stored
        n K + S and max(Q - S^2 / n, 0)."""
        C = y.shape[-1]
        yt, n = co.tiles_2d(y.float().reshape(-1, C), rows)
        n = n.float()
        nv = n.clone()
        if self.fault == "stats_last_row":  # the last tile's last valid row left out
            nv[-1] -= 1
        valid = (torch.arange(rows)[None, :] < nv[:, None])[:, :, None]
        K = yt[:, 0]
        d = torch.where(valid, yt - K[:, None], torch.zeros(()))
        S, Q = d.sum(1), (d * d).sum(1)
        return torch.stack([n[:, None] * K + S, (Q - S * S / n[:, None]).clamp_min(0)])

    def conv3x3s1_fwd_stats(self, x4, w4):
        N, Ci, H, W = x4.shape
        v = self.conv3x3s1_variant(N, H, W, Ci, w4.shape[0])
        y = self._fwd(x4, w4, 1)
        if v.startswith("tap"):
            return [y]
        return [y, self._stats(y.permute(0, 2, 3, 1), co.BM_WSR if v == "wsr" else co.BM)]

    @staticmethod
    def _bn_sums(dz, xc, rows):
        """[2, T, C] fp32 of a [M, C] gradient and centred BatchNorm input."""
        return torch.stack([co.tiles_2d(v, rows)[0].sum(1) for v in (dz, dz * xc)])

    def conv3x3s1_fwd_bnbwd(self, x4, w4, bn_x, bn_mask, bn_mean):
        N, Ci, H, W = x4.shape
        Co = w4.shape[0]
        v = self.conv3x3s1_variant(N, H, W, Ci, Co)
        y = self._fwd(x4, w4, 1)
        if not (v.startswith("halo") or (v == "wsr" and self.opt & 128)):
            return [y]
        yf = y.permute(0, 2, 3, 1).float().reshape(-1, Co)
        keep = _unpack(bn_mask, yf.shape).float() if bn_mask is not None else torch.ones_like(yf)
        xc = bn_x.permute(0, 2, 3, 1).float().reshape(-1, Co) - bn_mean
        return [y, self._bn_sums(yf * keep, xc, co.BM_WSR if v == "wsr" else co.BM)]

    # stride 2
    def conv3x3s2_fwd(self, x4, w4, stats):
        y = self._fwd(x4, w4, 2)
        return [y, self._stats(y.permute(0, 2, 3, 1), co.BM)] if stats else [y]

    def conv3x3s2_dgrad(self, dy4, wf, H, W, bn_x=None, bn_mask=None, bn_mean=None):
        dy = dy4.permute(0, 2, 3, 1).float()
        w = co.from_w_nchw(co.flip_ref(wf)).float()     # the flip is an involution
        N, Ho, Wo, Co = dy.shape
        Ci = w.shape[2]
        dxp = torch.zeros(N, H + 2, W + 2, Ci)
        for c0 in range(0, Co, co.CHUNK):
            for t in range(9):
                co.shift(dxp, t, Ho, Wo, 2).add_(dy[..., c0:c0 + co.CHUNK] @ w[c0:c0 + co.CHUNK, t])
        acc = dxp[:, 1:-1, 1:-1].contiguous()
        if self.fault == "s2_parity":       # phase (0, 0) takes tap (0, 1) for its only tap (1, 1)
            acc[:, 0::2, 0::2] = dy @ w[:, 1]
        if self.fault == "past_m" and W % 2:  # phase (0, 1)'s column past the image stored: it lands on the next pixel
            acc[0, 1, 0] = dy[0, 0, Wo - 1] @ w[:, 5]
        dx = acc.to(torch.bfloat16)
        if bn_x is None:
            return [co.nchw(dx)]
        keep = _unpack(bn_mask, dx.shape).float() if bn_mask is not None else torch.ones(dx.shape)
        dz, xc = dx.float() * keep, bn_x.permute(0, 2, 3, 1).float() - bn_mean
        parts = []
        for py in (0, 1):       # partial rows (2 py + px) tiles_per_phase + tile, tiles over the full phase grid
            for px in (0, 1):
                g = torch.zeros(2, N, Ho, Wo, Ci)
                a, b = dz[:, py::2, px::2], (dz * xc)[:, py::2, px::2]
                g[0, :, :a.shape[1], :a.shape[2]], g[1, :, :a.shape[1], :a.shape[2]] = a, b
                parts.append(torch.stack([co.tiles_2d(g[i].reshape(-1, Ci), co.BM)[0].sum(1) for i in (0, 1)]))
        return [co.nchw(dx), torch.cat(parts, 1)]

    # weight gradient: fp32 per split over its tiles, then the splits summed in order
    def _wgrad(self, x4, dy4, stride):
        x, dy = x4.permute(0, 2, 3, 1).float(), dy4.permute(0, 2, 3, 1).float()
        N, H, W, Ci = x.shape
        _, Ho, Wo, Co = dy.shape
        geo = self.conv3x3_wgrad_geo(N, H, W, Ci, Co, stride)
        if geo is None:
            return None
        R, ntiles, tps, nsplit, _ = geo
        xp = co.pad(x)
        xs = [co.shift(xp, t, Ho, Wo, stride).reshape(N * Ho, Wo, Ci) for t in range(9)]
        g = dy.reshape(N * Ho, Wo, Co)
        tiles = co.wgrad_tiles(N, Ho, R)
        assert len(tiles) == ntiles
        ws = torch.zeros(nsplit, Co, 9, Ci)
        for s in range(nsplit):
            mine = list(range(s * tps, min((s + 1) * tps, ntiles)))
            if self.fault == "tile_missing" and s == nsplit - 1:
                mine = mine[:-1]
            for tl in mine:
                g0, g1 = tiles[tl]
                rows = list(range(g0, g1))
                if self.fault == "row_twice" and tl == ntiles // 2:
                    rows.append(g0)
                gt = g[rows].reshape(-1, Co).t()
                for t in range(9):
                    ws[s, :, t] += gt @ xs[t][rows].reshape(-1, Ci)
        dw = torch.zeros(Co, 9, Ci)
        for s in range(nsplit):
            dw += ws[s]
        return co.w_nchw(dw.to(torch.bfloat16))

    def conv3x3s1_wgrad(self, x4, dy4):
        return self._wgrad(x4, dy4, 1)

    def conv3x3s2_wgrad(self, x4, dy4):
        return self._wgrad(x4, dy4, 2)


@pytest.fixture
def emu(monkeypatch):
    """tests/test_conv3x3_oracle_gpu.py bound to the emulation on the CPU."""
    e = Emu()
    monkeypatch.setattr(tg, "_C", lambda: e)
    monkeypatch.setattr(tg, "DEV", "cpu")
    monkeypatch.setattr(tg, "RECORD", {})
    tg._exact_case.cache_clear()
    yield e
    tg._exact_case.cache_clear()


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 4, 3, 5), (1, 1, 1, 2, 3), (2, 7, 6, 4, 2), (1, 2, 2, 3, 3), (2, 9, 5, 2, 4),
                                   (3, 13, 11, 5, 7), (1, 2, 9, 4, 4)])
def test_reference_equals_float64_conv2d_and_autograd(shape, stride):
    N, H, W, Ci, Co = shape
    if stride == 2 and min(H, W) < 2:
        H, W = 3, 2
    g = torch.Generator().manual_seed(H * W + stride)
    x = torch.randn(N, H, W, Ci, dtype=torch.float64, generator=g)
    w = torch.randn(Co, 9, Ci, dtype=torch.float64, generator=g)
    xr, wr = co.nchw(x).clone().requires_grad_(True), co.w_nchw(w).clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=stride, padding=1)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)
    dyn = dy.permute(0, 2, 3, 1).contiguous()
    assert y.shape[2:] == (co.out_size(H, stride), co.out_size(W, stride))
    torch.testing.assert_close(co.conv_fwd(x, w, stride), y.permute(0, 2, 3, 1), rtol=0, atol=1e-13)
    torch.testing.assert_close(co.conv_dgrad(dyn, w, H, W, stride), xr.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-13)
    torch.testing.assert_close(co.conv_wgrad(x, dyn, stride), co.from_w_nchw(wr.grad), rtol=0, atol=1e-13)
    torch.testing.assert_close(co.flip_ref(co.flip_ref(wr.detach())), wr.detach(), rtol=0, atol=0)
    # the data gradient IS the stride-1 forward on the flipped weights
    if stride == 1:
        wf = co.from_w_nchw(co.flip_ref(co.w_nchw(w)))
        torch.testing.assert_close(co.conv_fwd(dyn, wf), co.conv_dgrad(dyn, w, H, W), rtol=0, atol=1e-13)


def test_gather_references_equal_the_reference_on_their_fixtures():
    for stride, (N, H, W, Ci, Co) in ((1, (2, 5, 4, 64, 128)), (2, (2, 7, 5, 64, 64)), (2, (1, 6, 8, 128, 64))):
        Ho, Wo = co.out_size(H, stride), co.out_size(W, stride)
        x = co.position_coded(N, H, W, Ci)
        seen = torch.zeros(9 * Ci)
        for p in range(co.onehot_passes(Ci, Co)):
            w, tap, ch, sign = co.onehot_weights(Ci, Co, p)
            seen[tap * Ci + ch] += 1
            assert torch.equal(co.onehot_fwd_ref(x, tap, ch, sign, stride), co.conv_fwd(x.double(), w.double(), stride))
        assert seen.min() >= 1   # every (tap, channel) selected
        dy = co.position_coded(N, Ho, Wo, Co)
        seen = torch.zeros(9 * Co)
        for p in range(co.onehot_passes(Ci, Co, dgrad=True)):
            w, tap, ch, sign = co.onehot_weights(Ci, Co, p, dgrad=True)
            seen[tap * Co + ch] += 1
            assert torch.equal(co.onehot_dgrad_ref(dy, tap, ch, sign, H, W, stride),
                               co.conv_dgrad(dy.double(), w.double(), H, W, stride))
        assert seen.min() >= 1
        R, _, tps, _, _ = co.wgrad_geo(N, H, W, Ci, Co, stride)
        pixels = co.impulse_pixels(N, Ho, Wo, R, tps)
        assert len(set(pixels)) == len(pixels)
        assert all(0 <= n < N and 0 <= h < Ho and 0 <= w_ < Wo for n, h, w_ in pixels)
        for p in range(co.impulse_passes(Co, pixels)):
            idy, which, sign = co.impulse_dy(N, Ho, Wo, Co, pixels, p * Co)
            assert torch.equal(co.impulse_wgrad_ref(x, pixels, which, sign, stride),
                               co.conv_wgrad(x.double(), idy.double(), stride))


def test_position_code_tells_neighbours_apart():
    """Different between any two positions of a 3 x 3 neighbourhood and two rows / columns further, between
    neighbouring images at those offsets, and between channels less than 64 apart; 8 bits."""
    x = co.position_coded(3, 9, 9, 128)
    assert x.abs().max() <= 125 and torch.equal(x, x.to(torch.bfloat16).float())
    for dn in (-1, 0, 1):
        for dh in range(-4, 5):
            for dw in range(-4, 5):
                for dc in range(-63, 64):
                    if (dn, dh, dw, dc) != (0, 0, 0, 0) and (dc == 0 or (dn, dh, dw) == (0, 0, 0)):
                        assert (37 * dn + 101 * dh + 31 * dw + 17 * dc) % 251 != 0, (dn, dh, dw, dc)


def test_fixture_ranges():
    """The preconditions on the references the issue states, on the CPU."""
    for shape, lo in (((2, 7, 7, 64, 64), 60), ((1, 14, 14, 512, 64), 100)):
        x, w = co.fwd_operands(shape)
        ref = co.conv_fwd(x.double(), w.double())
        assert lo <= ref.abs().max() <= co.TERNARY_MAX and 15 < ref.std() < 33
        x, w = co.fwd_operands(shape, kind="offset")
        ref = co.conv_fwd(x.double(), w.double())[:, 1:-1, 1:-1]      # interior outputs: all nine taps
        assert ref.min() >= 0 and ref.max() <= 256 and 54 < ref.mean() < 74 and 5 < ref.std() < 12


# ----------------------------------------------------------------------------- a correct kernel passes every check
def test_emulation_reaches_the_named_variants_and_geometry(emu):
    for case in sorted(co.S1_CASES):
        tg._assert_variant(case)
    for case in tg.EXPECT_NO_WSR:
        with tg._opt(41 & ~32):
            tg._assert_variant(case, 41 & ~32)
    tg.test_wgrad_geometry_of_the_named_cases()
    tg.test_wgrad_declined_shapes_are_declared()
    tg.test_flip_is_the_permutation()


@pytest.mark.parametrize("case,opt", tg.OPT_RUNS, ids=[f"case{c:02d}-opt{o}" for c, o in tg.OPT_RUNS])
def test_emulation_s1_ternary(emu, case, opt):
    tg.test_s1_ternary_exact(case, opt)


@pytest.mark.parametrize("case", co.S1_ONEHOT)
def test_emulation_s1_onehot(emu, case):
    tg.test_s1_onehot(case)


@pytest.mark.parametrize("kind", ["randn", "cancel"])
@pytest.mark.parametrize("case", co.S1_ENVELOPE)
def test_emulation_s1_envelope(emu, case, kind):
    tg.test_s1_envelope(case, kind)


@pytest.mark.parametrize("case", co.S1_STATS)
def test_emulation_s1_stats(emu, case):
    for kind in ("ternary", "offset"):
        tg.test_s1_fwd_stats(case, kind)


@pytest.mark.parametrize("case,opt", [(5, 41), (6, 41), (10, 41 | 128)])
def test_emulation_s1_bnbwd(emu, case, opt):
    tg.test_s1_fwd_bnbwd(case, opt)


@pytest.mark.parametrize("i", range(len(co.S2_CASES)), ids=tg.S2_IDS)
def test_emulation_s2(emu, i):
    tg.test_s2_exact(co.S2_CASES[i])
    if i in co.S2_ONEHOT:
        tg.test_s2_onehot(i)
    if i in co.S2_ENVELOPE:
        for kind in ("randn", "cancel"):
            tg.test_s2_envelope(i, kind)


@pytest.mark.parametrize("stride,shape", tg.WGRAD_RUNS, ids=tg.WGRAD_IDS)
def test_emulation_wgrad(emu, stride, shape):
    tg.test_wgrad_exact(stride, shape)
    if shape in (co.WGRAD_S1_ENVELOPE if stride == 1 else co.WGRAD_S2_ENVELOPE):
        for kind in ("randn", "cancel"):
            tg.test_wgrad_envelope(stride, shape, kind)


# ----------------------------------------------------------------------------- planted faults
FWD_SHAPE = (8, 20, 20, 64, 64)     # 3200 pixels: one wrong pixel is 1 / 3200 of the output
SEAM_SHAPE = (3, 7, 7, 64, 64)      # tile 0 spans all three images
S2_SHAPE = (3, 13, 11, 64, 64)      # odd by odd
S2_LARGE = (16, 51, 51, 64, 64)     # odd by odd, 41616 pixels: one REPLACED pixel is below the old criterion
WG_SHAPE = (3, 28, 28, 64, 64)      # 21 tiles of 4 rows
SINGLE_PIXEL = ("pad_corner", "tap_dropped", "past_m")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _fwd_checks(e, shape, stride=1):
    """(exact check, envelope check, old criterion's figure) of the emulated forward at ``shape``."""
    Ci = shape[3]

    def exact():
        x, w = (t.to(torch.bfloat16) for t in co.fwd_operands(shape, stride))
        co.assert_exact_nhwc(e._fwd(co.nchw(x), co.w_nchw(w), stride).permute(0, 2, 3, 1),
                             co.conv_fwd(co.f64(x), co.f64(w), stride), "exact")

    x, w = (t.to(torch.bfloat16) for t in co.real_operands(shape, "fwd", "randn", stride))
    ref, mag = co.conv_fwd(co.f64(x), co.f64(w), stride), co.conv_fwd(co.f64(x).abs(), co.f64(w).abs(), stride)
    y = e._fwd(co.nchw(x), co.w_nchw(w), stride).permute(0, 2, 3, 1)

    def envelope():
        co.assert_within(y, ref, co.conv_envelope(ref, mag, 9 * Ci), 1.0, co.FLOOR, "envelope")
    return exact, envelope, _rel(y, ref)


def _dgrad_checks(e, shape, stride):
    N, H, W, Ci, Co = shape

    def run(dy, w):
        wf = e.conv3x3_flip(co.w_nchw(w))
        out = e.conv3x3s1_fwd(co.nchw(dy), wf) if stride == 1 else e.conv3x3s2_dgrad(co.nchw(dy), wf, H, W)[0]
        return out.permute(0, 2, 3, 1)

    def exact():
        dy, w = (t.to(torch.bfloat16) for t in co.dgrad_operands(shape, stride))
        co.assert_exact_nhwc(run(dy, w), co.conv_dgrad(co.f64(dy), co.f64(w), H, W, stride), "exact",
                             stride2_dgrad=stride == 2)

    dy, w = (t.to(torch.bfloat16) for t in co.real_operands(shape, "dgrad", "randn", stride))
    ref = co.conv_dgrad(co.f64(dy), co.f64(w), H, W, stride)
    mag = co.conv_dgrad(co.f64(dy).abs(), co.f64(w).abs(), H, W, stride)
    dx = run(dy, w)

    def envelope():
        co.assert_within(dx, ref, co.conv_envelope(ref, mag, 9 * Co), 1.0, co.FLOOR, "envelope")
    return exact, envelope, _rel(dx, ref)


def _wgrad_checks(e, shape, stride=1):
    N, H, W, Ci, Co = shape
    e.conv3x3_wgrad_tune(3 * (Co // 64) * (Ci // 64), 0)    # three splits of seven tiles
    R, ntiles, tps, nsplit, _ = e.conv3x3_wgrad_geo(N, H, W, Ci, Co, stride)
    assert (ntiles, tps, nsplit) == (21, 7, 3)

    def run(x, dy):
        return co.from_w_nchw(e._wgrad(co.nchw(x), co.nchw(dy), stride))

    def exact():
        x, dy = (t.to(torch.bfloat16) for t in co.wgrad_operands(shape, stride))
        co.assert_exact_dw(run(x, dy), co.conv_wgrad(co.f64(x), co.f64(dy), stride), "exact")

    def impulse():
        xc = co.position_coded(N, H, W, Ci)
        pixels = co.impulse_pixels(N, H, W, R, tps)
        for p in range(co.impulse_passes(Co, pixels)):
            idy, which, sign = co.impulse_dy(N, H, W, Co, pixels, p * Co)
            co.assert_exact_dw(run(xc.to(torch.bfloat16), idy.to(torch.bfloat16)),
                               co.impulse_wgrad_ref(xc, pixels, which, sign, stride), "impulse", R=R, Ho=H,
                               tiles_per_split=tps, pixels=pixels, which=which)

    x, dy = (t.to(torch.bfloat16) for t in co.real_operands(shape, "wgrad", "randn", stride))
    ref, mag = co.conv_wgrad(co.f64(x), co.f64(dy), stride), co.conv_wgrad(co.f64(x).abs(), co.f64(dy).abs(), stride)
    dw = run(x, dy)

    def envelope():
        co.assert_within(dw, ref, co.conv_envelope(ref, mag, N * H * W, nsplit), 1.0, co.FLOOR, "envelope")
    return exact, impulse, envelope, _rel(dw, ref)


def _stats_checks(e, shape):
    x, w = (t.to(torch.bfloat16) for t in co.fwd_operands(shape, 1, "offset"))
    ref = co.conv_fwd(co.f64(x), co.f64(w))
    y, part = e.conv3x3s1_fwd_stats(co.nchw(x), co.w_nchw(w))
    s, m2, env = co.stats_oracle(ref, co.BM)

    def exact():
        assert torch.equal(y.permute(0, 2, 3, 1), ref.to(torch.bfloat16))
        assert co.mismatches(part[0], s.float())[0] == 0, "sums differ"

    def envelope():
        co.assert_within(part[1], m2, env, 1.0, co.FLOOR, "m2")
    return exact, envelope


def _checks(fault, planted=True):
    """(the checks that must all fail with ``fault`` planted and pass without, the old criterion's figure or None)."""
    e = Emu(fault if planted else None)
    if fault in ("pad_corner", "tap_dropped"):
        ex, env, rel = _fwd_checks(e, FWD_SHAPE)
    elif fault == "wrong_image":
        ex, env, rel = _fwd_checks(e, SEAM_SHAPE)
    elif fault == "s2_odd_edge":
        ex, env, rel = _fwd_checks(e, S2_SHAPE, 2)
    elif fault == "flip_tap":
        ex, env, rel = _dgrad_checks(e, FWD_SHAPE, 1)
    elif fault in ("s2_parity", "past_m"):
        ex, env, rel = _dgrad_checks(e, S2_LARGE if fault == "past_m" else S2_SHAPE, 2)
    elif fault in ("tile_missing", "row_twice"):
        ex, imp, env, rel = _wgrad_checks(e, WG_SHAPE)
        return (ex, env) + ((imp,) if fault == "tile_missing" else ()), rel   # (no impulse sits in the doubled row)
    else:
        assert fault == "stats_last_row"
        return _stats_checks(e, (3, 13, 11, 64, 64)), None
    return (ex, env), rel


FAULTS = ("pad_corner", "tap_dropped", "wrong_image", "past_m", "flip_tap", "s2_parity", "s2_odd_edge", "tile_missing",
          "row_twice", "stats_last_row")


def test_checks_pass_without_a_fault():
    for fault in FAULTS:
        checks, rel = _checks(fault, planted=False)
        for check in checks:
            check()
        assert rel is None or rel < 1e-2


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_fails_exact_and_envelope(fault):
    checks, rel = _checks(fault)
    for check in checks:
        with pytest.raises(AssertionError):
            check()
    if fault in SINGLE_PIXEL:   # the gap: the earlier criterion accepts a wrong pixel
        assert rel < 1e-2, rel
    if fault == "flip_tap":
        w4 = co.w_nchw(torch.randn(64, 9, 64).to(torch.bfloat16))
        assert not torch.equal(Emu(fault).conv3x3_flip(w4), co.flip_ref(w4))
        assert torch.equal(Emu().conv3x3_flip(w4), co.flip_ref(w4))


def test_mismatch_reports_name_the_place():
    e = Emu("tap_dropped")
    N, H, W, Ci, Co = shape = FWD_SHAPE
    x = co.position_coded(N, H, W, Ci)
    w, tap, ch, sign = co.onehot_weights(Ci, Co, 4)      # pass 4: (co + 256) mod 576 -> taps 4 and 5
    assert int(tap[0]) == 4
    y = e._fwd(co.nchw(x.to(torch.bfloat16)), co.w_nchw(w.to(torch.bfloat16)), 1).permute(0, 2, 3, 1)
    with pytest.raises(AssertionError, match=r"tile 0, row 255, image 0 position \(12, 15\), channel 0, tap 4 "
                                             r"\(kh, kw\) = \(1, 1\), reduced channel 0 \(chunk 0\)"):
        co.assert_exact_nhwc(y, co.onehot_fwd_ref(x, tap, ch, sign), "onehot", tap=tap, ch=ch)
    assert "phase (py, px) = (1, 0), tile 0, row 13" in co.describe((0, 5, 2, 3), (2, 13, 11, 64), stride2_dgrad=True)
    e = Emu("tile_missing")
    ex, imp, env, _ = _wgrad_checks(e, WG_SHAPE)
    with pytest.raises(AssertionError, match=r"tile 20, split 2"):
        imp()


# ----------------------------------------------------------------------------- the host's halo bounds
def test_forward_halo_bound_covers_every_tile():
    """halo_rows_bound(H, W) >= the Q of every 256-pixel tile (kernels' pr0 / Q), over every alignment of a tile
    in an image: the tile origins 256 k mod H W cycle after H W / gcd(256, H W) tiles."""
    for H in range(1, 71):
        for W in range(1, 71):
            HW, H2, W2 = H * W, H + 2, W + 2
            ntile = HW // math.gcd(256, HW) + 1
            m0 = 256 * np.arange(ntile, dtype=np.int64)
            ml = m0 + 255
            pr0 = (m0 // HW) * H2 + (m0 % HW) // W
            Q = ((ml // HW) * H2 + (ml % HW) // W + 2 - pr0 + 1) * W2
            assert co.halo_rows_bound(H, W) >= Q.max(), (H, W, co.halo_rows_bound(H, W), int(Q.max()))
    # case 10's tiles align with its images (32 * 56 = 7 * 256): 464 rows staged under a bound of 580; case 11's do
    # not, and reach the bound
    assert (co.halo_rows_need(33, 32, 56), co.halo_rows_bound(32, 56)) == (464, 580)
    assert (co.halo_rows_need(5, 30, 56), co.halo_rows_bound(30, 56)) == (580, 580)


@pytest.mark.parametrize("stride", [1, 2])
def test_wgrad_halo_bound_covers_every_tile(stride):
    """conv3x3_wgrad.hip halo_rows(R, ...) >= the halo rows of every tile of the tile table, for every R the
    geometry search visits, with enough images for every alignment of a tile in an image."""
    for Hi in range(stride, 71):
        for Wi in range(stride, 71):
            H, W = co.out_size(Hi, stride), co.out_size(Wi, stride)
            hmax, kpmax = (256, 128) if stride == 1 else (320, 64)
            R = co.wgrad_rows_per_tile(W)
            while True:
                N = math.lcm(R, H) // H + R // H + 2
                bound = co.wgrad_halo_rows(R, H, W, stride, Hi, Wi)
                need = co.wgrad_halo_need(N, R, H, W, stride, Hi, Wi)
                assert bound >= need, (stride, Hi, Wi, R, bound, need)
                if R == 1 or not (bound > hmax or ((R * W + 15) & ~15) > kpmax):
                    break
                R -= 1
