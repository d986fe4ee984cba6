"""Exact and envelope oracles for the 3x3 convolution kernels (csrc/kernels/conv3x3.hip: six stride-1 forward
kernels, also the stride-1 data gradient on flipped weights; conv3x3_s2.hip: the stride-2 forward and 4-phase data
gradient; conv3x3_wgrad.hip: the split-K weight gradient at both strides; the BatchNorm epilogues of
tile_stats.h). A helper module imported by plain name, like gemm_oracle.py, whose comparator and constants
(``assert_within``, ``assert_exact``, ``mismatches``, U_BF16, U_FP32, FLOOR, TERNARY_MAX) it reuses.
tests/test_conv3x3_oracle_cpu.py proves on the CPU that it is sharp, tests/test_conv3x3_oracle_gpu.py runs the kernels.

Layout. Everything here is NHWC: x [N, H, W, Ci], w [Co, 9, Ci] (tap t = 3 kh + kw, the kernels' storage of a
channels_last [Co, Ci, 3, 3] weight), y [N, Ho, Wo, Co], Ho = (H - 1) // s + 1, padding 1. ``nchw`` / ``w_nchw``
give the channels_last views the bindings take without moving a byte.

Reference. No library convolution (MIOpen may pick Winograd, which is not exact on integers):
    y  = sum_t shift_t(pad(x)) @ w[:, t, :]^T         shift_t(xp)[n, oh, ow] = xp[n, s oh + kh, s ow + kw]
    dx = the same relation transposed: pad(dx)[shift_t] += dy @ w[:, t, :]
    dW[co, t, ci] = dy^T @ shift_t(pad(x))
in float64 on the stored operand values, on any device. The CPU test proves the three equal to float64
``F.conv2d`` and its autograd gradients, odd sizes at stride 2 included. Applied to |x|, |w|, |dy| they give the
magnitude terms of the envelopes.

(a) Exact fixtures: bit for bit. As gemm_oracle (a): integer operands with every partial sum below 2^24 keep
the fp32 accumulators exact in ANY order, across taps, 32-channel chunks and K-splits, and through the
fixed-order reduce kernel of the weight gradient; results up to 256 are bf16 numbers; so the output must EQUAL
``ref.to(bfloat16)``.
  * ``ternary``: entries in {-1, 0, +1}, nonzero with probability p = min(1, 32 / sqrt(Kred)), Kred = 9 Ci for
    the forward, 9 Co for the data gradient, N Ho Wo for the weight gradient; the generator is seeded from the
    shape. An output is a sum of at most Kred p^2 <= 1024 terms +-1 (standard deviation <= 32); the tests assert
    |ref| <= 256 on the REFERENCE, a precondition on the inputs.
  * ``offset``: entries in {0, 1} with density 8 / sqrt(Kred) (1 when Kred <= 64): interior outputs have mean
    Kred p^2 = 64 and standard deviation < 8, all in [0, 256]. For the statistics epilogues, where mean^2 >> variance.
  * One-hot weights on a position-coded input. ``position_coded``: x[n, h, w, c] = ((37 n + 101 h + 31 w + 17 c)
    mod 251) - 125, 8 bits, different between any two positions of a 3 x 3 neighbourhood (and two rows or
    columns further), between neighbouring images and between channels less than 64 apart (the CPU test checks
    that). ``onehot_weights``: w[co] = +-e_(tap, ci) with (tap, ci)(co) = (co + pass Co) mod 9 Ci (tap-major), over
    ceil(9 Ci / Co) passes, so every (tap, channel) is selected once. Then y[n, oh, ow, co] = +-x[n, s oh + kh - 1,
    s ow + kw - 1, ci], or 0 in the padding: a gather (``onehot_fwd_ref``), exact under any accumulation arithmetic.
    For the data gradient the roles turn: ``onehot_weights(Co, Ci, pass, dgrad=True)`` gives every INPUT channel
    one (tap, co), and dx[n, ih, iw, ci] = +-dy[n, (ih + 1 - kh) / s, (iw + 1 - kw) / s, co] where that pixel
    exists (``onehot_dgrad_ref``, a scatter of copies). A mismatch report (``describe``) names the 256-pixel tile,
    the row in it, the image position, the tap, the 32-channel chunk and, at stride 2, the phase (py, px).
  * Impulse output gradients for the weight gradient, ``impulse_dy``: one +-1 per output channel at a pixel from
    ``impulse_pixels``: image corners, the first and last pixel of weight-gradient tiles (the first two, the last
    two and the first and last tile of every split), and the pixels on either side of every image boundary that
    falls inside a tile. Then dW[co, t, ci] = +-pad(x)[pixel(co) + shift(t), ci] on the coded input: a gather.
  * conv3x3_flip is a permutation: ``flip_ref`` = w.flip(2, 3).transpose(0, 1), bit for bit.

(b) Real-valued operands: an envelope, c = 1, floor = FLOOR. Derived as ``gemm_envelope``: one rounding of the
output to bf16, U_BF16 |ref|; a sum of Kred exact products in fp32 in ANY order errs by at most (Kred - 1)
U_FP32 sum |terms| to first order, the split-K partials add nsplit - 1 roundings and the reduce's two-level sum
no more than that again; the factor 2 allows for accumulation inside the MFMA unit that need not be IEEE
sequential summation:
    forward:  U_BF16 |ref| + 2 (9 Ci + 2) U_FP32 (|x| * |w|)       data gradient: 9 Co for 9 Ci
    wgrad:    U_BF16 |ref| + 2 (N Ho Wo + nsplit + 2) U_FP32 (|dy|^T * |x|)
with * the same three reference functions on absolute values. Operands (``real_operands``): ``randn``, weights
scaled so that outputs are about N(0, 1.5^2), and ``cancel``, built as gemm_oracle.real_operands builds it: the
second half of the reduced channels repeats the first with the weights negated and one entry in 64 redrawn
(weight gradient, which reduces over pixels: odd images repeat the even ones with dy negated, one entry in 64
redrawn), so ref is about 2^-7 of the magnitude term, where a relative tolerance would pass anything. No
constant is fitted to what the kernels return.

(c) Fused statistics (tile_stats.h, layout [2, T, C], tiles of ``rows`` consecutive pixels: 224 on the row-tile
kernel, 256 elsewhere, as the binding's pdt_conv3x3s1_stats_tile_rows / _bnbwd_tile_rows say). Run on the exact
fixtures, where the accumulator values and the stored bf16 values coincide.
  * part[0], per-tile sums: integers of magnitude at most 256 * 256, exact in fp32 in any order (also as
    n K + sum (y - K)): compared bit for bit with the float64 sums rounded to fp32.
  * part[1], centred sums of squares, against sum (y - tile mean)^2 in float64 with the envelope
        (n_t + 16) U_FP32 (sum (y - K)^2 + (sum (y - K))^2 / n_t),     K = the tile's first row, c = 1:
    the shifted form of tile_stats.h computes Q = sum (y - K)^2 and S = sum (y - K) (exact on integers below
    2^24) and then Q - S^2 / n: a square, a division and a subtraction, each rounded relative to a quantity
    the bracket bounds; a two-pass or pairwise-merged (Chan) form sums n_t squares (y - mean)^2 <= 2 (y - K)^2 +
    2 (mean - K)^2 in fp32, which (n_t + 16) U_FP32 times the bracket bounds as well. One row left out moves an
    entry by about (y - mean)^2 ~ 64 on the offset fixture, ~100 such bounds.
  * Backward partials (conv3x3s1_fwd_bnbwd, conv3x3s2_dgrad with bn_x): ``bn_inputs`` gives an integer bn_x in
    [-8, 8], an integer bn_mean in [-8, 8] and a random ReLU bit mask (bit c % 8 of byte (m C + c) / 8). dz = y
    mask; sum dz and sum dz (x - mean) are integers below 256 * 256 * 16 = 2^20: both rows bit for bit. The
    stride-2 data gradient's tiles are 256 consecutive pixels of ONE phase's (n, ih // 2, iw // 2) space, row
    (2 py + px) tiles_per_phase + tile.

What the GPU found is recorded in profiles/r15/conv3x3_oracle_ratios.txt.
"""
from __future__ import annotations

import math

import torch

from gemm_oracle import (FLOOR, TERNARY_MAX, U_BF16, U_FP32, assert_exact, assert_within,  # noqa: F401  (re-exported)
                         mismatches)

BM = 256          # pixels per forward / data-gradient tile
BM_WSR = 224      # ... on the row-tile kernel (4 rows of 56)
CHUNK = 32        # input channels per k-step chunk
VARIANTS = ("tap_wide", "tap_narrow", "halo_wide", "halo_narrow", "wst", "wsr")

# (N, H, W, Ci, Co) -> the forward variant and the stride-1 data-gradient variant (the forward launcher on dy
# with Ci and Co swapped) under the default conv3x3_opt bits on 256 compute units
S1_CASES = {
    1: (1, 1, 1, 64, 64),
    2: (2, 3, 3, 64, 128),
    3: (1, 5, 300, 64, 128),
    4: (5, 7, 7, 128, 64),
    5: (11, 7, 7, 64, 128),
    6: (21, 28, 28, 64, 512),
    7: (2, 13, 11, 64, 64),
    8: (23, 54, 54, 64, 64),
    9: (300, 4, 56, 64, 64),
    10: (33, 32, 56, 64, 64),
    11: (5, 30, 56, 64, 64),    # wst with tiles that cross images at W = 56: the 580-row halo (case 10 stages 464)
}
S1_ONEHOT = (1, 2, 4, 5, 7, 9)
S1_ENVELOPE = (3, 5, 6, 8, 10)
S1_STATS = (5, 6, 7, 8, 9, 10)
S2_CASES = [(1, 2, 2, 64, 64), (2, 13, 11, 128, 256), (2, 9, 30, 128, 128), (5, 15, 15, 64, 64),
            (9, 14, 14, 128, 128), (3, 24, 24, 64, 128), (2, 17, 20, 128, 64)]
S2_ONEHOT = (0, 1, 3)
S2_ENVELOPE = (1, 4, 5)
WGRAD_S1_CASES = [S1_CASES[2], S1_CASES[4], S1_CASES[5], S1_CASES[7], (2, 56, 56, 64, 64), (3, 28, 28, 128, 128),
                  (7, 14, 14, 256, 256)]
WGRAD_S1_ENVELOPE = ((3, 28, 28, 128, 128), (7, 14, 14, 256, 256))
WGRAD_S2_ENVELOPE = (S2_CASES[4], S2_CASES[5])
# shapes the weight-gradient kernel declines (no tile of whole rows fits its K-row cap): (shape, stride)
EXPECT_DECLINED = [((1, 5, 300, 64, 64), 1)]


def f64(t):
    return t.float().double()


def out_size(H, stride):
    return (H - 1) // stride + 1


def nchw(t):
    """NHWC storage as the channels_last [N, C, H, W] tensor the bindings take (a view)."""
    return t.permute(0, 3, 1, 2)


def w_nhwc(w):
    """[Co, 9, Ci] -> [Co, 3, 3, Ci]."""
    return w.reshape(w.shape[0], 3, 3, w.shape[2])


def w_nchw(w):
    """[Co, 9, Ci] storage as the channels_last [Co, Ci, 3, 3] weight (a view)."""
    return w_nhwc(w).permute(0, 3, 1, 2)


def from_w_nchw(w4):
    """A [Co, Ci, 3, 3] weight (any strides) as [Co, 9, Ci]."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], 9, w4.shape[1])


# ----------------------------------------------------------------------------- reference
def pad(x):
    N, H, W, C = x.shape
    xp = x.new_zeros(N, H + 2, W + 2, C)
    xp[:, 1:-1, 1:-1] = x
    return xp


def shift(xp, t, Ho, Wo, stride):
    """The padded input pixels tap ``t`` pairs with the Ho x Wo outputs: xp[n, s oh + kh, s ow + kw] (a view)."""
    kh, kw = divmod(t, 3)
    return xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]


def conv_fwd(x, w, stride=1):
    """x [N, H, W, Ci], w [Co, 9, Ci] -> y [N, Ho, Wo, Co], in the operands' dtype (float64 for a reference)."""
    N, H, W, _ = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = pad(x)
    y = x.new_zeros(N, Ho, Wo, w.shape[0])
    for t in range(9):
        y += shift(xp, t, Ho, Wo, stride) @ w[:, t, :].t()
    return y


def conv_dgrad(dy, w, H, W, stride=1):
    """dy [N, Ho, Wo, Co], w [Co, 9, Ci] -> dx [N, H, W, Ci]."""
    N, Ho, Wo, _ = dy.shape
    assert (Ho, Wo) == (out_size(H, stride), out_size(W, stride))
    dxp = dy.new_zeros(N, H + 2, W + 2, w.shape[2])
    for t in range(9):
        shift(dxp, t, Ho, Wo, stride).add_(dy @ w[:, t, :])
    return dxp[:, 1:-1, 1:-1].contiguous()


def conv_wgrad(x, dy, stride=1):
    """x [N, H, W, Ci], dy [N, Ho, Wo, Co] -> dW [Co, 9, Ci]."""
    _, Ho, Wo, Co = dy.shape
    xp = pad(x)
    g = dy.reshape(-1, Co).t()
    return torch.stack([g @ shift(xp, t, Ho, Wo, stride).reshape(-1, x.shape[3]) for t in range(9)], 1)


def flip_ref(w4):
    """conv3x3_flip of a [Co, Ci, 3, 3] weight: wf[ci, co, kh, kw] = w[co, ci, 2 - kh, 2 - kw]."""
    return w4.flip(2, 3).transpose(0, 1)


# ----------------------------------------------------------------------------- (a) exact fixtures
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ternary_p(kred):
    return min(1.0, 32.0 / math.sqrt(kred))


def offset_p(kred):
    return min(1.0, 8.0 / math.sqrt(kred))


def _draw(shape, p, g, signed):
    u = torch.rand(*shape, generator=g)
    if signed:
        return torch.where(u < p / 2, -1.0, torch.where(u < p, 1.0, 0.0))
    return (u < p).float()


def exact_operands(shapes, kred, key, kind="ternary"):
    """fp32 CPU tensors of the given shapes, ``ternary`` ({-1, 0, +1}) or ``offset`` ({0, 1}), from a generator
    seeded with ``key`` (the case's shape and role)."""
    g = _gen(*key, 1 if kind == "offset" else 0)
    p = ternary_p(kred) if kind == "ternary" else offset_p(kred)
    return [_draw(s, p, g, kind == "ternary") for s in shapes]


def fwd_operands(shape, stride=1, kind="ternary"):
    """(x [N, H, W, Ci], w [Co, 9, Ci]) of the forward fixture."""
    N, H, W, Ci, Co = shape
    return exact_operands([(N, H, W, Ci), (Co, 9, Ci)], 9 * Ci, shape + (stride, 1), kind)


def dgrad_operands(shape, stride=1, kind="ternary"):
    """(dy [N, Ho, Wo, Co], w [Co, 9, Ci]) of the data-gradient fixture."""
    N, H, W, Ci, Co = shape
    return exact_operands([(N, out_size(H, stride), out_size(W, stride), Co), (Co, 9, Ci)], 9 * Co,
                          shape + (stride, 2), kind)


def wgrad_operands(shape, stride=1, kind="ternary"):
    """(x [N, H, W, Ci], dy [N, Ho, Wo, Co]) of the weight-gradient fixture."""
    N, H, W, Ci, Co = shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    return exact_operands([(N, H, W, Ci), (N, Ho, Wo, Co)], N * Ho * Wo, shape + (stride, 3), kind)


def position_coded(N, H, W, C, device="cpu"):
    """[N, H, W, C] fp32: ((37 n + 101 h + 31 w + 17 c) mod 251) - 125."""
    def axis(n, k, d):
        return (k * torch.arange(n, device=device)).reshape([-1 if i == d else 1 for i in range(4)])
    return ((axis(N, 37, 0) + axis(H, 101, 1) + axis(W, 31, 2) + axis(C, 17, 3)) % 251 - 125).float()


def onehot_passes(Ci, Co, dgrad=False):
    """Passes after which every (tap, reduced channel) was selected by some output channel."""
    kred, rows = (9 * Co, Ci) if dgrad else (9 * Ci, Co)
    return (kred + rows - 1) // rows


def onehot_weights(Ci, Co, p, dgrad=False, device="cpu"):
    """Pass ``p``. Forward: output channel co selects (tap, ci) = divmod((co + p Co) mod 9 Ci, Ci). Data gradient:
    input channel ci selects (tap, co) = divmod((ci + p Ci) mod 9 Co, Co). Returns (w [Co, 9, Ci] fp32, tap, ch,
    sign), the last three indexed by the selecting channel."""
    rows, red = (Ci, Co) if dgrad else (Co, Ci)
    r = torch.arange(rows, device=device)
    idx = (r + p * rows) % (9 * red)
    tap, ch = idx // red, idx % red
    sign = torch.where((r + p) % 3 == 0, -1.0, 1.0)
    w = torch.zeros(Co, 9, Ci, device=device)
    if dgrad:
        w[ch, tap, r] = sign
    else:
        w[r, tap, ch] = sign
    return w, tap, ch, sign


def onehot_fwd_ref(x, tap, ch, sign, stride=1):
    """y[n, oh, ow, co] = sign[co] pad(x)[n, s oh + kh(co), s ow + kw(co), ch(co)]: a gather, float64."""
    N, H, W, _ = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = pad(x.double())
    y = xp.new_zeros(N, Ho, Wo, tap.numel())
    for t in range(9):
        cols = (tap == t).nonzero()[:, 0]
        if cols.numel():
            y[..., cols] = shift(xp, t, Ho, Wo, stride)[..., ch[cols]] * sign[cols].double()
    return y


def onehot_dgrad_ref(dy, tap, ch, sign, H, W, stride=1):
    """dx[n, ih, iw, ci] = sign[ci] dy[n, (ih + 1 - kh) / s, (iw + 1 - kw) / s, ch(ci)] where that pixel exists,
    else 0: copies, float64."""
    N, Ho, Wo, _ = dy.shape
    dxp = dy.new_zeros(N, H + 2, W + 2, tap.numel(), dtype=torch.float64)
    for t in range(9):
        cols = (tap == t).nonzero()[:, 0]
        if cols.numel():
            shift(dxp, t, Ho, Wo, stride)[..., cols] = dy.double()[..., ch[cols]] * sign[cols].double()
    return dxp[:, 1:-1, 1:-1].contiguous()


def wgrad_tiles(N, Ho, R):
    """[(first global output row, end)] of the weight gradient's pixel tiles: R whole rows of the N Ho rows."""
    NH = N * Ho
    return [(g0, min(g0 + R, NH)) for g0 in range(0, NH, R)]


def impulse_pixels(N, Ho, Wo, R, tiles_per_split):
    """The declared probe pixels (n, oh, ow) of the weight gradient, in order, without repeats."""
    tiles = wgrad_tiles(N, Ho, R)
    nt = len(tiles)
    picks = {0, 1, nt - 2, nt - 1}
    for s in range(0, nt, tiles_per_split):
        picks |= {s, min(s + tiles_per_split, nt) - 1}
    rows = []  # (global row, column)
    for n in (0, N - 1):
        rows += [(n * Ho, 0), (n * Ho, Wo - 1), (n * Ho + Ho - 1, 0), (n * Ho + Ho - 1, Wo - 1)]
    for t in sorted(p for p in picks if 0 <= p < nt):
        rows += [(tiles[t][0], 0), (tiles[t][1] - 1, Wo - 1)]
    for g0, g1 in tiles:  # an image boundary strictly inside a tile
        for b in range((g0 // Ho + 1) * Ho, g1, Ho):
            rows += [(b - 1, Wo - 1), (b, 0)]
    out = []
    for g, c in rows:
        px = (g // Ho, g % Ho, c)
        if px not in out:
            out.append(px)
    return out


def impulse_dy(N, Ho, Wo, Co, pixels, p=0, device="cpu"):
    """dy [N, Ho, Wo, Co] with one +-1 per output channel at pixels[(co + p) % len]. Returns (dy, index [Co] into
    ``pixels``, sign [Co])."""
    co = torch.arange(Co, device=device)
    which = (co + p) % len(pixels)
    sign = torch.where((co + p) % 3 == 0, -1.0, 1.0)
    px = torch.tensor(pixels, device=device)[which]
    dy = torch.zeros(N, Ho, Wo, Co, device=device)
    dy[px[:, 0], px[:, 1], px[:, 2], co] = sign
    return dy, which, sign


def impulse_passes(Co, pixels):
    return (len(pixels) + Co - 1) // Co


def impulse_wgrad_ref(x, pixels, which, sign, stride=1):
    """dW[co, t, ci] = sign[co] pad(x)[n, s oh + kh, s ow + kw, ci] at pixel(co) = (n, oh, ow): a gather, float64."""
    xp = pad(x.double())
    px = torch.tensor(pixels, device=x.device)[which]
    taps = [xp[px[:, 0], stride * px[:, 1] + t // 3, stride * px[:, 2] + t % 3] for t in range(9)]
    return torch.stack(taps, 1) * sign.double()[:, None, None]


# ----------------------------------------------------------------------------- reports
def describe(idx, shape4, rows=BM, tap=None, ch=None, stride2_dgrad=False):
    """Where element ``idx`` = (n, h, w, c) of an NHWC output [N, H, W, C] sits in the kernel's terms: the tile
    of ``rows`` pixels and the row in it, the image position, with ``tap`` / ``ch`` (indexed by c) the tap and
    32-channel chunk a one-hot probe selected there. ``stride2_dgrad``: tiles run over one phase's pixels."""
    n, h, w, c = idx
    _, H, W, _ = shape4
    if stride2_dgrad:
        Hp, Wp = out_size(H, 2), out_size(W, 2)
        m = (n * Hp + h // 2) * Wp + w // 2
        s = f"phase (py, px) = ({h % 2}, {w % 2}), tile {m // rows}, row {m % rows}"
    else:
        m = (n * H + h) * W + w
        s = f"tile {m // rows}, row {m % rows}"
    s += f", image {n} position ({h}, {w}), channel {c}"
    if tap is not None:
        k = int(ch[c])
        s += f", tap {int(tap[c])} (kh, kw) = {divmod(int(tap[c]), 3)}, reduced channel {k} (chunk {k // CHUNK})"
    return s


def assert_exact_nhwc(got, ref64, name="", record=None, **where):
    """``got`` (bf16, NHWC [N, H, W, C]) must equal ``ref64.to(bfloat16)``; the report is ``describe``'s."""
    want = ref64.to(torch.bfloat16)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (name, got.shape, got.dtype, want.shape)
    C = got.shape[3]
    n, at = mismatches(got.reshape(-1, C), want.reshape(-1, C))
    if record is not None:
        record[name] = max(record.get(name, 0), n)
    if n:
        m, c = at
        _, H, W, _ = got.shape
        idx = (m // (H * W), m // W % H, m % W, c)
        raise AssertionError(f"{name}: {n} of {got.numel()} elements differ; first at {idx}: "
                             f"{describe(idx, got.shape, **where)}: "
                             f"got {float(got[idx]):.9g}, want {float(want[idx]):.9g}")
    return 0


def assert_exact_dw(got, ref64, name="", record=None, R=None, Ho=None, tiles_per_split=None, pixels=None, which=None):
    """``got`` (bf16 [Co, 9, Ci]) must equal ``ref64.to(bfloat16)``. With an impulse probe's ``pixels`` / ``which``
    the report names the pixel, its weight-gradient tile and split."""
    want = ref64.to(torch.bfloat16)
    assert got.shape == want.shape and got.dtype == torch.bfloat16, (name, got.shape, got.dtype, want.shape)
    Co, _, Ci = got.shape
    n, at = mismatches(got.reshape(Co, 9 * Ci), want.reshape(Co, 9 * Ci))
    if record is not None:
        record[name] = max(record.get(name, 0), n)
    if n:
        co, k = at
        t, ci = divmod(k, Ci)
        s = f"co {co}, tap {t} (kh, kw) = {divmod(t, 3)}, ci {ci} (channel block {ci // 64})"
        if pixels is not None:
            pn, oh, ow = pixels[int(which[co])]
            tile = (pn * Ho + oh) // R
            s += f", impulse at image {pn} pixel ({oh}, {ow}): tile {tile}, split {tile // tiles_per_split}"
        raise AssertionError(f"{name}: {n} of {got.numel()} elements differ; first at ({co}, {t}, {ci}): {s}: "
                             f"got {float(got[co, t, ci]):.9g}, want {float(want[co, t, ci]):.9g}")
    return 0


# ----------------------------------------------------------------------------- (b) envelope
def _q(t):
    return t.to(torch.bfloat16).float()


def real_operands(shape, role, kind="randn", stride=1, seed=0):
    """fp32 CPU operands holding bf16 values. role "fwd": (x, w); "dgrad": (dy, w); "wgrad": (x, dy). ``randn``:
    the gathered tensor ~ N(0, 1), the weights ~ N(0, 1.5^2 / Kred) (wgrad: dy ~ N(0, 1.5^2 / (N Ho Wo))). ``cancel``:
    the second half of the reduced channels repeats the first with the weights negated, one entry in 64 redrawn;
    wgrad: image 2k + 1 repeats image 2k with dy negated, one entry in 64 redrawn (an odd last image keeps only
    the redrawn entries)."""
    N, H, W, Ci, Co = shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    g = _gen(*shape, stride, seed, {"fwd": 1, "dgrad": 2, "wgrad": 3}[role], 7 if kind == "cancel" else 0)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if role == "wgrad":
        sd = 1.5 / math.sqrt(N * Ho * Wo)
        x, dy = _q(rn(N, H, W, Ci)), _q(rn(N, Ho, Wo, Co) * sd)
        if kind == "cancel":
            redraw = torch.rand(N, Ho, Wo, Co, generator=g) < 1.0 / 64
            fresh = _q(rn(N, Ho, Wo, Co) * sd)
            src = torch.arange(N) // 2 * 2
            paired = (torch.arange(N) % 2 == 1)[:, None, None, None]
            x = x[src].contiguous()
            anti = torch.where(paired, -dy[src], torch.zeros(()))
            has_pair = (src + 1 < N)[:, None, None, None]
            dy = torch.where(paired, torch.where(redraw, fresh, anti),
                             torch.where(has_pair, dy, torch.where(redraw, fresh, torch.zeros(()))))
        return x.contiguous(), dy.contiguous()
    cr, cw = (Ci, Co) if role == "fwd" else (Co, Ci)     # reduced channels, the other weight dimension
    sd = 1.5 / math.sqrt(9 * cr)
    k = cr // 2 if kind == "cancel" else cr
    a = _q(rn(N, H, W, k)) if role == "fwd" else _q(rn(N, Ho, Wo, k))
    b = _q(rn(cw, 9, k) * sd)                            # [other, tap, reduced]
    if kind == "cancel":
        redraw = torch.rand(cw, 9, k, generator=g) < 1.0 / 64
        b2 = torch.where(redraw, _q(rn(cw, 9, k) * sd), -b)
        a, b = torch.cat([a, a], 3), torch.cat([b, b2], 2)
    w = b if role == "fwd" else b.permute(2, 1, 0)       # -> [Co, 9, Ci]
    return a.contiguous(), w.contiguous()


def conv_envelope(ref, mag, kred, nsplit=0):
    """U_BF16 |ref| + 2 (Kred + nsplit + 2) U_FP32 mag, with mag the reference function on absolute values."""
    return U_BF16 * ref.abs() + 2 * (kred + nsplit + 2) * U_FP32 * mag


# ----------------------------------------------------------------------------- (c) fused statistics
def tiles_2d(y2, rows):
    """[M, C] -> ([T, rows, C] zero-padded, n_t [T] float64)."""
    M, C = y2.shape
    T = (M + rows - 1) // rows
    yp = y2.new_zeros(T * rows, C)
    yp[:M] = y2
    n = torch.full((T,), float(rows), dtype=torch.float64, device=y2.device)
    n[-1] = M - (T - 1) * rows
    return yp.reshape(T, rows, C), n


def stats_oracle(y64, rows):
    """Per-tile statistics of the float64 output y [N, H, W, C] over tiles of ``rows`` consecutive pixels.
    Returns (sums [T, C], m2 [T, C], env_m2 [T, C]) in float64."""
    C = y64.shape[-1]
    yt, n = tiles_2d(y64.reshape(-1, C), rows)
    T = yt.shape[0]
    valid = (torch.arange(rows, device=y64.device)[None, :] < n[:, None])[:, :, None]
    s = yt.sum(1)
    mean = s / n[:, None]
    m2 = (torch.where(valid, yt - mean[:, None, :], 0.0) ** 2).sum(1)
    d = torch.where(valid, yt - yt[:, :1, :], 0.0)
    env = (n[:, None] + 16) * U_FP32 * ((d * d).sum(1) + d.sum(1) ** 2 / n[:, None])
    assert s.shape == (T, C)
    return s, m2, env


def bn_inputs(N, H, W, C, seed=0):
    """(bn_x [N, H, W, C] integers in [-8, 8], bn_mean [C] integers in [-8, 8], keep [N, H, W, C] bool, mask bytes
    [N H W C / 8] uint8 with bit c % 8 of byte (m C + c) / 8), fp32 / bool / uint8 on the CPU."""
    g = _gen(N, H, W, C, seed, 99)
    bx = torch.randint(-8, 9, (N, H, W, C), generator=g).float()
    mean = torch.randint(-8, 9, (C,), generator=g).float()
    keep = torch.rand(N, H, W, C, generator=g) > 0.3
    bits = keep.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)
    return bx, mean, keep, bits.sum(1).to(torch.uint8)


def bnbwd_oracle(y64, bn_x, bn_mean, keep, rows=BM, phases=False):
    """[2, T, C] float64: per tile sum dz and sum dz (x - mean), dz = y keep. ``phases``: the stride-2 data
    gradient's tiles: for each phase (py, px) in order, tiles of ``rows`` pixels of y[:, py::2, px::2] laid out on
    the FULL phase grid (Hp, Wp) = (ceil(H / 2), ceil(W / 2)), pixels outside the image adding nothing."""
    N, H, W, C = y64.shape
    dz = y64 * keep.double()
    a, b = dz, dz * (bn_x.double() - bn_mean.double())
    if not phases:
        return torch.stack([tiles_2d(v.reshape(-1, C), rows)[0].sum(1) for v in (a, b)])
    Hp, Wp = out_size(H, 2), out_size(W, 2)
    out = []
    for v in (a, b):
        per = []
        for py in (0, 1):
            for px in (0, 1):
                g = v.new_zeros(N, Hp, Wp, C)
                sub = v[:, py::2, px::2]
                g[:, :sub.shape[1], :sub.shape[2]] = sub
                per.append(tiles_2d(g.reshape(-1, C), rows)[0].sum(1))
        out.append(torch.cat(per))
    return torch.stack(out)


# ----------------------------------------------------------------------------- host geometry (the kernels' own)
def halo_rows_bound(H, W, bm=BM):
    """conv3x3.hip halo_rows_bound: the host's upper bound of the padded-halo rows Q of a ``bm``-pixel tile."""
    rows = (bm - 1) // W + 2
    imgs = 2 if rows <= H else (rows - 1) // H + 2
    return (rows + 2 * imgs) * (W + 2)


def halo_rows_need(N, H, W, bm=BM):
    """The largest Q any tile of an N-image input needs, by the kernels' own pr0 / Q formulas."""
    HW, M, H2, W2 = H * W, N * H * W, H + 2, W + 2
    need = 0
    for m0 in range(0, M, bm):
        mlast = min(m0 + bm, M) - 1
        pr0 = (m0 // HW) * H2 + (m0 % HW) // W
        need = max(need, ((mlast // HW) * H2 + (mlast % HW) // W + 2 - pr0 + 1) * W2)
    return need


def s1_variant(N, H, W, Ci, Co, opt=41, small_grid=256):
    """conv3x3.hip variant_of: the stride-1 forward's dispatch (``small_grid``: PDT_SMALL_GRID_NARROW's threshold)."""
    if opt & 32 and Ci == 64 and Co == 64 and W == 56 and H % 4 == 0 and N * (H // 4) >= 256:
        return "wsr"
    if Ci == 64 and Co == 64:
        if halo_rows_bound(H, W) <= 640:
            return "wst"
    elif halo_rows_bound(H, W) <= 512:
        wide = Co % 128 == 0 and not (N * H * W + 255) // 256 * (Co // 128) < small_grid
        return "halo_wide" if wide else "halo_narrow"
    return "tap_wide" if Co % 128 == 0 else "tap_narrow"


def wgrad_rows_per_tile(W):
    return max(1, (112 + W // 2) // W)


def wgrad_halo_rows(R, H, W, stride=1, Hi=0, Wi=0):
    """conv3x3_wgrad.hip halo_rows: the host's bound of a tile's halo rows (H, W: OUTPUT size)."""
    o = 0
    if stride == 1:
        imgs = 1
        for _ in range(H):
            imgs = max(imgs, (o + R - 1) // H + 1)
            o = (o + R) % H
        return (R + 2 * imgs) * ((W + 2 + 3) & ~3)
    rows = 0
    for _ in range(H):
        last = o + R - 1
        rows = max(rows, (last // H) * (Hi + 2) + 2 * (last % H) + 2 - 2 * o + 1)
        o = (o + R) % H
    return rows * 2 * (((Wi + 3) // 2 + 3) & ~3)


def wgrad_halo_need(N, R, H, W, stride=1, Hi=0, Wi=0):
    """The most halo rows any tile of the weight gradient's tile table stages (the kernel's load_tile: nh)."""
    if stride == 1:
        Hi, Wi = H, W
    W2 = (W + 2 + 3) & ~3 if stride == 1 else 2 * (((Wi + 3) // 2 + 3) & ~3)
    H2, need = Hi + 2, 0
    for g0, g1 in wgrad_tiles(N, H, R):
        gl = g1 - 1
        prs = (g0 // H) * H2 + stride * (g0 % H)
        pre = (gl // H) * H2 + stride * (gl % H) + 2
        need = max(need, (pre - prs + 1) * W2)
    return need


def wgrad_geo(N, H, W, Ci, Co, stride, target_wgs=0, co_tile=0):
    """conv3x3_wgrad.hip geo_of at the INPUT size H x W: (R, ntiles, tiles_per_split, nsplit, co_tile) or None."""
    if Ci % 64 or Co % 64 or N < 1 or H < stride or W < stride or N * H * W * max(Ci, Co) >= 2 ** 31:
        return None
    if stride == 1:
        co_t = co_tile if co_tile == 64 or (co_tile == 128 and Co % 128 == 0) else (128 if Co % 128 == 0 else 64)
    else:
        co_t = 64 if co_tile == 64 or Co % 128 else 128
    target = target_wgs if target_wgs > 0 else (256 if co_t == 128 else 512)
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    hmax, kpmax = (256, 128) if stride == 1 else (320, 64)
    R = wgrad_rows_per_tile(Wo)
    while R > 1 and (wgrad_halo_rows(R, Ho, Wo, stride, H, W) > hmax or ((R * Wo + 15) & ~15) > kpmax):
        R -= 1
    if ((R * Wo + 15) & ~15) > kpmax or wgrad_halo_rows(R, Ho, Wo, stride, H, W) > hmax:
        return None
    ntiles = (N * Ho + R - 1) // R
    nblk = (Co // co_t) * (Ci // 64)
    ns = max(1, min((target + nblk - 1) // nblk, ntiles))
    tps = (ntiles + ns - 1) // ns
    return R, ntiles, tps, (ntiles + tps - 1) // tps, co_t
