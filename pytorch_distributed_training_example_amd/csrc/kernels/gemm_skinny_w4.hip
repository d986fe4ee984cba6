// W4A16 weight-streaming skinny GEMM for gfx950 on group-wise int4 weights, and the quantiser that packs them.
//   mode 0: Y[m, n] = bf16(sum_g scale[g, n] * (sum_{k in group g} X[m, k] q[n, k]))                     [M, N]
//   mode 1: SwiGLU of that on packed [gate; up] rows, from the two bf16-rounded values                   [M, N / 2]
// X [M, K] bf16; q [N, K] integers in [-7, 7] stored as two's-complement nibbles in Wq [N, K / 2] bytes (layout
// below); scale [K / 128, N] fp32, group-major: one per (128 consecutive k, output feature). 1 <= M <= 64,
// N % 16 == 0 (mode 1: N % 32 == 0), K % 256 == 0, K < 2^24, Wq below 2^31 bytes, everything row-contiguous and
// 16-byte aligned. The inner sum is the MFMA unit's fp32 on exact bf16 operands (no scale is folded into an
// operand); the outer sum is one fp32 fma per group, in group order; one rounding per output (after the split
// combine when S > 1). No atomics: the order of summation is a function of (M, N, K, S) only.
//
// The third member of the skinny family (gemm_skinny.hip: bf16, gemm_skinny_w8.hip: e4m3 with a scale per
// row). A scale per group cannot wait until the whole sum is done, so the accumulation has two levels, and
// that decides the byte layout, which the quantiser writes for this kernel:
//   W   A weight row's 128-byte line holds 256 k: one K step, two groups. Lane (c, g) = (lane & 15, lane >> 4)
//       loads bytes [32 g, 32 g + 32) of row c's line (two 16-byte non-temporal loads). Word i (0..7) of those
//       bytes holds the eight values k = 256 s + 32 i + 8 g + j, j = 0..7: it is the lane's A operand of
//       v_mfma_f32_16x16x32_bf16 number i of the step, and that MFMA contracts over the contiguous block
//       k = 256 s + 32 i .. + 31. MFMAs 0-3 are group 2 s (the first load), MFMAs 4-7 group 2 s + 1 (the second):
//       no MFMA mixes two groups. Within a word nibble t holds j = 2 t and nibble t + 4 holds j = 2 t + 1, so a
//       bf16 pair is two extracts of one word at shifts 4 t and 4 t + 16.
//   cvt int4 -> bf16 in registers, exactly (|q| <= 8 has 4 significant bits): v_bfe_i32 (sign-extending
//       extract), v_cvt_f32_i32, and one v_cvt_pk_bf16_f32 per pair: 2.5 VALU operations per value, done right
//       before the item's MFMAs, behind the loads of the items after it.
//   X   standard B-operand placement: for MFMA i lane (c, g) loads the 16 bytes x[16 t + c][256 s + 32 i + 8 g ..],
//       buffer loads over a resource of M rows (a token column at or past M reads zero in hardware). 8 fragments
//       per step and column tile, held per chunk and reused by the wave's FT feature tiles.
//   acc Per group and column tile four chained MFMAs start from a zero C; then four fp32 fmas per lane,
//       acc[r] += part[r] * scale[group, n0 + 4 g + r]: the accumulator layout gives a lane four consecutive
//       features of one token, so its four scales are one 16-byte load (the same address across a lane group),
//       which is why scale is group-major. The scale loads are issued with the item's weight loads.
// Geometry. A chunk is one 256-wide step, so K = 1024 still gives each of the four waves a chunk. An item
// (chunk x feature tile) is 2 x 16 bytes of weights per lane, 2 KB per wave, plus its 2 x 16 bytes of scales:
// 16 VGPRs. A wave runs a ring of eight item buffers (128 VGPRs) and requests item i + 7 before it converts and
// multiplies item i: 14 KB of weights per wave in flight against the W8 kernel's 12. The ring index is static:
// items are flattened as i = FT * (chunk turn) + ft and the loop is unrolled by eight, which FT in {1, 2, 4}
// divides. NT 1 (a decode step) is bounded to 256 registers, two waves per SIMD. NT 2 and 4 hold 64 and 128 VGPRs
// of X beside the ring's 128 and spilled at that bound (52-87 VGPRs), so they are bounded to one wave per SIMD
// (512 registers, accumulators in AGPRs) and stay out of scratch: profiles/r26/skinny_w4_gemm.txt.
// A workgroup is 4 waves that own FT feature tiles and one range of chunks (all of K when S == 1), taken
// round-robin (wave w: chunks w, w + 4, ...). No LDS and no barrier in the loop. The four waves' fp32 tiles are
// merged through LDS in wave order 0..3 behind one barrier, wave w finishing output tiles w, w + 4, ...; the merge
// rounds and stores, or (S > 1) stores the fp32 tile, already scaled, to ws [S, M, N] for
// gemm_skinny_w4_combine_kernel, which adds the partials in split order and rounds once.
// MODE_SWIGLU: as in the siblings, feature tiles come in (gate, up) pairs, both are rounded to bf16 and
// swiglu_fwd2 is applied to the rounded values. Every kernel here is compiled without the packed fp32
// instructions, so the epilogue's bits equal swiglu.hip's on this kernel's own unfused output.
//
// pdt_gemm_skinny_w4_geo(M, N, K, mode, splits) -> (S, FT, NT), a pure function of its arguments, the family's rule
// on 256-wide chunks:
//   NT  the smallest of 1, 2, 4 with 16 NT >= M.
//   FT  from {1, 2, 4} ({2, 4} in MODE_SWIGLU) with FT NT <= 8: the largest that still gives 512 workgroups, else
//       the smallest.
//   S   1 when there are at least 256 workgroups or splits == 1; otherwise ceil(256 / groups), at most nch / 2
//       and at most 16. splits > 0 asks for that many (at most nch come out).
//
// pdt_quant_groups_int4: w [N, K] bf16 -> Wq, scale; one wave per (row, line), fp32 throughout: amax over the
// 128-element group, scale = amax * (1 / 7) (1 for a zero group), inv = 7 / amax (0 for a zero group),
// q = clamp(rint(w * inv), -7, 7) with ties to even, written straight into the packed layout; ops/linear.py
// computes the same bytes in torch.
#include "../common.h"
#include "../launchers.h"
#include "../swiglu_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int CHUNK = 256;             // k per chunk: one 128-byte line of a weight row, two groups, 8 MFMAs
constexpr int GROUP = 128;             // k per scale
constexpr int RING = 8;                // item buffers per wave; RING - 1 items are in flight ahead of the MFMAs
constexpr uint32_t OOB = 0x80000000u;  // a buffer offset past any operand: the load returns zero
constexpr int W_NT = 2;                // aux bits of the W loads: nt (non-temporal)
enum { MODE_NONE = 0, MODE_SWIGLU = 1 };

#if defined(__HIP_DEVICE_COMPILE__)
#define PDT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PDT_NO_PACKED_F32
#endif

// (a function with a target feature of its own inlines only what is always_inline: __syncthreads is not)
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int AUX>
__device__ __forceinline__ u4 load16(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, AUX);
}

// One item: the lane's 32 bytes of one line of a W row (w[h]: words 4 h .. 4 h + 3, group h of the chunk) and its
// four scales of either group.
struct Item {
  u4 w[2];
  f4 s[2];
};

__device__ __forceinline__ void load_item(Item& it, __amdgpu_buffer_rsrc_t wrs, __amdgpu_buffer_rsrc_t srs,
                                          uint32_t wrow, uint32_t srow, int chunk, uint32_t srow_bytes) {
  const bool in = wrow != OOB;
  const uint32_t woff = in ? wrow + 128u * (uint32_t)chunk : OOB;
  const uint32_t soff = in ? srow + 2u * (uint32_t)chunk * srow_bytes : OOB;
  it.w[0] = load16<W_NT>(wrs, woff);
  it.w[1] = load16<W_NT>(wrs, woff + 16);
  it.s[0] = __builtin_bit_cast(f4, load16<0>(srs, soff));
  it.s[1] = __builtin_bit_cast(f4, load16<0>(srs, in ? soff + srow_bytes : OOB));
}

// The 8 X fragments of a chunk of one row: fragment i is the 16 bytes at 64 i of the lane's slice.
__device__ __forceinline__ void load_x_chunk(bf16x8 (&f)[8], __amdgpu_buffer_rsrc_t rs, uint32_t row_off, int chunk) {
  const uint32_t off = row_off + 512u * (uint32_t)chunk;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = __builtin_bit_cast(bf16x8, load16<0>(rs, off + 64 * i));
}

// One word: 8 two's-complement nibbles -> 8 bf16, exactly; value j = 2 t is nibble t, j = 2 t + 1 nibble t + 4.
__device__ __forceinline__ bf16x8 cvt8(uint32_t w) {
  bf16x8 r;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f2 p = f2{(float)((int)(w << (28 - 4 * t)) >> 28), (float)((int)(w << (12 - 4 * t)) >> 28)};
    const bf16x2 b = __builtin_convertvector(p, bf16x2);
    r[2 * t] = b[0];
    r[2 * t + 1] = b[1];
  }
  return r;
}

__device__ __forceinline__ f4 round_bf16(f4 v) {
  return f4{bf2f(f2bf(v[0])), bf2f(f2bf(v[1])), bf2f(f2bf(v[2])), bf2f(f2bf(v[3]))};
}

// swiglu.hip's values for four consecutive features: pairs (0, 1) and (2, 3) of the bf16-rounded gate and up
__device__ __forceinline__ void swiglu4(f4 gate, f4 up, float (&o)[4]) {
  const f4 g = round_bf16(gate), u = round_bf16(up);
  const gf2 a = swiglu_fwd2(gf2{g[0], g[1]}, gf2{u[0], u[1]});
  const gf2 b = swiglu_fwd2(gf2{g[2], g[3]}, gf2{u[2], u[3]});
  o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
}

// First W row of feature tile ft of workgroup blk, or -1 past the end. MODE_SWIGLU: tiles 2p, 2p + 1 are the
// gate and up tiles of pair p.
template <int FT, int MODE>
__device__ __forceinline__ int tile_row0(int blk, int ft, int N) {
  if (MODE == MODE_SWIGLU) {
    const int F = N >> 1, n0 = (blk * (FT / 2) + (ft >> 1)) * 16;
    return n0 < F ? n0 + ((ft & 1) ? F : 0) : -1;
  }
  const int n0 = (blk * FT + ft) * 16;
  return n0 < N ? n0 : -1;
}

template <int NT, int FT, int MODE>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256, NT == 1 ? 2 : 1) void gemm_skinny_w4_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const float* __restrict__ scale,
    uint16_t* __restrict__ y, float* __restrict__ ws, int M, int N, int K) {
  static_assert(FT * NT <= 8 && RING % FT == 0 && (MODE == MODE_NONE || FT % 2 == 0), "gemm_skinny_w4: instantiation");
  __shared__ f4 red[4][FT * NT][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int blk = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
  const int nch = K / CHUNK;
  const int cb = (int)((int64_t)sp * nch / S), ce = (int)((int64_t)(sp + 1) * nch / S);
  const uint32_t wrow_bytes = (uint32_t)K >> 1, srow_bytes = 4u * (uint32_t)N;
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), (short)0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(w), (short)0, N * (K >> 1), 0x00020000);
  const __amdgpu_buffer_rsrc_t srs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(scale), (short)0, (K / GROUP) * N * 4, 0x00020000);

  // byte offsets of the lane's slice within chunk 0: W row c of each feature tile (32 bytes), its four scales of
  // group 0 (features r0 + 4 g ..), X row 16 j + c (16 bytes per MFMA)
  uint32_t wrow[FT], srow[FT], xrow[NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    const int r0 = tile_row0<FT, MODE>(blk, ft, N);
    wrow[ft] = r0 >= 0 ? (uint32_t)(r0 + c) * wrow_bytes + 32u * g : OOB;
    srow[ft] = r0 >= 0 ? 4u * (uint32_t)(r0 + 4 * g) : OOB;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) xrow[j] = (uint32_t)(16 * j + c) * (uint32_t)K * 2u + 16u * g;  // row >= M: past the end

  f4 acc[FT][NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[ft][j] = f4{0.f, 0.f, 0.f, 0.f};

  // ---- the K loop over this wave's items i = FT * turn + ft (chunk cb + wv + 4 turn): item i + RING - 1's bytes
  // are requested before item i's are converted and multiplied. i0 % RING == 0, so ring slot and ft are static.
  const int turns = ce > cb + wv ? (ce - cb - wv + 3) / 4 : 0, items = turns * FT;
  Item ring[RING];
  bf16x8 xf[NT][8];
#pragma unroll
  for (int u = 0; u < RING - 1; ++u)
    if (u < items) load_item(ring[u], wrs, srs, wrow[u % FT], srow[u % FT], cb + wv + 4 * (u / FT), srow_bytes);
  for (int i0 = 0; i0 < items; i0 += RING) {
#pragma unroll
    for (int u = 0; u < RING; ++u) {
      const int i = i0 + u;
      if (i < items) {
        constexpr int AHEAD = RING - 1;
        const int ft = u % FT, chunk = cb + wv + 4 * (i / FT);
        if (i + AHEAD < items)
          load_item(ring[(u + AHEAD) % RING], wrs, srs, wrow[(u + AHEAD) % FT], srow[(u + AHEAD) % FT],
                    cb + wv + 4 * ((i + AHEAD) / FT), srow_bytes);
        if (ft == 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j) load_x_chunk(xf[j], xrs, xrow[j], chunk);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // one group: four MFMAs from a zero C, then the scale
          const u4 b = ring[u].w[h];
          const f4 s = ring[u].s[h];
          const bf16x8 a0 = cvt8(b[0]), a1 = cvt8(b[1]), a2 = cvt8(b[2]), a3 = cvt8(b[3]);
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            f4 part = f4{0.f, 0.f, 0.f, 0.f};
            part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf[j][4 * h], part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf[j][4 * h + 1], part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, xf[j][4 * h + 2], part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, xf[j][4 * h + 3], part, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ft][j][r] = __builtin_fmaf(part[r], s[r], acc[ft][j][r]);
          }
        }
      }
    }
  }

  // ---- merge the four waves in wave order; wave w finishes output tiles w, w + 4, ...
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int j = 0; j < NT; ++j) red[wv][ft * NT + j][lane] = acc[ft][j];
  block_barrier();
  constexpr int UNITS = (MODE == MODE_SWIGLU ? FT / 2 : FT) * NT;
  for (int u = wv; u < UNITS; u += 4) {
    const int fu = u / NT, j = u - fu * NT;  // feature tile (or pair) and column tile
    const int tok = 16 * j + c;
    const int ft = MODE == MODE_SWIGLU ? 2 * fu : fu;
    const int r0 = tile_row0<FT, MODE>(blk, ft, N);
    f4 a = red[0][ft * NT + j][lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) a += red[ww][ft * NT + j][lane];
    f4 b = f4{0.f, 0.f, 0.f, 0.f};
    if (MODE == MODE_SWIGLU) {
      b = red[0][(ft + 1) * NT + j][lane];
#pragma unroll
      for (int ww = 1; ww < 4; ++ww) b += red[ww][(ft + 1) * NT + j][lane];
    }
    if (r0 < 0 || tok >= M) continue;
    if (S > 1) {
      float* p = ws + ((int64_t)sp * M + tok) * N + r0 + 4 * g;
      *reinterpret_cast<f4*>(p) = a;
      if (MODE == MODE_SWIGLU) *reinterpret_cast<f4*>(p + (N >> 1)) = b;
    } else if (MODE == MODE_SWIGLU) {
      float o[4];
      swiglu4(a, b, o);
      Vec4<uint16_t>::st(y, (int64_t)tok * (N >> 1) + r0 + 4 * g, o);
    } else {
      const float o[4] = {a[0], a[1], a[2], a[3]};
      Vec4<uint16_t>::st(y, (int64_t)tok * N + r0 + 4 * g, o);
    }
  }
}

// One thread per 4 consecutive outputs: the S scaled partials in split order, one rounding.
template <int MODE>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void gemm_skinny_w4_combine_kernel(
    const float* __restrict__ ws, uint16_t* __restrict__ y, int M, int N, int S) {
  const int NO = MODE == MODE_SWIGLU ? N >> 1 : N;  // output row length
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M * (NO >> 2)) return;
  const int m = i / (NO >> 2), n = (i - m * (NO >> 2)) * 4;
  const float* p = ws + (int64_t)m * N + n;
  const int64_t stride = (int64_t)M * N;
  f4 a = *reinterpret_cast<const f4*>(p);
  for (int s = 1; s < S; ++s) a += *reinterpret_cast<const f4*>(p + s * stride);
  float o[4] = {a[0], a[1], a[2], a[3]};
  if (MODE == MODE_SWIGLU) {
    f4 b = *reinterpret_cast<const f4*>(p + NO);
    for (int s = 1; s < S; ++s) b += *reinterpret_cast<const f4*>(p + NO + s * stride);
    swiglu4(a, b, o);
  }
  Vec4<uint16_t>::st(y, (int64_t)m * NO + n, o);
}

// One wave per (row, line), 4 per workgroup. Lane l < 32 takes the eight values k = 256 s + 8 l .. + 7: the word
// (i, g) = (l >> 2, l & 3) of the packed line; lanes 0-15 are the line's first group, 16-31 its second. Lanes
// 32-63 mirror them and store nothing.
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void quant_groups_int4_kernel(const uint16_t* __restrict__ w,
                                                                                  uint8_t* __restrict__ wq,
                                                                                  float* __restrict__ scale, int N,
                                                                                  int K) {
  const int lane = threadIdx.x & 63, l = lane & 31, lines = K / CHUNK;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= (int64_t)N * lines) return;
  const int n = (int)(unit / lines), s = (int)(unit - (int64_t)n * lines);
  float v[8];
  ld8_bf16(w + (int64_t)n * K + CHUNK * s + 8 * l, v);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[i]));
#pragma unroll
  for (int b = 3; b >= 0; --b) {  // over the 16 lanes of the group
    const int other = __builtin_amdgcn_ds_bpermute((lane ^ (1 << b)) << 2, __builtin_bit_cast(int, amax));
    amax = __builtin_fmaxf(amax, __builtin_bit_cast(float, other));
  }
  const float inv = amax > 0.f ? 7.0f / amax : 0.f;
  if (lane == 0 || lane == 16) scale[(int64_t)(2 * s + (lane >> 4)) * N + n] = amax > 0.f ? amax * (1.0f / 7.0f) : 1.0f;
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float q = __builtin_fminf(__builtin_fmaxf(__builtin_rintf(v[j] * inv), -7.f), 7.f);
    word |= ((uint32_t)(int)q & 15u) << (4 * (j >> 1) + 16 * (j & 1));
  }
  if (lane < 32)
    *reinterpret_cast<uint32_t*>(wq + (int64_t)n * (K >> 1) + 128 * s + 32 * (l & 3) + 4 * (l >> 2)) = word;
}

template <int NT, int FT, int MODE>
void launch(dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* w, const float* scale, uint16_t* y, float* ws,
            int M, int N, int K) {
  hipLaunchKernelGGL((gemm_skinny_w4_kernel<NT, FT, MODE>), grid, dim3(256), 0, s, x, w, scale, y, ws, M, N, K);
}

// The instantiations: FT in {1, 2, 4} ({2, 4} in MODE_SWIGLU) with FT NT <= 8; the caller has checked FT.
template <int NT, int MODE>
void launch_ft(int FT, dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* w, const float* scale, uint16_t* y,
               float* ws, int M, int N, int K) {
  if constexpr (MODE == MODE_NONE)
    if (FT == 1) return launch<NT, 1, MODE>(grid, s, x, w, scale, y, ws, M, N, K);
  if constexpr (NT <= 2)
    if (FT == 4) return launch<NT, 4, MODE>(grid, s, x, w, scale, y, ws, M, N, K);
  launch<NT, 2, MODE>(grid, s, x, w, scale, y, ws, M, N, K);
}

}  // namespace

extern "C" {

// w [N, K] bf16 row-contiguous, 16-byte aligned, K % 256 == 0 -> wq [N, K / 2] packed nibbles, scale [K / 128, N].
int pdt_quant_groups_int4(const uint16_t* w, uint8_t* wq, float* scale, int N, int K, hipStream_t s) {
  if (N < 1 || K < CHUNK || K % CHUNK != 0) return -1;
  const int64_t units = (int64_t)N * (K / CHUNK);
  if ((units + 3) / 4 > 0x7fffffffLL) return -3;
  hipLaunchKernelGGL(quant_groups_int4_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, w, wq, scale, N, K);
  return 0;
}

// (S, FT, NT) into geo3: the rule in this file's header. -1: outside the contract; -3: Wq past 2^31 bytes or
// K past 2^24.
int pdt_gemm_skinny_w4_geo(int M, int N, int K, int mode, int splits, int* geo3) {
  if (M < 1 || M > 64 || N < 16 || N % 16 != 0 || K < CHUNK || K % CHUNK != 0 || splits < 0) return -1;
  if (mode != MODE_NONE && mode != MODE_SWIGLU) return -1;
  if (mode == MODE_SWIGLU && N % 32 != 0) return -1;
  if ((int64_t)N * (K / 2) >= 0x80000000LL || K >= (1 << 24)) return -3;
  const int NT = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  const int T = N / 16, ftmin = mode == MODE_SWIGLU ? 2 : 1, ftmax = 8 / NT < 4 ? 8 / NT : 4;
  int FT = ftmin;
  for (int ft = ftmax; ft > ftmin; ft >>= 1)
    if ((T + ft - 1) / ft >= 512) {
      FT = ft;
      break;
    }
  const int groups = (T + FT - 1) / FT, nch = K / CHUNK;
  int S = splits;
  if (S == 0) {
    S = 1;
    if (groups < 256) {
      S = (256 + groups - 1) / groups;
      if (S > nch / 2) S = nch / 2;
      if (S > 16) S = 16;
      if (S < 1) S = 1;
    }
  }
  if (S > nch) S = nch;
  geo3[0] = S;
  geo3[1] = FT;
  geo3[2] = NT;
  return 0;
}

// x [M, K] bf16, wq [N, K / 2] packed nibbles, scale [K / 128, N] fp32, all row-contiguous and 16-byte aligned.
// mode 0: y [M, N]; mode 1 (SwiGLU, wq = [gate; up] rows): y [M, N / 2]. (S, FT, NT) as pdt_gemm_skinny_w4_geo
// returns them (any S in [1, nch] and any served FT are accepted); S > 1 needs ws, S M N floats, and launches
// the combine.
int pdt_gemm_skinny_w4(const uint16_t* x, const uint8_t* wq, const float* scale, uint16_t* y, float* ws, int M, int N,
                       int K, int mode, int S, int FT, int NT, hipStream_t s) {
  int geo[3];
  const int rc = pdt_gemm_skinny_w4_geo(M, N, K, mode, 0, geo);
  if (rc != 0) return rc;
  const int nch = K / CHUNK;
  if (NT != geo[2] || S < 1 || S > nch || S > 65535) return -2;
  if ((FT != 1 && FT != 2 && FT != 4) || FT * NT > 8 || (mode == MODE_SWIGLU && FT == 1)) return -2;
  if (S > 1 && !ws) return -4;
  const dim3 grid((N / 16 + FT - 1) / FT, S);
  if (mode == MODE_NONE) {
    if (NT == 1) launch_ft<1, MODE_NONE>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
    else if (NT == 2) launch_ft<2, MODE_NONE>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
    else launch_ft<4, MODE_NONE>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
  } else {
    if (NT == 1) launch_ft<1, MODE_SWIGLU>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
    else if (NT == 2) launch_ft<2, MODE_SWIGLU>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
    else launch_ft<4, MODE_SWIGLU>(FT, grid, s, x, wq, scale, y, ws, M, N, K);
  }
  if (S > 1) {
    const int items = M * ((mode == MODE_SWIGLU ? N / 2 : N) / 4);
    const dim3 cgrid((items + 255) / 256);
    if (mode == MODE_SWIGLU)
      hipLaunchKernelGGL(gemm_skinny_w4_combine_kernel<MODE_SWIGLU>, cgrid, dim3(256), 0, s, ws, y, M, N, S);
    else
      hipLaunchKernelGGL(gemm_skinny_w4_combine_kernel<MODE_NONE>, cgrid, dim3(256), 0, s, ws, y, M, N, S);
  }
  return 0;
}

}  // extern "C"
