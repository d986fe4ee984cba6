// W8A16 weight-streaming skinny GEMM for gfx950 and the row-wise quantiser that feeds it.
//   mode 0: Y[m, n] = bf16(scale[n] * sum_k X[m, k] float(Wq[n, k]))                                      [M, N]
//   mode 1: SwiGLU of that on packed [gate; up] rows, from the two bf16-rounded values                     [M, N / 2]
// X [M, K] bf16, Wq [N, K] OCP e4m3fn, scale [N] fp32 (one per output feature), 1 <= M <= 64, N % 16 == 0
// (mode 1: N % 32 == 0), K % 128 == 0, row-contiguous and 16-byte aligned, N K < 2^31 bytes, K < 2^24 (32-bit
// buffer offsets for 64 rows of X). fp32 accumulation, one fp32 multiply by scale[n] after the whole sum (after
// the split combine when S > 1), one rounding per output. No atomics: the order of summation is a function of
// (M, N, K, S) only.
//
// The bf16 kernel (gemm_skinny.hip) streams weights to the matrix cores' registers with no LDS in the K loop;
// this is that idea laid out again for one-byte weights. What changes is the line: a weight row's 128-byte line
// holds 128 k values instead of 64, and every byte needs one VALU conversion before an MFMA can use it.
//   W   global -> registers as bytes. One K step is 128 wide: lane (c, g) = (lane & 15, lane >> 4) loads the 32
//       contiguous bytes [32 g, 32 g + 32) of row c's line (two 16-byte loads), so lanes c, c + 16, c + 32, c + 48
//       cover it. The 32 values become four v_mfma_f32_16x16x32_bf16 A operands: operand i of step s holds
//       k = 128 s + 32 g + 8 i + j in slot j. Non-temporal, the bf16 kernel's choice; no A/B was measured
//       for this kernel, so there is no tune entry.
//   cvt e4m3 -> bf16 is exact (4 significant bits into 8, the exponent range is inside bf16's):
//       v_cvt_pk_f32_fp8 on a byte pair, v_cvt_pk_bf16_f32 on the two floats, one VALU instruction per value
//       on average. An item's 64 values per lane are converted right before its MFMAs, which is after the loads of
//       the items behind it have been issued: the VALU work runs under memory latency, not in front of it.
//   X   small and L2-resident, buffer loads over a resource of M rows (a token column at or past M reads zero in
//       hardware, whatever follows X in memory). Same placement as W: per step lane (c, g) loads the 64
//       contiguous bytes of row c that hold k = 128 s + 32 g .. + 31 (four 16-byte loads, one per MFMA). A dot
//       product does not care where its terms sit as long as both operands agree.
// Geometry. A chunk is 256 k (two steps): K = 1024 still has four chunks, one per wave, where a 512-wide chunk
// would leave two of llama_medium's four waves without work. An item is one chunk of one feature tile: 4 loads
// of 16 bytes per lane, 4 KB per wave, 8 MFMAs per column tile. To keep the bf16 kernel's bytes in flight with
// items half its size, a wave runs a ring of four item buffers (16 VGPRs each, 64 in all: what the bf16 kernel
// spends on its two) and issues item i + 3's loads before it converts and multiplies item i: 12 KB per wave are
// in flight against the bf16 kernel's 8. X is held per chunk (8 NT fragments, 32 NT VGPRs) and reused by the
// wave's FT feature tiles. The ring index is static: items are flattened as i = FT * (chunk turn) + ft and
// the loop is unrolled by four, which FT in {1, 2, 4} divides. __launch_bounds__(256, 2) holds the widest
// instantiation (NT 4, FT 2: 128 VGPRs of X, 64 of ring, 32 accumulators, the converted operands) to 256 registers,
// two waves per SIMD, without scratch; left alone the compiler took 268 and one wave (profiles/r22/skinny_w8_gemm.txt).
// A workgroup is 4 waves that own FT feature tiles and one range of chunks (all of K when S == 1), taken
// round-robin (wave w: chunks w, w + 4, ...; the count need not divide by 4 and K % 256 may be 128: a step at or
// past K is loaded from an out-of-range offset, zero, for both operands). No barrier in the loop. The four
// waves' fp32 tiles are merged through LDS in wave order 0..3 behind one barrier, wave w finishing output tiles
// w, w + 4, ...; the merge multiplies by scale[n], rounds and stores, or (S > 1) stores the unscaled fp32 tile to
// ws [S, M, N] for gemm_skinny_w8_combine_kernel, which adds the partials in split order, multiplies by
// scale[n] and rounds once.
// MODE_SWIGLU: as in the bf16 kernel, feature tiles come in (gate, up) pairs, both are rounded to bf16 and
// swiglu_fwd2 is applied to the rounded values. Every kernel here is compiled without the packed fp32
// instructions (per-function target feature); the forward formula has nothing to contract, so its bits equal
// swiglu.hip's on this kernel's own unfused output (tests/test_gemm_skinny_w8_gpu.py asserts it).
//
// pdt_gemm_skinny_w8_geo(M, N, K, mode, splits) -> (S, FT, NT), a pure function of its arguments:
//   NT  the smallest of 1, 2, 4 with 16 NT >= M.
//   FT  from {1, 2, 4} ({2, 4} in MODE_SWIGLU) with FT NT <= 8: the largest that still gives 512 workgroups, else
//       the smallest (the bf16 kernel's rule: a larger FT amortises the X fragments, but not at the price of
//       idle CUs).
//   S   1 when there are at least 256 workgroups or splits == 1; otherwise ceil(256 / groups), at most nch / 2
//       and at most 16. splits > 0 asks for that many (at most nch come out).
//
// pdt_quant_rows_e4m3: w [N, K] bf16 -> wq [N, K] e4m3, scale [N]; one wave per row, two passes. fp32 throughout:
// amax = max |w|, scale = amax * (1 / 448) (1 when amax == 0), inv = 448 / amax (0 when amax == 0),
// wq = e4m3_rne(clamp(w * inv, -448, 448)); the CPU path of ops/linear.py computes the same bytes.
#include "../common.h"
#include "../fp8_pack.h"
#include "../launchers.h"
#include "../swiglu_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int STEP = 128;              // k per step: one 128-byte line of a weight row
constexpr int CHUNK = 256;             // k per chunk: 2 steps, 4 W loads and 8 MFMAs per feature and column tile
constexpr int RING = 4;                // item buffers per wave; RING - 1 items are in flight ahead of the MFMAs
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

// One item: the lane's 2 x 32 bytes of a 256-wide chunk of a W row; f[2 s], f[2 s + 1] are step s. A step at or
// past K is read from OOB.
__device__ __forceinline__ void load_w_item(u4 (&f)[4], __amdgpu_buffer_rsrc_t rs, uint32_t row_off, int k0, int K) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = k0 + STEP * s;
    const uint32_t off = k < K ? row_off + (uint32_t)k : OOB;
    f[2 * s] = load16<W_NT>(rs, off);
    f[2 * s + 1] = load16<W_NT>(rs, off + 16);
  }
}

// The 8 X fragments of a chunk of one row: fragment 4 s + i is the 16 bytes at 256 s + 16 i of the lane's slice.
__device__ __forceinline__ void load_x_chunk(bf16x8 (&f)[8], __amdgpu_buffer_rsrc_t rs, uint32_t row_off, int k0,
                                             int K) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = k0 + STEP * s;
    const uint32_t off = k < K ? row_off + 2u * (uint32_t)k : OOB;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[4 * s + i] = __builtin_bit_cast(bf16x8, load16<0>(rs, off + 16 * i));
  }
}

// 8 e4m3 bytes (two words) -> 8 bf16, exactly, in byte order
__device__ __forceinline__ bf16x8 cvt8(uint32_t lo, uint32_t hi) {
  const bf16x2 a = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), bf16x2);
  const bf16x2 b = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true), bf16x2);
  const bf16x2 c = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), bf16x2);
  const bf16x2 d = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true), bf16x2);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
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

__device__ __forceinline__ f4 scaled(f4 a, const float* __restrict__ scale, int n) {
  const f4 s = *reinterpret_cast<const f4*>(scale + n);  // n % 4 == 0
  return f4{a[0] * s[0], a[1] * s[1], a[2] * s[2], a[3] * s[3]};
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
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256, 2) void gemm_skinny_w8_kernel(
    const uint16_t* __restrict__ x, const uint8_t* __restrict__ w, const float* __restrict__ scale,
    uint16_t* __restrict__ y, float* __restrict__ ws, int M, int N, int K) {
  static_assert(FT * NT <= 8 && RING % FT == 0 && (MODE == MODE_NONE || FT % 2 == 0), "gemm_skinny_w8: instantiation");
  __shared__ f4 red[4][FT * NT][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int blk = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
  const int nch = (K + CHUNK - 1) / CHUNK;
  const int cb = (int)((int64_t)sp * nch / S), ce = (int)((int64_t)(sp + 1) * nch / S);
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), (short)0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(w), (short)0, N * K, 0x00020000);

  // byte offsets of the lane's slice within step 0: W row c of each feature tile (32 bytes), X row 16 j + c (64)
  uint32_t wrow[FT], xrow[NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    const int r0 = tile_row0<FT, MODE>(blk, ft, N);
    wrow[ft] = r0 >= 0 ? (uint32_t)(r0 + c) * (uint32_t)K + 32u * g : OOB;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) xrow[j] = (uint32_t)(16 * j + c) * (uint32_t)K * 2u + 64u * g;  // row >= M: past the end

  f4 acc[FT][NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[ft][j] = f4{0.f, 0.f, 0.f, 0.f};

  // ---- the K loop over this wave's items i = FT * turn + ft (chunk cb + wv + 4 turn): item i + RING - 1's bytes
  // are requested before item i's are converted and multiplied. i0 % RING == 0, so ring slot and ft are static.
  const int turns = ce > cb + wv ? (ce - cb - wv + 3) / 4 : 0, items = turns * FT;
  u4 ring[RING][4];
  bf16x8 xf[NT][8];
#pragma unroll
  for (int u = 0; u < RING - 1; ++u)
    if (u < items) load_w_item(ring[u], wrs, wrow[u % FT], (cb + wv + 4 * (u / FT)) * CHUNK, K);
  for (int i0 = 0; i0 < items; i0 += RING) {
#pragma unroll
    for (int u = 0; u < RING; ++u) {
      const int i = i0 + u;
      if (i < items) {
        constexpr int AHEAD = RING - 1;
        const int ft = u % FT, k0 = (cb + wv + 4 * (i / FT)) * CHUNK;
        if (i + AHEAD < items)
          load_w_item(ring[(u + AHEAD) % RING], wrs, wrow[(u + AHEAD) % FT], (cb + wv + 4 * ((i + AHEAD) / FT)) * CHUNK, K);
        if (ft == 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j) load_x_chunk(xf[j], xrs, xrow[j], k0, K);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // 16 bytes: two operands
          const u4 b = ring[u][q];
          const bf16x8 a0 = cvt8(b[0], b[1]), a1 = cvt8(b[2], b[3]);
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            acc[ft][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf[j][2 * q], acc[ft][j], 0, 0, 0);
            acc[ft][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf[j][2 * q + 1], acc[ft][j], 0, 0, 0);
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
      swiglu4(scaled(a, scale, r0 + 4 * g), scaled(b, scale, r0 + (N >> 1) + 4 * g), o);
      Vec4<uint16_t>::st(y, (int64_t)tok * (N >> 1) + r0 + 4 * g, o);
    } else {
      a = scaled(a, scale, r0 + 4 * g);
      const float o[4] = {a[0], a[1], a[2], a[3]};
      Vec4<uint16_t>::st(y, (int64_t)tok * N + r0 + 4 * g, o);
    }
  }
}

// One thread per 4 consecutive outputs: the S partials in split order, the scale, one rounding.
template <int MODE>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void gemm_skinny_w8_combine_kernel(
    const float* __restrict__ ws, const float* __restrict__ scale, uint16_t* __restrict__ y, int M, int N, int S) {
  const int NO = MODE == MODE_SWIGLU ? N >> 1 : N;  // output row length
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M * (NO >> 2)) return;
  const int m = i / (NO >> 2), n = (i - m * (NO >> 2)) * 4;
  const float* p = ws + (int64_t)m * N + n;
  const int64_t stride = (int64_t)M * N;
  f4 a = *reinterpret_cast<const f4*>(p);
  for (int s = 1; s < S; ++s) a += *reinterpret_cast<const f4*>(p + s * stride);
  a = scaled(a, scale, n);
  float o[4] = {a[0], a[1], a[2], a[3]};
  if (MODE == MODE_SWIGLU) {
    f4 b = *reinterpret_cast<const f4*>(p + NO);
    for (int s = 1; s < S; ++s) b += *reinterpret_cast<const f4*>(p + NO + s * stride);
    swiglu4(a, scaled(b, scale, NO + n), o);
  }
  Vec4<uint16_t>::st(y, (int64_t)m * NO + n, o);
}

// One wave per row (4 rows per workgroup). Pass 1: the row's amax; pass 2: 8 values per lane per turn -> 8 bytes.
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void quant_rows_e4m3_kernel(const uint16_t* __restrict__ w,
                                                                                uint8_t* __restrict__ wq,
                                                                                float* __restrict__ scale, int N,
                                                                                int K) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const uint16_t* row = w + (int64_t)n * K;
  float amax = 0.f;
  for (int k = 8 * lane; k < K; k += 512) {
    float v[8];
    ld8_bf16(row + k, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[i]));
  }
#pragma unroll
  for (int b = 5; b >= 0; --b) {  // (builtins: __shfl_xor and __float_as_int are not always_inline, see block_barrier)
    const int other = __builtin_amdgcn_ds_bpermute((lane ^ (1 << b)) << 2, __builtin_bit_cast(int, amax));
    amax = __builtin_fmaxf(amax, __builtin_bit_cast(float, other));
  }
  const float inv = e4m3_row_inv(amax);
  if (lane == 0) scale[n] = e4m3_row_scale(amax);
  uint8_t* out = wq + (int64_t)n * K;
  for (int k = 8 * lane; k < K; k += 512) {
    float v[8];
    ld8_bf16(row + k, v);
    uint2 o;
    o.x = pack4_fp8(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv);
    o.y = pack4_fp8(v[4] * inv, v[5] * inv, v[6] * inv, v[7] * inv);
    *reinterpret_cast<uint2*>(out + k) = o;
  }
}

template <int NT, int FT, int MODE>
void launch(dim3 grid, hipStream_t s, const uint16_t* x, const uint8_t* w, const float* scale, uint16_t* y, float* ws,
            int M, int N, int K) {
  hipLaunchKernelGGL((gemm_skinny_w8_kernel<NT, FT, MODE>), grid, dim3(256), 0, s, x, w, scale, y, ws, M, N, K);
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

// w [N, K] bf16 row-contiguous, 16-byte aligned, K % 8 == 0 -> wq [N, K] e4m3 (8-byte aligned rows), scale [N].
int pdt_quant_rows_e4m3(const uint16_t* w, uint8_t* wq, float* scale, int N, int K, hipStream_t s) {
  if (N < 1 || K < 8 || K % 8 != 0) return -1;
  hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((N + 3) / 4), dim3(256), 0, s, w, wq, scale, N, K);
  return 0;
}

// (S, FT, NT) into geo3: the rule in this file's header. -1: outside the contract; -3: W past 2^31 bytes or
// K past 2^24.
int pdt_gemm_skinny_w8_geo(int M, int N, int K, int mode, int splits, int* geo3) {
  if (M < 1 || M > 64 || N < 16 || N % 16 != 0 || K < STEP || K % STEP != 0 || splits < 0) return -1;
  if (mode != MODE_NONE && mode != MODE_SWIGLU) return -1;
  if (mode == MODE_SWIGLU && N % 32 != 0) return -1;
  if ((int64_t)N * K >= 0x80000000LL || K >= (1 << 24)) return -3;
  const int NT = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  const int T = N / 16, ftmin = mode == MODE_SWIGLU ? 2 : 1, ftmax = 8 / NT < 4 ? 8 / NT : 4;
  int FT = ftmin;
  for (int ft = ftmax; ft > ftmin; ft >>= 1)
    if ((T + ft - 1) / ft >= 512) {
      FT = ft;
      break;
    }
  const int groups = (T + FT - 1) / FT, nch = (K + CHUNK - 1) / CHUNK;
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

// x [M, K] bf16, wq [N, K] e4m3, scale [N] fp32, all row-contiguous and 16-byte aligned. mode 0: y [M, N]; mode 1
// (SwiGLU, wq = [gate; up] rows): y [M, N / 2]. (S, FT, NT) as pdt_gemm_skinny_w8_geo returns them (any S in
// [1, nch] and any served FT are accepted); S > 1 needs ws, S M N floats, and launches the combine.
int pdt_gemm_skinny_w8(const uint16_t* x, const uint8_t* wq, const float* scale, uint16_t* y, float* ws, int M, int N,
                       int K, int mode, int S, int FT, int NT, hipStream_t s) {
  int geo[3];
  const int rc = pdt_gemm_skinny_w8_geo(M, N, K, mode, 0, geo);
  if (rc != 0) return rc;
  const int nch = (K + CHUNK - 1) / CHUNK;
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
      hipLaunchKernelGGL(gemm_skinny_w8_combine_kernel<MODE_SWIGLU>, cgrid, dim3(256), 0, s, ws, scale, y, M, N, S);
    else
      hipLaunchKernelGGL(gemm_skinny_w8_combine_kernel<MODE_NONE>, cgrid, dim3(256), 0, s, ws, scale, y, M, N, S);
  }
  return 0;
}

}  // extern "C"
