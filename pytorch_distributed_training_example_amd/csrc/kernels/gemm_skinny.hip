// Weight-streaming skinny GEMM for gfx950: Y[M, N] = X[M, K] W[N, K]^T with 1 <= M <= 64 (the Linears of a
// decode step or a short extend), bf16 operands, fp32 accumulation, one rounding to bf16 per output.
// N % 16 == 0, K % 64 == 0, X and W row-contiguous, N K 2 < 2^31 bytes (32-bit buffer offsets). No atomics: the
// order of summation is a function of (M, N, K, S) only, so the same inputs give the same bits every run.
//
// There is nothing to reuse at these shapes: every weight is read once and meets at most 64 tokens. The kernel
// therefore keeps wide weight loads in flight and feeds the matrix cores from registers, with no LDS in the
// K loop.
//
// Operands are swapped, as in the flash and decode kernels: the 16 weight rows of a feature tile are the rows
// of v_mfma_f32_16x16x32_bf16 (A), up to 16 tokens its columns (B), so lane (c, g) = (lane & 15, lane >> 4)
// ends with features 4g .. 4g + 3 of token c: one 8-byte store. NT in {1, 2, 4} column tiles cover M <= 16 /
// 32 / 64; a W fragment is fetched once and serves all NT.
//   W   global -> MFMA A registers. Per 64-wide K step lane (c, g) loads the 32 contiguous bytes
//       [32 g, 32 g + 32) of row c's 128-byte line (two 16-byte loads, two MFMAs), so lanes c, c + 16, c + 32,
//       c + 48 cover the line. Slot j of the first MFMA's operand is then k = 16 g + j, of the second
//       16 g + 8 + j: not the instruction's natural k order, but X is loaded with the same placement and a dot
//       product does not care where its terms sit (gemm.hip's F8 comment makes the same argument).
//       Non-temporal (the weights are read once per launch): in the captured llama_medium decode step that
//       measured 5 % faster than plain loads (1.03 against 1.09 ms), although a shape replayed on its own is
//       level or up to 15 % slower with it (lm_head; profiles/r21/skinny_gemm.txt). pdt_gemm_skinny_tune keeps
//       the A/B.
//   X   small and L2-resident: buffer loads over a resource of M rows, so token columns at or past M read as
//       zero in hardware, whatever follows X in memory; they are never stored. Per 256-wide K chunk a wave holds
//       8 NT X fragments (32 NT VGPRs) and reuses them for its FT feature tiles.
// A workgroup is 4 waves that own FT feature tiles (16 rows of W each) and one range of 256-wide K chunks
// (all of K when S == 1). The waves take the range's chunks round-robin (wave w: chunks w, w + 4, ...; the
// count need not divide by 4, and the last chunk may hold 1-3 steps: a step at or past K is loaded from an
// out-of-range offset, zero, for both operands). The loop over (chunk, feature tile) is pipelined in
// registers: the next item's 8 W loads (8 KB per wave) are issued before the current item's 8 NT MFMAs, and
// there is no barrier in it. The four waves' fp32 tiles are then merged through LDS in wave order 0..3 behind
// one barrier, wave w finishing output tiles w, w + 4, ...
//
// MODE_SWIGLU: W is c_fc's packed [2F, K] (gate rows [0, F), up rows [F, 2F), F % 16 == 0). Feature tiles come
// in pairs (gate rows n .. n + 15, up rows F + n .. F + n + 15, FT even); the merge rounds both to bf16 and
// applies swiglu_fwd2 (swiglu_math.h) to the rounded values, storing [M, F]: what swiglu.hip computes from
// this kernel's own unfused output. The kernels here are compiled without the packed fp32 instructions (a
// per-function target feature, as attn_extend_kernel), swiglu.hip with them; the forward formula is
// multiplies, one add of a transcendental's result, v_exp_f32 and v_rcp_f32, with nothing to contract, and a
// packed multiply is the scalar one per lane, so the bits agree (tests/test_gemm_skinny_gpu.py asserts it).
//
// Grid split-K (S > 1): workgroup (group, s) takes chunks [s nch / S, (s + 1) nch / S) and stores its merged
// fp32 tile to ws [S, M, N]; gemm_skinny_combine_kernel adds the S partials in split order, rounds once and,
// in MODE_SWIGLU, applies the pair formula. S == 1 launches no combine.
//
// Geometry, pdt_gemm_skinny_geo(M, N, K, mode, splits) -> (S, FT, NT), a pure function of its arguments:
//   NT  the smallest of 1, 2, 4 with 16 NT >= M.
//   FT  feature tiles per workgroup, from {1, 2, 4} ({2, 4} in MODE_SWIGLU) with FT NT <= 8 (the accumulators
//       and 32 NT X registers have to leave room for two W buffers): the largest that still gives 512
//       workgroups, two per CU at the occupancy of the widest instantiation (2 waves per SIMD), else the
//       smallest. A larger FT amortises a wave's X fragments, which it re-reads from L2 per chunk.
//   S   1 when there are at least 256 workgroups (one per CU) or splits == 1; otherwise ceil(256 / groups),
//       at most nch / 2 (a split keeps two chunks, so at least two waves of a workgroup stream) and at most 16.
//       splits > 0 asks for that many (at most nch come out).
#include "../common.h"
#include "../launchers.h"
#include "../swiglu_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int CHUNK = 256;             // K elements per chunk: 4 steps of 64, 8 MFMAs per feature and column tile
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
__device__ __forceinline__ bf16x8 load8(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, AUX));
}

// The 8 fragments of one 256-wide chunk of a row: step s at byte offset 128 s of the chunk, fragments 2s and
// 2s + 1 the lane's two 16-byte halves. A step at or past K is read from OOB.
template <int AUX>
__device__ __forceinline__ void load_chunk(bf16x8 (&f)[8], __amdgpu_buffer_rsrc_t rs, uint32_t row_off, int k0,
                                           int K) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = k0 + 64 * s;
    const uint32_t off = k < K ? row_off + 2u * (uint32_t)k : OOB;
    f[2 * s] = load8<AUX>(rs, off);
    f[2 * s + 1] = load8<AUX>(rs, off + 16);
  }
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

template <int NT, int FT, int MODE, int WAUX>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void gemm_skinny_kernel(const uint16_t* __restrict__ x,
                                                                            const uint16_t* __restrict__ w,
                                                                            uint16_t* __restrict__ y,
                                                                            float* __restrict__ ws, int M, int N,
                                                                            int K) {
  static_assert(FT * NT <= 8 && (MODE == MODE_NONE || FT % 2 == 0), "gemm_skinny: instantiation");
  __shared__ f4 red[4][FT * NT][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int blk = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
  const int nch = (K + CHUNK - 1) / CHUNK;
  const int cb = (int)((int64_t)sp * nch / S), ce = (int)((int64_t)(sp + 1) * nch / S);
  const __amdgpu_buffer_rsrc_t xrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), (short)0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(w), (short)0, N * K * 2, 0x00020000);

  // byte offsets of the lane's 32 bytes within step 0: W row c of each feature tile, X row 16 j + c
  uint32_t wrow[FT], xrow[NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    const int r0 = tile_row0<FT, MODE>(blk, ft, N);
    wrow[ft] = r0 >= 0 ? (uint32_t)(r0 + c) * (uint32_t)K * 2u + 32u * g : OOB;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) xrow[j] = (uint32_t)(16 * j + c) * (uint32_t)K * 2u + 32u * g;  // row >= M: past the end

  f4 acc[FT][NT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[ft][j] = f4{0.f, 0.f, 0.f, 0.f};

  // ---- the K loop: items (chunk, feature tile), the next item's W in flight under the current item's MFMAs
  bf16x8 wq[2][8];
  int ch = cb + wv;
  if (ch < ce) load_chunk<WAUX>(wq[0], wrs, wrow[0], ch * CHUNK, K);
  for (; ch < ce; ch += 4) {
    bf16x8 xf[NT][8];
#pragma unroll
    for (int j = 0; j < NT; ++j) load_chunk<0>(xf[j], xrs, xrow[j], ch * CHUNK, K);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) {
      // FT even: the buffers alternate with ft; FT == 1: the next chunk's lands in wq[1] and is moved down
      bf16x8(&cur)[8] = wq[FT == 1 ? 0 : (ft & 1)];
      bf16x8(&nxt)[8] = wq[FT == 1 ? 1 : ((ft + 1) & 1)];
      if (ft + 1 < FT) {
        load_chunk<WAUX>(nxt, wrs, wrow[ft + 1 < FT ? ft + 1 : 0], ch * CHUNK, K);
      } else if (ch + 4 < ce) {
        load_chunk<WAUX>(nxt, wrs, wrow[0], (ch + 4) * CHUNK, K);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[ft][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[i], xf[j][i], acc[ft][j], 0, 0, 0);
      if (FT == 1 && ch + 4 < ce) {
#pragma unroll
        for (int i = 0; i < 8; ++i) cur[i] = nxt[i];
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

// One thread per 4 consecutive outputs: the S partials in split order, one rounding.
template <int MODE>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256) void gemm_skinny_combine_kernel(const float* __restrict__ ws,
                                                                                    uint16_t* __restrict__ y, int M,
                                                                                    int N, int S) {
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

int g_w_nt = 1;  // pdt_gemm_skinny_tune

template <int NT, int FT, int MODE>
void launch(dim3 grid, hipStream_t s, const uint16_t* x, const uint16_t* w, uint16_t* y, float* ws, int M, int N,
            int K) {
  if (g_w_nt)
    hipLaunchKernelGGL((gemm_skinny_kernel<NT, FT, MODE, W_NT>), grid, dim3(256), 0, s, x, w, y, ws, M, N, K);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<NT, FT, MODE, 0>), grid, dim3(256), 0, s, x, w, y, ws, M, N, K);
}

// The instantiations: FT in {1, 2, 4} ({2, 4} in MODE_SWIGLU) with FT NT <= 8; the caller has checked FT.
template <int NT, int MODE>
void launch_ft(int FT, dim3 grid, hipStream_t s, const uint16_t* x, const uint16_t* w, uint16_t* y, float* ws, int M,
               int N, int K) {
  if constexpr (MODE == MODE_NONE)
    if (FT == 1) return launch<NT, 1, MODE>(grid, s, x, w, y, ws, M, N, K);
  if constexpr (NT <= 2)
    if (FT == 4) return launch<NT, 4, MODE>(grid, s, x, w, y, ws, M, N, K);
  launch<NT, 2, MODE>(grid, s, x, w, y, ws, M, N, K);
}

}  // namespace

extern "C" {

// A/B only: W loads non-temporal (1, the default) or plain (0); negative: query. Returns the previous setting.
int pdt_gemm_skinny_tune(int w_nontemporal) {
  const int prev = g_w_nt;
  if (w_nontemporal >= 0) g_w_nt = w_nontemporal ? 1 : 0;
  return prev;
}

// (S, FT, NT) into geo3: the rule in this file's header. -1: outside the contract; -3: W past 2^31 bytes.
int pdt_gemm_skinny_geo(int M, int N, int K, int mode, int splits, int* geo3) {
  if (M < 1 || M > 64 || N < 16 || N % 16 != 0 || K < 64 || K % 64 != 0 || splits < 0) return -1;
  if (mode != MODE_NONE && mode != MODE_SWIGLU) return -1;
  if (mode == MODE_SWIGLU && N % 32 != 0) return -1;
  if ((int64_t)N * K * 2 >= 0x80000000LL) return -3;
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

// x [M, K], w [N, K] bf16 row-contiguous, 16-byte aligned. mode 0: y [M, N]; mode 1 (SwiGLU, w = [gate; up]
// rows): y [M, N / 2]. (S, FT, NT) as pdt_gemm_skinny_geo returns them (any S in [1, nch] and any served FT are
// accepted); S > 1 needs ws, S M N floats, and launches the combine.
int pdt_gemm_skinny(const uint16_t* x, const uint16_t* w, uint16_t* y, float* ws, int M, int N, int K, int mode, int S,
                    int FT, int NT, hipStream_t s) {
  int geo[3];
  const int rc = pdt_gemm_skinny_geo(M, N, K, mode, 0, geo);
  if (rc != 0) return rc;
  const int nch = (K + CHUNK - 1) / CHUNK;
  if (NT != geo[2] || S < 1 || S > nch || S > 65535) return -2;
  if ((FT != 1 && FT != 2 && FT != 4) || FT * NT > 8 || (mode == MODE_SWIGLU && FT == 1)) return -2;
  if (S > 1 && !ws) return -4;
  const dim3 grid((N / 16 + FT - 1) / FT, S);
  if (mode == MODE_NONE) {
    if (NT == 1) launch_ft<1, MODE_NONE>(FT, grid, s, x, w, y, ws, M, N, K);
    else if (NT == 2) launch_ft<2, MODE_NONE>(FT, grid, s, x, w, y, ws, M, N, K);
    else launch_ft<4, MODE_NONE>(FT, grid, s, x, w, y, ws, M, N, K);
  } else {
    if (NT == 1) launch_ft<1, MODE_SWIGLU>(FT, grid, s, x, w, y, ws, M, N, K);
    else if (NT == 2) launch_ft<2, MODE_SWIGLU>(FT, grid, s, x, w, y, ws, M, N, K);
    else launch_ft<4, MODE_SWIGLU>(FT, grid, s, x, w, y, ws, M, N, K);
  }
  if (S > 1) {
    const int items = M * ((mode == MODE_SWIGLU ? N / 2 : N) / 4);
    const dim3 cgrid((items + 255) / 256);
    if (mode == MODE_SWIGLU)
      hipLaunchKernelGGL(gemm_skinny_combine_kernel<MODE_SWIGLU>, cgrid, dim3(256), 0, s, ws, y, M, N, S);
    else
      hipLaunchKernelGGL(gemm_skinny_combine_kernel<MODE_NONE>, cgrid, dim3(256), 0, s, ws, y, M, N, S);
  }
  return 0;
}

}  // extern "C"
