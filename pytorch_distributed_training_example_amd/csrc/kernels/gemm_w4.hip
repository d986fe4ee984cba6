// W4A16 GEMM for any row count on group-wise int4 weights (gfx950): the tiled, compute-bound sibling of
// gemm_skinny_w4.hip on exactly its operands.
//   Y[m, n] = bf16(sum_g scale[g, n] * (sum_{k in group g} X[m, k] q[n, k]))                              [M, N]
// X [M, K] bf16, any M >= 1 (built for M > 64); q [N, K] integers in [-7, 7] as nibbles in Wq [N, K / 2] bytes
// (ops/linear.py pack_int4 defines the layout; gemm_skinny_w4.hip's header restates it); scale [K / 128, N] fp32,
// group-major. N % 16 == 0, K % 256 == 0, K < 2^24, Wq below 2^31 bytes, everything row-contiguous and 16-byte
// aligned. The inner sum is the MFMA unit's fp32 on exact bf16 operands, four chained v_mfma_f32_16x16x32_bf16
// from a zero C per 128-wide group (no scale is folded into an operand); the outer sum is one fp32 fma per group
// in group order; one rounding per output (after the split combine when S > 1). No atomics and no merge inside
// the workgroup: the order of summation is a function of (M, N, K, S) only.
// Roundings the kernel's own summation adds per output, beside the MFMA chains: K / 128 (one per group fma) + S
// (the S - 1 adds of the combine, rounded up). tests/test_gemm_w4_gpu.py uses this expression as its ksplit.
//
// Design. Tokens are MFMA columns and features MFMA rows, as in the skinny family, so a lane's four accumulator
// rows are features 4 g .. 4 g + 3 of token c ((c, g) = (lane & 15, lane >> 4)) and its four scales of a group
// are one 16-byte load. A workgroup is 4 waves on a BM x 128 tile of Y; wave w owns the FW = 2 feature tiles
// n0 + 32 w + 16 f of it and all BM tokens.
//   W   never touches LDS. Per group and feature tile a lane loads the 16 bytes (4 words) of its row's line
//       that are its A operands of the group's four MFMAs (buffer loads over a resource that ends at row N: a
//       feature tile past N reads zeros and is never stored), converts them to bf16 in registers (v_bfe_i32,
//       v_cvt_f32_i32, v_cvt_pk_bf16_f32: exact) and keeps the FW x 4 fragments stationary while it sweeps the
//       BM / 16 token tiles. Each nibble is converted once per workgroup and used by BM / 16 MFMAs; no two waves
//       hold the same feature tile. The next group's words and scales are requested before the sweep.
//   X   goes through LDS, shared by the four waves: a [BM, 128] bf16 image per stage (one group, 256 bytes per
//       row), two stages. Thread t stages chunk t & 15 of rows (t >> 4) + 16 j with buffer loads over a resource
//       that starts at the tile's first row and ends at row M (a row at or past M reads zeros, never memory),
//       requested before the sweep of the current stage and written to the other stage after it; one barrier per
//       group. 16-byte chunks are XOR-swizzled by row & 15 (gemm.hip's swz on 256-byte rows, which cover all 64
//       banks once): the B-operand ds_read_b128 of lane (c, g) for MFMA i, chunk (4 i + g) ^ c of row 16 t + c,
//       is conflict-free, and so are the staging writes (16 threads: 16 chunks of one row).
//   acc per (feature tile, token tile) and group: four chained MFMAs from a zero C into a short-lived f4, then
//       four fmas by the lane's scales. The sweep is unrolled, so FW chains per token tile and the next tile's
//       are independent and in flight together. Only FW x BM / 16 x 4 running sums persist.
// Budget (BM = 128 / 64): running sums 64 / 32 registers, stationary fragments 32, X in flight to LDS 32 / 16,
// next words and scales 16, B fragments and partials ~48: 2 workgroups per CU by registers (__launch_bounds__
// (256, 2)); LDS 64 / 32 KB per workgroup, so 2 per CU at BM = 128 (128 of 160 KB). The compiler's figures are in
// profiles/r28/gemm_w4_tall.txt.
// The two constraints, per wave and group at BM = 128, FW = 2 (a CU's LDS delivers 128 bytes per clock, an MFMA
// 16x16x32 takes 16 clocks of its SIMD: gemm.hip's header):
//   1. LDS read bandwidth. A B fragment is 1 KB per wave and serves FW MFMAs: 8 token tiles x 4 fragments =
//      32 KB per wave, 128 KB per workgroup = 1024 clocks of the CU's LDS, against 8 x 2 x 4 = 64 MFMAs = 1024
//      clocks of each SIMD. LDS reads alone are at parity with the matrix pipe (plus 32 KB of staging writes):
//      this geometry cannot pass about half of the MFMA peak. FW = 4 would halve the reads but holds 128 running
//      sums and 64 fragment registers, which leaves no room for 2 workgroups per CU; with 1 there is nothing to
//      run behind the barrier. FW = 2 is the choice; the ceiling is stated, not hidden.
//   2. Conversion VALU. 2.5 operations per nibble, 32 nibbles per lane, tile and group: 160 operations, plus
//      the 64 scale fmas: ~224 VALU issues = ~900 clocks per wave and group, under the 1024 MFMA clocks they
//      overlap with. At BM = 64 the MFMAs halve and the conversions do not: that instantiation is VALU-bound and
//      exists for shapes with too few tiles to fill the chip, where nothing is compute-bound anyway.
//
// pdt_gemm_w4_geo(M, N, K, splits) -> (S, BM, BN), a pure function of its arguments:
//   BN  128.
//   BM  128 when M > 64 and there are at least 128 tiles of 128 x 128, else 64 (twice the workgroups).
//   S   grid split over the 256-wide K steps. 1 when there are at least 256 workgroups, when splits == 1, or when
//       M N > 2^19 (the fp32 partials' round trip would cost more than the idle CUs); otherwise ceil(256 /
//       workgroups), at most K / 512 and at most 8. splits > 0 asks for that many (at most K / 256 come out).
//       Split s takes K steps [s nch / S, (s + 1) nch / S) and stores its scaled fp32 tile to ws [S, M, N];
//       gemm_w4_combine_kernel adds the partials in split order and rounds once.
#include "../common.h"
#include "../launchers.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int CHUNK = 256;             // k per K step: one 128-byte line of a weight row, two groups
constexpr int GROUP = 128;             // k per scale and per LDS stage
constexpr int FW = 2;                  // feature tiles per wave
constexpr int BN = 4 * FW * 16;        // features per workgroup
constexpr int ROW = GROUP * 2;         // bytes of an LDS row
constexpr uint32_t OOB = 0x80000000u;  // a buffer offset past any operand: the load returns zero

__device__ __forceinline__ u4 load16(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
}

__device__ __forceinline__ int swz(int row, int chunk) { return row * ROW + ((chunk ^ (row & 15)) << 4); }

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

template <int BM>
__global__ __launch_bounds__(256, 2) void gemm_w4_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ w,
                                                         const float* __restrict__ scale, uint16_t* __restrict__ y,
                                                         float* __restrict__ ws, int M, int N, int K) {
  constexpr int TT = BM / 16;      // token tiles
  constexpr int XL = BM / 16;      // 16-byte chunks of X a thread stages per group: BM rows x 16 chunks / 256 threads
  constexpr int STAGE = BM * ROW;  // bytes
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, sp = blockIdx.z, S = gridDim.z;
  const int nch = K / CHUNK;
  const int g0 = 2 * (int)((int64_t)sp * nch / S), g1 = 2 * (int)((int64_t)(sp + 1) * nch / S);  // this split's groups
  const int rows = min(BM, M - m0);
  const uint32_t xrow_bytes = 2u * (uint32_t)K, srow_bytes = 4u * (uint32_t)N;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(x + (int64_t)m0 * K), (short)0, (int)((uint32_t)rows * xrow_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(w), (short)0, N * (K >> 1), 0x00020000);
  const __amdgpu_buffer_rsrc_t srs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(scale), (short)0, (K / GROUP) * N * 4, 0x00020000);

  // byte offsets of the lane's slices within group 0: its 16 bytes of W row c of either feature tile, its four
  // scales (features 4 g ..), the X chunks it stages (a row at or past `rows` lies past the resource) and where
  // they go in a stage
  uint32_t wrow[FW], srow[FW], xoff[XL];
  int xdst[XL];
#pragma unroll
  for (int f = 0; f < FW; ++f) {
    const int n = n0 + (wv * FW + f) * 16;
    wrow[f] = n < N ? (uint32_t)(n + c) * ((uint32_t)K >> 1) + 32u * g : OOB;
    srow[f] = n < N ? 4u * (uint32_t)(n + 4 * g) : OOB;
  }
#pragma unroll
  for (int j = 0; j < XL; ++j) {
    const int row = (tid >> 4) + 16 * j, ch = tid & 15;
    xoff[j] = (uint32_t)row * xrow_bytes + 16u * ch;
    xdst[j] = swz(row, ch);
  }
  int xsrc[4];  // the lane's B fragment of MFMA i within token tile 0 of a stage
#pragma unroll
  for (int i = 0; i < 4; ++i) xsrc[i] = swz(c, 4 * i + g);

  f4 acc[FW][TT];
#pragma unroll
  for (int f = 0; f < FW; ++f)
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[f][t] = f4{0.f, 0.f, 0.f, 0.f};

  u4 xr[XL], wr[FW];
  f4 sr[FW], sc[FW];
  bf16x8 a[FW][4];
  auto request = [&](int G) {  // group G: line G >> 1, its half G & 1
#pragma unroll
    for (int j = 0; j < XL; ++j) xr[j] = load16(xrs, xoff[j] + (uint32_t)ROW * G);
#pragma unroll
    for (int f = 0; f < FW; ++f) {
      wr[f] = load16(wrs, wrow[f] + 128u * (G >> 1) + 16u * (G & 1));
      sr[f] = __builtin_bit_cast(f4, load16(srs, srow[f] + (uint32_t)G * srow_bytes));
    }
  };
  auto land = [&](char* st) {  // X to the stage, W to fragments
#pragma unroll
    for (int j = 0; j < XL; ++j) *reinterpret_cast<u4*>(st + xdst[j]) = xr[j];
#pragma unroll
    for (int f = 0; f < FW; ++f) {
      sc[f] = sr[f];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[f][i] = cvt8(wr[f][i]);
    }
  };

  request(g0);
  land(lds);
  __syncthreads();
  for (int G = g0; G < g1; ++G) {
    const char* st = lds + ((G - g0) & 1) * STAGE;
    const bool more = G + 1 < g1;
    if (more) request(G + 1);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      bf16x8 b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const bf16x8*>(st + t * 16 * ROW + xsrc[i]);
#pragma unroll
      for (int f = 0; f < FW; ++f) {
        f4 part = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[f][i], b[i], part, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[f][t][r] = __builtin_fmaf(part[r], sc[f][r], acc[f][t][r]);
      }
    }
    // the other stage was last read in the sweep before this one, which every wave left at the last barrier
    if (more) land(lds + (((G - g0) & 1) ^ 1) * STAGE);
    __syncthreads();
  }

#pragma unroll
  for (int f = 0; f < FW; ++f) {
    const int n = n0 + (wv * FW + f) * 16;
    if (n >= N) continue;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int tok = m0 + 16 * t + c;
      if (tok >= M) continue;
      if (S > 1) {
        *reinterpret_cast<f4*>(ws + ((int64_t)sp * M + tok) * N + n + 4 * g) = acc[f][t];
      } else {
        const float o[4] = {acc[f][t][0], acc[f][t][1], acc[f][t][2], acc[f][t][3]};
        Vec4<uint16_t>::st(y, (int64_t)tok * N + n + 4 * g, o);
      }
    }
  }
}

// One thread per 4 consecutive outputs: the S scaled partials in split order, one rounding.
__global__ __launch_bounds__(256) void gemm_w4_combine_kernel(const float* __restrict__ ws, uint16_t* __restrict__ y,
                                                              int64_t quads, int64_t MN, int S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  const float* p = ws + 4 * i;
  f4 a = *reinterpret_cast<const f4*>(p);
  for (int s = 1; s < S; ++s) a += *reinterpret_cast<const f4*>(p + s * MN);
  const float o[4] = {a[0], a[1], a[2], a[3]};
  Vec4<uint16_t>::st(y, 4 * i, o);
}

}  // namespace

extern "C" {

// (S, BM, BN) into geo3: the rule in this file's header. -1: outside the contract; -3: Wq past 2^31 bytes, K past
// 2^24 or more token bands than a grid holds.
int pdt_gemm_w4_geo(int M, int N, int K, int splits, int* geo3) {
  if (M < 1 || N < 16 || N % 16 != 0 || K < CHUNK || K % CHUNK != 0 || splits < 0) return -1;
  if ((int64_t)N * (K / 2) >= 0x80000000LL || K >= (1 << 24) || (M + 63) / 64 > 65535) return -3;
  const int64_t nb = (N + BN - 1) / BN, tiles128 = (int64_t)((M + 127) / 128) * nb;
  const int BM = (M > 64 && tiles128 >= 128) ? 128 : 64;
  const int64_t wgs = (int64_t)((M + BM - 1) / BM) * nb;
  const int nch = K / CHUNK;
  int S = splits;
  if (S == 0) {
    S = 1;
    if (wgs < 256 && (int64_t)M * N <= (1 << 19)) {
      S = (int)((256 + wgs - 1) / wgs);
      if (S > nch / 2) S = nch / 2;
      if (S > 8) S = 8;
      if (S < 1) S = 1;
    }
  }
  if (S > nch) S = nch;
  geo3[0] = S;
  geo3[1] = BM;
  geo3[2] = BN;
  return 0;
}

// x [M, K] bf16, wq [N, K / 2] packed nibbles, scale [K / 128, N] fp32, y [M, N] bf16, all row-contiguous and
// 16-byte aligned. (S, BM) as pdt_gemm_w4_geo returns them (any S in [1, K / 256] and either BM are accepted);
// S > 1 needs ws, S M N floats, and launches the combine.
int pdt_gemm_w4(const uint16_t* x, const uint8_t* wq, const float* scale, uint16_t* y, float* ws, int M, int N, int K,
                int S, int BM, hipStream_t s) {
  int geo[3];
  const int rc = pdt_gemm_w4_geo(M, N, K, 0, geo);
  if (rc != 0) return rc;
  if (S < 1 || S > K / CHUNK || S > 65535 || (BM != 64 && BM != 128)) return -2;
  if (S > 1 && !ws) return -4;
  const int64_t MN = (int64_t)M * N, quads = MN / 4;
  if ((quads + 255) / 256 > 0x7fffffffLL) return -3;
  const dim3 grid((N + BN - 1) / BN, (M + BM - 1) / BM, S);
  if (BM == 128)
    hipLaunchKernelGGL(gemm_w4_kernel<128>, grid, dim3(256), 0, s, x, wq, scale, y, ws, M, N, K);
  else
    hipLaunchKernelGGL(gemm_w4_kernel<64>, grid, dim3(256), 0, s, x, wq, scale, y, ws, M, N, K);
  if (S > 1)
    hipLaunchKernelGGL(gemm_w4_combine_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, ws, y, quads, MN,
                       S);
  return 0;
}

}  // extern "C"
