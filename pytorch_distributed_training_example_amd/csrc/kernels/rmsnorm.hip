// RMSNorm forward/backward for gfx950 (Llama-style decoders: D = 768, 1024, 2048).
//
// The design of layernorm.hip without the mean and the bias. One wave64 per row: the row stays in
// registers (D/64 values per lane, 8-byte bf16 vectors), so the forward is one HBM read and one write:
//   rstd = 1 / sqrt(mean_j(x_j^2) + eps),   y = round_T(x * rstd * w),   rstd kept (fp32) for the backward.
// The backward computes, with xh = x * rstd,
//   dx = rstd * (g w - xh * mean_j(g w xh))   (+ ds)
// per row in registers and per-workgroup partial dw slabs, summed by a fixed-order second pass
// (deterministic, no atomics).
//
// Residual fusion (pre-norm blocks), as ln_fwd_kernel does it: the forward optionally adds a residual
// branch first, s = round_T(x + h) (exactly what a separate add would store), writes s (the new residual
// stream) and normalises it; the backward optionally adds the residual stream's own gradient ds.
#include "../common.h"
#include "../colsum_finalize.h"
#include "../dispatch.h"
#include "../launchers.h"
#include "../fp8_pack.h"

using namespace pdt;

namespace {

constexpr int kRowsPerBlock = 4;  // 4 waves, one row each

// The row arithmetic shared by rms_fwd_kernel and rms_fwd_fp8_kernel, so both produce the same bits (the
// fp8 form quantizes exactly the bf16 y). The contraction is pinned to what rms_fwd_kernel has always
// compiled to: each square rounded on its own and added in (k, j) order (never fused: the squares issue as
// packed multiplies), one fused multiply-add for mean + eps.
template <int K>
__device__ __forceinline__ float rms_rstd(const float (&v)[K][4], float eps) {
#pragma clang fp contract(off)
  constexpr int D = 256 * K;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) q += v[k][j] * v[k][j];
  return rsqrtf(__builtin_fmaf(wave_sum(q), 1.f / D, eps));
}
__device__ __forceinline__ float rms_val(float v, float rstd, float w) {
#pragma clang fp contract(off)
  return v * rstd * w;
}

// K = D / 256: 4-element groups per lane (D = 256*K)
template <typename T, int K>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                      const float* __restrict__ w, T* __restrict__ y,
                                                      T* __restrict__ sum_out, float* __restrict__ rstd_out,
                                                      int64_t N, float eps) {
  constexpr int D = 256 * K;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= N) return;
  const T* xr = x + row * D;
  float v[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Vec4<T>::ld(xr, (int64_t)(k * 256 + lane * 4), v[k]);
    if (res != nullptr) {  // s = x + h, stored and normalised at storage precision
      float hv[4];
      Vec4<T>::ld(res + row * D, (int64_t)(k * 256 + lane * 4), hv);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = round_to<T>(v[k][j] + hv[j]);
      Vec4<T>::st(sum_out + row * D, (int64_t)(k * 256 + lane * 4), v[k]);
    }
  }
  const float rstd = rms_rstd<K>(v, eps);
  T* yr = y + row * D;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = k * 256 + lane * 4;
    float wv[4], o[4];
    Vec4<float>::ld(w, c, wv);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = rms_val(v[k][j], rstd, wv[j]);
    Vec4<T>::st(yr, (int64_t)c, o);
  }
  if (lane == 0) rstd_out[row] = rstd;
}

// RMSNorm (+ residual add) whose output goes straight to e4m3 for the fp8 GEMM that consumes it (ops/fp8.py
// Fp8Act: a Llama block's c_attn and c_fc inputs), the twin of layernorm.hip's ln_fwd_fp8_kernel. Unfused, the
// bf16 y was written here and read back by a cast-transpose pass; this kernel writes y as fp8 row-major AND
// transposed, scaled by the consumer's delayed scale, with |y|max folded into its amax slot. y is rounded to
// bf16 before quantizing and s, rstd come from rms_rstd / rms_val, so the bytes equal the unfused chain's.
// A workgroup owns 32 rows (8 waves x 4 rows, every row's loads issued before any row's math); the fp8 rows
// also go to an LDS image (row pitch D + 4 bytes: the transposed readers' 8-row blocks hit distinct banks)
// from which the transposed 32-B row segments are written. Tiles are placed XCD-aware so the four tiles
// sharing a 128-B line of y^T write it through one L2. N % 16 == 0 keeps the 8-row blocks whole.
template <int K>
__global__ __launch_bounds__(512) void rms_fwd_fp8_kernel(const uint16_t* __restrict__ x,
                                                          const uint16_t* __restrict__ res,
                                                          const float* __restrict__ w,
                                                          uint16_t* __restrict__ sum_out, uint8_t* __restrict__ yq,
                                                          uint8_t* __restrict__ yqt, float* __restrict__ rstd_out,
                                                          int64_t N, float eps, const float* __restrict__ scale,
                                                          float* __restrict__ amax, int striped) {
  constexpr int D = 256 * K, kRows = 32, kPitch = D + 4;
  __shared__ __attribute__((aligned(16))) uint8_t tile[kRows * kPitch];
  __shared__ float red[8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * kRows;
  const float s8 = *scale;
  float wr[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) Vec4<float>::ld(w, k * 256 + lane * 4, wr[k]);
  float am = 0.f;
  uint2 xv[4][K], hv[4][K];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t row = m0 + wv * 4 + q;
    if (row < N) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        xv[q][k] = *reinterpret_cast<const uint2*>(x + row * D + k * 256 + lane * 4);
        if (res != nullptr) hv[q][k] = *reinterpret_cast<const uint2*>(res + row * D + k * 256 + lane * 4);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tr = wv * 4 + q;
    const int64_t row = m0 + tr;
    if (row >= N) continue;  // wave-uniform
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      v[k][0] = __uint_as_float(xv[q][k].x << 16); v[k][1] = __uint_as_float(xv[q][k].x & 0xffff0000u);
      v[k][2] = __uint_as_float(xv[q][k].y << 16); v[k][3] = __uint_as_float(xv[q][k].y & 0xffff0000u);
      if (res != nullptr) {  // s = x + h, stored and normalised at storage precision (as rms_fwd_kernel)
        const float hh[4] = {__uint_as_float(hv[q][k].x << 16), __uint_as_float(hv[q][k].x & 0xffff0000u),
                             __uint_as_float(hv[q][k].y << 16), __uint_as_float(hv[q][k].y & 0xffff0000u)};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = round_to<uint16_t>(v[k][j] + hh[j]);
        Vec4<uint16_t>::st(sum_out + row * D, (int64_t)(k * 256 + lane * 4), v[k]);
      }
    }
    const float rstd = rms_rstd<K>(v, eps);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = round_to<uint16_t>(rms_val(v[k][j], rstd, wr[k][j]));
        am = fmaxf(am, fabsf(o[j]));
      }
      const uint32_t pk = pack4_fp8(o[0] * s8, o[1] * s8, o[2] * s8, o[3] * s8);
      *reinterpret_cast<uint32_t*>(yq + row * D + k * 256 + lane * 4) = pk;
      *reinterpret_cast<uint32_t*>(tile + tr * kPitch + k * 256 + lane * 4) = pk;
    }
    if (lane == 0) rstd_out[row] = rstd;
  }
  __syncthreads();
  // y^T: item (word column g, 8-row block rb) -> 4 rows of y^T, 8 bytes each
  for (int it = threadIdx.x; it < (D / 4) * 4; it += 512) {
    const int rb = it & 3, g = it >> 2;
    if (m0 + rb * 8 < N) {
      uint32_t t8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t8[i] = *reinterpret_cast<const uint32_t*>(tile + (rb * 8 + i) * kPitch + g * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<uint2*>(yqt + (int64_t)(g * 4 + j) * N + m0 + rb * 8) =
            make_uint2(byte_col(t8[0], t8[1], t8[2], t8[3], j), byte_col(t8[4], t8[5], t8[6], t8[7], j));
    }
  }
  am = wave_max(am);
  if (lane == 0) red[wv] = am;
  __syncthreads();
  if (threadIdx.x == 0) {
    float bm = red[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) bm = fmaxf(bm, red[i]);
    if (bm > 0.f) atomicMax(reinterpret_cast<int*>(amax_slot(amax, striped, blockIdx.x)), __float_as_int(bm));
  }
}

// Backward: dx per row; per-workgroup partial dw written to part[blk][D]. A workgroup owns the rows
// [blk * rows_per_block, (blk + 1) * rows_per_block), its 4 waves take them interleaved.
template <typename T, int K>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                      const T* __restrict__ dres, const float* __restrict__ w,
                                                      const float* __restrict__ rstd, T* __restrict__ dx,
                                                      float* __restrict__ part, int64_t N, int rows_per_block) {
  constexpr int D = 256 * K;
  __shared__ float sdw[4][D];
  const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
  float dw[K][4], wr[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Vec4<float>::ld(w, k * 256 + lane * 4, wr[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) dw[k][j] = 0.f;
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(N, r0 + rows_per_block);
  // RF rows per wave in flight (rows r, r + 4, ...): all their loads are issued before any row's math,
  // so a wave exposes the memory latency once per RF rows (as ln_bwd_kernel)
  constexpr int RF = K <= 4 ? 4 : 2;
  for (int64_t row0 = r0 + wv_id; row0 < r1; row0 += 4 * RF) {
    float g[RF][K][4], xh[RF][K][4], rr[RF][K][4];
    float rs[RF];
    bool ok[RF];
#pragma unroll
    for (int q = 0; q < RF; ++q) {
      const int64_t row = row0 + 4 * q;
      ok[q] = row < r1;
      const int64_t rw = ok[q] ? row : row0;  // duplicate load for a missing row, result unused
      rs[q] = rstd[rw];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t c = rw * D + k * 256 + lane * 4;
        Vec4<T>::ld(dy, c, g[q][k]);
        Vec4<T>::ld(x, c, xh[q][k]);
        if (dres != nullptr) Vec4<T>::ld(dres, c, rr[q][k]);
      }
    }
#pragma unroll
    for (int q = 0; q < RF; ++q) {
      if (!ok[q]) continue;
      const int64_t row = row0 + 4 * q;
      float s2 = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[q][k][j] *= rs[q];
          dw[k][j] += g[q][k][j] * xh[q][k][j];
          g[q][k][j] *= wr[k][j];  // g w from here on
          s2 += g[q][k][j] * xh[q][k][j];
        }
      s2 = wave_sum(s2) * (1.f / D);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = rs[q] * (g[q][k][j] - xh[q][k][j] * s2);
          if (dres != nullptr) o[j] += rr[q][k][j];  // + the residual stream's own gradient
        }
        Vec4<T>::st(dx, row * D + k * 256 + lane * 4, o);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) sdw[wv_id][k * 256 + lane * 4 + j] = dw[k][j];
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256)
    part[(int64_t)blockIdx.x * D + c] = sdw[0][c] + sdw[1][c] + sdw[2][c] + sdw[3][c];
}

// The backward's partition: at least kBwdMinRows rows per workgroup (8 per wave), at most kBwdMaxBlocks
// workgroups (2 per CU; the dw slab is nblk x D floats). Past kBwdMinRows * kBwdMaxBlocks rows a
// workgroup owns more than kBwdMinRows.
constexpr int64_t kBwdMinRows = 32, kBwdMaxBlocks = 512;

inline int rms_bwd_blocks(int64_t N, int& rows_per_block) {
  return row_blocks(N, kBwdMinRows, kBwdMaxBlocks, rows_per_block);
}

}  // namespace

extern "C" {

int64_t pdt_rms_workspace_floats(int64_t N, int D) {
  int rpb;
  return (int64_t)rms_bwd_blocks(N, rpb) * D;
}

// Forward and backward take the same widths, K = D / 256 in {1, .., 6, 8}: every forward has its backward.

// res / sum_out: optional residual branch h and the stored sum s = x + h (both or neither).
int pdt_rms_fwd(const void* x, const void* res, int dtype, const float* w, void* y, void* sum_out, float* rstd,
                int64_t N, int D, float eps, hipStream_t s) {
  if ((res == nullptr) != (sum_out == nullptr)) return -2;
  if (D <= 0 || D % 256 != 0) return -1;
  if (N == 0) return 0;
  const dim3 grid((unsigned)((N + kRowsPerBlock - 1) / kRowsPerBlock));
  const bool ok = with_k<1, 2, 3, 4, 5, 6, 8>(D / 256, [&](auto kc) {
    with_elem(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((rms_fwd_kernel<T, decltype(kc)::value>), grid, dim3(256), 0, s, (const T*)x, (const T*)res,
                         w, (T*)y, (T*)sum_out, rstd, N, eps);
    });
  });
  return ok ? 0 : -1;
}

// bf16 x (+ res -> sum_out) -> RMSNorm -> e4m3 yq [N, D] and yq^T [D, N] (scale / amax: the consumer's fp8
// state row). N % 16 == 0; D = 256 K with K in {1, .., 6}: the 32-row LDS image at pitch D + 4 passes 64 KB at
// K = 8, which keeps rms_fwd + the cast pass.
int pdt_rms_fwd_fp8(const uint16_t* x, const uint16_t* res, const float* w, uint16_t* sum_out, uint8_t* yq,
                    uint8_t* yqt, float* rstd, int64_t N, int D, float eps, const float* scale, float* amax,
                    int striped, hipStream_t s) {
  if ((res == nullptr) != (sum_out == nullptr)) return -2;
  if (D <= 0 || D % 256 != 0 || N < 0 || N % 16 != 0) return -1;
  const int64_t nblk = (N + 31) / 32;
  if (nblk > 0x7fffffffLL) return -1;
  bool launch = N > 0;
  const bool ok = with_k<1, 2, 3, 4, 5, 6>(D / 256, [&](auto kc) {
    if (!launch) return;
    hipLaunchKernelGGL((rms_fwd_fp8_kernel<decltype(kc)::value>), dim3((unsigned)nblk), dim3(512), 0, s, x, res, w,
                       sum_out, yq, yqt, rstd, N, eps, scale, amax, striped);
  });
  return ok ? 0 : -1;
}

// dres: optional gradient added into dx (residual stream), same dtype/layout as dx. ws: pdt_rms_workspace_floats.
// An empty input launches only the finalize, over no slabs: dw = 0.
int pdt_rms_bwd(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* rstd,
                void* dx, float* dw, int64_t N, int D, float* ws, hipStream_t s) {
  if (D <= 0 || D % 256 != 0) return -1;
  int rpb;
  const int nblk = rms_bwd_blocks(N, rpb);
  const bool ok = with_k<1, 2, 3, 4, 5, 6, 8>(D / 256, [&](auto kc) {
    if (nblk == 0) return;
    with_elem(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((rms_bwd_kernel<T, decltype(kc)::value>), dim3(nblk), dim3(256), 0, s, (const T*)dy,
                         (const T*)x, (const T*)dres, w, rstd, (T*)dx, ws, N, rpb);
    });
  });
  if (!ok) return -1;
  hipLaunchKernelGGL((colsum_finalize_kernel<1, float>), dim3((D + 15) / 16), dim3(256), 0, s, ws, nblk, D, dw,
                     (float*)nullptr);
  return 0;
}

}  // extern "C"
