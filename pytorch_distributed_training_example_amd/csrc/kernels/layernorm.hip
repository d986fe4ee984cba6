// LayerNorm forward/backward for gfx950 (ViT-B/16 D=768, GPT-2-medium D=1024).
//
// Not in the reference (no transformer); required by the ViT / GPT-2 north-star configs.
// One wave64 per row: the row stays in registers (D/64 values per lane, 8-byte bf16
// vectors), so the forward is an exact two-pass mean/variance with a single HBM read and
// write. The backward computes dx per row in registers and per-workgroup partial
// dgamma/dbeta (fixed-order second pass: deterministic, no atomics).
//
// Residual fusion (pre-norm transformer blocks): the forward optionally adds a residual branch
// first, s = x + h (rounded to the storage dtype, exactly as a separate add would store it),
// writes s (the new residual stream) and normalises it; the backward optionally adds the
// residual stream's own gradient, dx = LN'(dy) + ds. That removes the separate add kernels
// (2 per block forward, 2 per block backward) and one full read of s.
#include "../common.h"
#include "../colsum_finalize.h"
#include "../dispatch.h"
#include "../launchers.h"
#include "../fp8_pack.h"
#include "../philox.h"

using namespace pdt;

namespace {

constexpr int kRowsPerBlock = 4;  // 4 waves, one row each

// Row statistics and the normalised value, shared by ln_fwd_kernel and ln_fwd_fp8_kernel with FP
// contraction off, so both produce the same bits (the fp8 form quantizes exactly the bf16 y).
template <int K>
__device__ __forceinline__ void ln_stats(const float (&v)[K][4], float eps, float& mean, float& rstd) {
#pragma clang fp contract(off)
  constexpr int D = 256 * K;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) s += v[k][0] + v[k][1] + v[k][2] + v[k][3];
  mean = wave_sum(s) * (1.f / D);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = v[k][j] - mean;
      q += d * d;
    }
  rstd = rsqrtf(wave_sum(q) * (1.f / D) + eps);
}
__device__ __forceinline__ float ln_val(float v, float mean, float rstd, float w, float b) {
#pragma clang fp contract(off)
  return (v - mean) * rstd * w + b;
}

// K = D / 256: 4-element groups per lane (D = 256*K)
// DROP (residual dropout, with res): s = x + round_T(h * m * scale), the mask regenerated from the
// ticket (philox.h, flat layout: a lane's 4 elements are one word of one call). The dropped h is
// rounded to T before the add, as dropout_kernel would have stored it, so s and y equal
// add+LayerNorm of the separately dropped h bit for bit, with no extra byte moved.
template <typename T, int K, bool DROP = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                     const float* __restrict__ w, const float* __restrict__ b,
                                                     T* __restrict__ y, T* __restrict__ sum_out,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     int64_t N, float eps, const int64_t* __restrict__ ticket = nullptr,
                                                     int dstream = 0, int thr = 0) {
  constexpr int D = 256 * K;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= N) return;
  DropSite site;
  if constexpr (DROP) site = drop_site(ticket, dstream, thr);
  const T* xr = x + row * D;
  float v[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Vec4<T>::ld(xr, (int64_t)(k * 256 + lane * 4), v[k]);
    if (res != nullptr) {  // s = x + h, stored and normalised at storage precision
      float hv[4];
      Vec4<T>::ld(res + row * D, (int64_t)(k * 256 + lane * 4), hv);
      if constexpr (DROP) {
        const uint32_t mw = drop_flat_word(site, (uint64_t)(row * D + k * 256 + lane * 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = drop_keep(mw, j, site.thr) ? round_to<T>(hv[j] * site.scale) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = round_to<T>(v[k][j] + hv[j]);
      Vec4<T>::st(sum_out + row * D, (int64_t)(k * 256 + lane * 4), v[k]);
    }
  }
  float mean, rstd;
  ln_stats<K>(v, eps, mean, rstd);
  T* yr = y + row * D;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = k * 256 + lane * 4;
    float wv[4], bv[4], o[4];
    Vec4<float>::ld(w, c, wv);
    Vec4<float>::ld(b, c, bv);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ln_val(v[k][j], mean, rstd, wv[j], bv[j]);
    Vec4<T>::st(yr, (int64_t)c, o);
  }
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}

// LayerNorm (+ residual add) whose output goes straight to e4m3 for the fp8 GEMM that consumes it
// (ops/fp8.py Fp8Act: a transformer block's qkv and fc1 inputs). Unfused, the bf16 y was written
// here and read back by a cast-transpose pass; now the kernel writes y as fp8 row-major AND
// transposed (the layouts the forward and the weight-gradient GEMMs take), scaled by the consumer's
// delayed scale, with |y|max folded into its amax slot. y is rounded to bf16 before quantizing, so
// the bytes equal the unfused chain's. A workgroup owns 32 rows (8 waves x 4 rows, every row's loads
// issued before any row's math: one exposed latency per wave); the fp8 rows also go to an LDS image (row pitch D + 4 bytes: the transposed
// readers' 8-row blocks hit distinct banks) from which the transposed 32-B row segments are written.
// Tiles are placed XCD-aware so the four tiles sharing a 128-B line of y^T write it through one L2.
template <int K>
__global__ __launch_bounds__(512) void ln_fwd_fp8_kernel(const uint16_t* __restrict__ x,
                                                         const uint16_t* __restrict__ res,
                                                         const float* __restrict__ w, const float* __restrict__ b,
                                                         uint16_t* __restrict__ sum_out, uint8_t* __restrict__ yq,
                                                         uint8_t* __restrict__ yqt, float* __restrict__ mean_out,
                                                         float* __restrict__ rstd_out, int64_t N, float eps,
                                                         const float* __restrict__ scale, float* __restrict__ amax,
                                                         int striped) {
  constexpr int D = 256 * K, kRows = 32, kPitch = D + 4;
  __shared__ __attribute__((aligned(16))) uint8_t tile[kRows * kPitch];
  __shared__ float red[8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * kRows;
  const float s8 = *scale;
  float wr[K][4], br[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Vec4<float>::ld(w, k * 256 + lane * 4, wr[k]);
    Vec4<float>::ld(b, k * 256 + lane * 4, br[k]);
  }
  float am = 0.f;
  {
    constexpr int r0 = 0;
    uint2 xv[4][K], hv[4][K];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = m0 + wv * 4 + r0 + q;
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
      const int tr = wv * 4 + r0 + q;
      const int64_t row = m0 + tr;
      if (row >= N) continue;  // wave-uniform
      float v[K][4];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        v[k][0] = __uint_as_float(xv[q][k].x << 16); v[k][1] = __uint_as_float(xv[q][k].x & 0xffff0000u);
        v[k][2] = __uint_as_float(xv[q][k].y << 16); v[k][3] = __uint_as_float(xv[q][k].y & 0xffff0000u);
        if (res != nullptr) {  // s = x + h, stored and normalised at storage precision (as ln_fwd_kernel)
          const float hh[4] = {__uint_as_float(hv[q][k].x << 16), __uint_as_float(hv[q][k].x & 0xffff0000u),
                               __uint_as_float(hv[q][k].y << 16), __uint_as_float(hv[q][k].y & 0xffff0000u)};
#pragma unroll
          for (int j = 0; j < 4; ++j) v[k][j] = round_to<uint16_t>(v[k][j] + hh[j]);
          Vec4<uint16_t>::st(sum_out + row * D, (int64_t)(k * 256 + lane * 4), v[k]);
        }
      }
      float mean, rstd;
      ln_stats<K>(v, eps, mean, rstd);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = round_to<uint16_t>(ln_val(v[k][j], mean, rstd, wr[k][j], br[k][j]));
          am = fmaxf(am, fabsf(o[j]));
        }
        const uint32_t pk = pack4_fp8(o[0] * s8, o[1] * s8, o[2] * s8, o[3] * s8);
        *reinterpret_cast<uint32_t*>(yq + row * D + k * 256 + lane * 4) = pk;
        *reinterpret_cast<uint32_t*>(tile + tr * kPitch + k * 256 + lane * 4) = pk;
      }
      if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    }
  }
  __syncthreads();
  // y^T: item (word column g, 8-row block rb) -> 4 rows of y^T, 8 bytes each; N % 16 == 0 keeps
  // 8-row blocks whole
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

// Backward: dx per row; per-block partial dgamma/dbeta written to part[blk][2][D].
// DROP: a second output dh = round_T(dx * m * scale), the gradient of the dropped residual branch
// (dx as stored, i.e. rounded to T first: what a separate dropout backward would have read). It is
// formed in a second loop at the end of the kernel, each lane re-reading the dx values it wrote
// itself (its own stores, still in L2: no HBM read). Forming dh next to dx in the main loop changed
// how the compiler vectorised and contracted the dx / dgamma / dbeta arithmetic (1-ulp differences
// from the non-DROP instantiation); with the main loop's code left exactly as it is, the DROP kernel's
// dx, dgamma, dbeta equal the non-DROP kernel's bit for bit.
template <typename T, int K, bool DROP = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const T* __restrict__ dres,
                                                     const float* __restrict__ w, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, T* __restrict__ dx,
                                                     float* __restrict__ part, int64_t N, int rows_per_block,
                                                     T* __restrict__ dh = nullptr,
                                                     const int64_t* __restrict__ ticket = nullptr, int dstream = 0,
                                                     int thr = 0) {
  constexpr int D = 256 * K;
  DropSite site;
  if constexpr (DROP) site = drop_site(ticket, dstream, thr);
  __shared__ float sdw[4][D];
  __shared__ float sdb[4][D];
  const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
  float dw[K][4], db[K][4], wr[K][4];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Vec4<float>::ld(w, k * 256 + lane * 4, wr[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { dw[k][j] = 0.f; db[k][j] = 0.f; }
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(N, r0 + rows_per_block);
  // RF rows per wave in flight (rows r, r + 4, ...): all loads of them are issued before any
  // row's math, so a wave exposes the memory latency once per RF rows (single-row: 2.5 TB/s)
  constexpr int RF = K <= 4 ? 4 : 2;
  for (int64_t row0 = r0 + wv_id; row0 < r1; row0 += 4 * RF) {
    float g[RF][K][4], xh[RF][K][4], rr[RF][K][4];
    float mu[RF], rs[RF];
    bool ok[RF];
#pragma unroll
    for (int q = 0; q < RF; ++q) {
      const int64_t row = row0 + 4 * q;
      ok[q] = row < r1;
      const int64_t rw = ok[q] ? row : row0;  // duplicate load for a missing second row, result unused
      mu[q] = mean[rw];
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
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          xh[q][k][j] = (xh[q][k][j] - mu[q]) * rs[q];
          db[k][j] += g[q][k][j];
          dw[k][j] += g[q][k][j] * xh[q][k][j];
          const float gw = g[q][k][j] * wr[k][j];
          s1 += gw;
          s2 += gw * xh[q][k][j];
        }
      s1 = wave_sum(s1) * (1.f / D);
      s2 = wave_sum(s2) * (1.f / D);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = rs[q] * (g[q][k][j] * wr[k][j] - s1 - xh[q][k][j] * s2);
          if (dres != nullptr) o[j] += rr[q][k][j];  // + the residual stream's own gradient
        }
        Vec4<T>::st(dx, row * D + k * 256 + lane * 4, o);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sdw[wv_id][k * 256 + lane * 4 + j] = dw[k][j];
      sdb[wv_id][k * 256 + lane * 4 + j] = db[k][j];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
    part[((int64_t)blockIdx.x * 2 + 0) * D + c] = sdw[0][c] + sdw[1][c] + sdw[2][c] + sdw[3][c];
    part[((int64_t)blockIdx.x * 2 + 1) * D + c] = sdb[0][c] + sdb[1][c] + sdb[2][c] + sdb[3][c];
  }
  if constexpr (DROP) {  // the same (row, k, lane) ownership as the stores of dx above
    for (int64_t row = r0 + wv_id; row < r1; row += 4) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int64_t c = row * D + k * 256 + lane * 4;
        float o[4];
        Vec4<T>::ld(dx, c, o);
        const uint32_t mw = drop_flat_word(site, (uint64_t)c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = drop_keep(mw, j, site.thr) ? o[j] * site.scale : 0.f;
        Vec4<T>::st(dh, c, o);
      }
    }
  }
}

// Workgroup cap (PDT_LN_BWD_BLOCKS, read once; A/B): 512 = 2 workgroups per CU.
inline int64_t ln_bwd_cap() {
  static int64_t cap = 0;
  if (cap == 0) {
    const char* e = getenv("PDT_LN_BWD_BLOCKS");
    const int64_t v = (e && e[0]) ? strtol(e, nullptr, 10) : 512;
    cap = v >= 64 && v <= 4096 ? v : 512;
  }
  return cap;
}

// Minimum rows per workgroup (PDT_LN_BWD_ROWS, read once; A/B): 32 = 8 rows per wave.
inline int64_t ln_bwd_min_rows() {
  static int64_t r = 0;
  if (r == 0) {
    const char* e = getenv("PDT_LN_BWD_ROWS");
    const int64_t v = (e && e[0]) ? strtol(e, nullptr, 10) : 32;
    r = v >= 4 && v <= 256 ? v : 32;
  }
  return r;
}

// The backward's partition; the dgamma/dbeta slab is nblk x 2 x D floats.
inline int ln_bwd_blocks(int64_t N, int& rows_per_block) {
  return row_blocks(N, ln_bwd_min_rows(), ln_bwd_cap(), rows_per_block);
}

// pdt_ln_fwd (DROP = false: ticket = nullptr, dstream = thr = 0) and pdt_ln_fwd_drop.
template <bool DROP>
int ln_fwd(const void* x, const void* res, int dtype, const float* w, const float* b, void* y, void* sum_out,
           float* mean, float* rstd, int64_t N, int D, float eps, const int64_t* ticket, int dstream, int thr,
           hipStream_t s) {
  if (D % 256 != 0) return -1;
  if (N == 0) return 0;
  const dim3 grid((unsigned)((N + kRowsPerBlock - 1) / kRowsPerBlock));
  const auto launch = [&](auto kc) {
    with_elem(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((ln_fwd_kernel<T, decltype(kc)::value, DROP>), grid, dim3(256), 0, s, (const T*)x,
                         (const T*)res, w, b, (T*)y, (T*)sum_out, mean, rstd, N, eps, ticket, dstream, thr);
    });
  };
  // DROP stops at K = 8 as its backward does (ln_bwd below: the dropout form exists for training only)
  if constexpr (DROP) return with_k<1, 2, 3, 4, 5, 6, 8>(D / 256, launch) ? 0 : -1;
  else return with_k<1, 2, 3, 4, 5, 6, 8, 10, 12, 16>(D / 256, launch) ? 0 : -1;
}

// pdt_ln_bwd (DROP = false: dh = ticket = nullptr, dstream = thr = 0) and pdt_ln_bwd_drop. An empty input
// launches only the finalize, over no slabs: dw = db = 0.
template <bool DROP>
int ln_bwd(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* mean,
           const float* rstd, void* dx, void* dh, float* dw, float* db, int64_t N, int D, float* ws,
           const int64_t* ticket, int dstream, int thr, hipStream_t s) {
  if (D % 256 != 0 || D > 2048) return -1;
  int rpb;
  const int nblk = ln_bwd_blocks(N, rpb);
  const auto launch = [&](auto kc) {
    with_elem(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      hipLaunchKernelGGL((ln_bwd_kernel<T, decltype(kc)::value, DROP>), dim3(nblk), dim3(256), 0, s, (const T*)dy,
                         (const T*)x, (const T*)dres, w, mean, rstd, (T*)dx, ws, N, rpb, (T*)dh, ticket, dstream,
                         thr);
    });
  };
  // K <= 8 (the forward goes to 16): the kernel's LDS is 2 x 4 x D floats, 64 KB at D = 2048
  if (nblk > 0 && !with_k<1, 2, 3, 4, 5, 6, 8>(D / 256, launch)) return -1;
  hipLaunchKernelGGL((colsum_finalize_kernel<2, float>), dim3((D + 15) / 16), dim3(256), 0, s, ws, nblk, D, dw, db);
  return 0;
}

}  // namespace

extern "C" {

int64_t pdt_ln_workspace_floats(int64_t N, int D) {
  int rpb;
  return (int64_t)ln_bwd_blocks(N, rpb) * 2 * D;
}

// res / sum_out: optional residual branch h and the stored sum s = x + h (both or neither).
int pdt_ln_fwd(const void* x, const void* res, int dtype, const float* w, const float* b, void* y, void* sum_out,
               float* mean, float* rstd, int64_t N, int D, float eps, hipStream_t s) {
  if ((res == nullptr) != (sum_out == nullptr)) return -2;
  return ln_fwd<false>(x, res, dtype, w, b, y, sum_out, mean, rstd, N, D, eps, nullptr, 0, 0, s);
}

// bf16 x (+ res -> sum_out) -> LayerNorm -> e4m3 yq [N, D] and yq^T [D, N] (scale / amax: the
// consumer's fp8 state row). N % 16 == 0; D = 256 K.
int pdt_ln_fwd_fp8(const uint16_t* x, const uint16_t* res, const float* w, const float* b, uint16_t* sum_out,
                   uint8_t* yq, uint8_t* yqt, float* mean, float* rstd, int64_t N, int D, float eps,
                   const float* scale, float* amax, int striped, hipStream_t s) {
  if ((res == nullptr) != (sum_out == nullptr)) return -2;
  if (D % 256 != 0 || N % 16 != 0) return -1;
  if (N == 0) return 0;
  const dim3 grid((unsigned)((N + 31) / 32));
  // K in {2, .., 6}, shorter than pdt_ln_fwd's list: K = 8 would spill (a wave holds 4 rows of x and h)
  const bool ok = with_k<2, 3, 4, 5, 6>(D / 256, [&](auto kc) {
    hipLaunchKernelGGL((ln_fwd_fp8_kernel<decltype(kc)::value>), grid, dim3(512), 0, s, x, res, w, b, sum_out, yq, yqt,
                       mean, rstd, N, eps, scale, amax, striped);
  });
  return ok ? 0 : -1;
}

// Residual dropout inside add+LayerNorm: s = x + dropout(res), y = LN(s). thr in 1..255.
int pdt_ln_fwd_drop(const void* x, const void* res, int dtype, const float* w, const float* b, void* y,
                    void* sum_out, float* mean, float* rstd, int64_t N, int D, float eps, const int64_t* ticket,
                    int dstream, int thr, hipStream_t s) {
  if (res == nullptr || sum_out == nullptr || ticket == nullptr || thr < 1 || thr > 255) return -2;
  return ln_fwd<true>(x, res, dtype, w, b, y, sum_out, mean, rstd, N, D, eps, ticket, dstream, thr, s);
}

// dres: optional gradient added into dx (residual stream), same dtype/layout as dx.
int pdt_ln_bwd(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* mean,
               const float* rstd, void* dx, float* dw, float* db, int64_t N, int D, float* ws, hipStream_t s) {
  return ln_bwd<false>(dy, x, dres, dtype, w, mean, rstd, dx, nullptr, dw, db, N, D, ws, nullptr, 0, 0, s);
}

// The backward of pdt_ln_fwd_drop: dx as pdt_ln_bwd, and dh = dropout-backward of dx.
int pdt_ln_bwd_drop(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* mean,
                    const float* rstd, void* dx, void* dh, float* dw, float* db, int64_t N, int D, float* ws,
                    const int64_t* ticket, int dstream, int thr, hipStream_t s) {
  if (dh == nullptr || ticket == nullptr || thr < 1 || thr > 255) return -2;
  return ln_bwd<true>(dy, x, dres, dtype, w, mean, rstd, dx, dh, dw, db, N, D, ws, ticket, dstream, thr, s);
}

}  // extern "C"
