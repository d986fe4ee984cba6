// SwiGLU (gated SiLU) on the packed gate/up GEMM output, forward/backward for gfx950.
//
// gu: [N, 2F] (bf16 / fp32), gate g = gu[:, :F], up projection u = gu[:, F:] (one GEMM with the packed
// [2F, D] weight). With sg = sigma(g) = 1 / (1 + e^-g):
//   forward   y[n, f] = round_T(g sg u)                                   [N, F]
//   backward  dg = dy u sg (1 + g (1 - sg)),   du = dy g sg               packed dgu [N, 2F], one pass
// sg is recomputed from gu in the backward; nothing but gu is saved. fp32 math on value pairs (swiglu_math.h,
// shared with the fp8-emitting forms in fp8.hip: packed multiplies / FMAs, one v_exp_f32 + one v_rcp_f32 per
// value). 1 - sg is formed as e^-g sg for g > 0, where the subtraction would cancel. F % 8 == 0: a lane owns
// 8 columns of one row, 16-byte accesses.
#include "../common.h"
#include "../dispatch.h"
#include "../launchers.h"
#include "../swiglu_math.h"

using namespace pdt;

namespace {

template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ y, int64_t items,
                                                         int F8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int64_t n = i / F8;
  const int c = (int)(i - n * F8) * 8;
  const int64_t F = (int64_t)F8 * 8;
  float g[8], u[8], o[8];
  Vec8<T>::ld(gu + n * 2 * F + c, g);
  Vec8<T>::ld(gu + n * 2 * F + F + c, u);
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const gf2 r = swiglu_fwd2(gf2{g[j], g[j + 1]}, gf2{u[j], u[j + 1]});
    o[j] = r.x;
    o[j + 1] = r.y;
  }
  Vec8<T>::st(y + n * F + c, o);
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ gu,
                                                         T* __restrict__ dgu, int64_t items, int F8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int64_t n = i / F8;
  const int c = (int)(i - n * F8) * 8;
  const int64_t F = (int64_t)F8 * 8;
  float d[8], g[8], u[8], og[8], ou[8];
  Vec8<T>::ld(dy + n * F + c, d);
  Vec8<T>::ld(gu + n * 2 * F + c, g);
  Vec8<T>::ld(gu + n * 2 * F + F + c, u);
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    gf2 rg, ru;
    swiglu_bwd2(gf2{d[j], d[j + 1]}, gf2{g[j], g[j + 1]}, gf2{u[j], u[j + 1]}, rg, ru);
    og[j] = rg.x; og[j + 1] = rg.y;
    ou[j] = ru.x; ou[j + 1] = ru.y;
  }
  Vec8<T>::st(dgu + n * 2 * F + c, og);
  Vec8<T>::st(dgu + n * 2 * F + F + c, ou);
}

inline int swiglu_grid(int64_t N, int F, int64_t& items, dim3& grid) {
  if (F <= 0 || F % 8 != 0 || N < 0) return -1;
  items = N * (F / 8);
  const int64_t nb = (items + 255) / 256;
  if (nb > 0x7fffffffLL) return -1;
  grid = dim3((unsigned)nb);
  return 0;
}

}  // namespace

extern "C" {

// gu [N, 2F] -> y [N, F]; both contiguous and 16-byte aligned, F % 8 == 0.
int pdt_swiglu_fwd(const void* gu, int dtype, void* y, int64_t N, int F, hipStream_t s) {
  int64_t items;
  dim3 grid;
  if (swiglu_grid(N, F, items, grid) != 0) return -1;
  if (items == 0) return 0;
  with_elem(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(swiglu_fwd_kernel<T>, grid, dim3(256), 0, s, (const T*)gu, (T*)y, items, F / 8);
  });
  return 0;
}

// dy [N, F], gu [N, 2F] -> dgu [N, 2F] = [dg | du].
int pdt_swiglu_bwd(const void* dy, const void* gu, int dtype, void* dgu, int64_t N, int F, hipStream_t s) {
  int64_t items;
  dim3 grid;
  if (swiglu_grid(N, F, items, grid) != 0) return -1;
  if (items == 0) return 0;
  with_elem(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(swiglu_bwd_kernel<T>, grid, dim3(256), 0, s, (const T*)dy, (const T*)gu, (T*)dgu, items, F / 8);
  });
  return 0;
}

}  // extern "C"
