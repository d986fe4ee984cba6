// Dropout with counter-generated masks (csrc/philox.h) for gfx950.
//
// Not in the reference (no dropout anywhere in it); serves the GPT-2 / ViT configs.
//   dropout_begin_kernel  the per-forward ticket (key, step) and the step counter's increment
//   dropout_kernel        y = round_T(x * m * scale): the embedding site and the unfused block path;
//                         the backward is the same kernel on dy. One thread per 16-element Philox
//                         block (one call, every byte used), 16-byte accesses.
//   dropout_mask_*        the bool mask itself, through the same device functions the fused kernels
//                         (layernorm.hip, attention.hip) inline: what the tests compare with the CPU.
#include "../common.h"
#include "../dispatch.h"
#include "../launchers.h"
#include "../philox.h"

using namespace pdt;

namespace {

// state = (key, step) on the device: the key too, so a set_state() after a hipGraph capture is seen
__global__ void dropout_begin_kernel(int64_t* __restrict__ state, int64_t* __restrict__ ticket) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int64_t s = state[1];
    ticket[0] = state[0];
    ticket[1] = s;
    state[1] = s + 1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n,
                                                      const int64_t* __restrict__ ticket, int stream, int thr) {
  const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i0 = blk * 16;
  if (i0 >= n) return;
  const DropSite site = drop_site(ticket, stream, thr);
  const PhiloxOut o = drop_block(site, (uint64_t)blk);
  if (i0 + 16 <= n) {
    float v[16];
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
      for (int q = 0; q < 4; ++q) Vec4<float>::ld(x, i0 + 4 * q, *reinterpret_cast<float(*)[4]>(&v[4 * q]));
    } else {
      ld8_bf16(x + i0, *reinterpret_cast<float(*)[8]>(&v[0]));
      ld8_bf16(x + i0 + 8, *reinterpret_cast<float(*)[8]>(&v[8]));
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = drop_keep(o.w[e >> 2], e & 3, site.thr) ? v[e] * site.scale : 0.f;
    if constexpr (std::is_same<T, float>::value) {
#pragma unroll
      for (int q = 0; q < 4; ++q) Vec4<float>::st(y, i0 + 4 * q, *reinterpret_cast<float(*)[4]>(&v[4 * q]));
    } else {
      st8_bf16(y + i0, *reinterpret_cast<float(*)[8]>(&v[0]));
      st8_bf16(y + i0 + 8, *reinterpret_cast<float(*)[8]>(&v[8]));
    }
  } else {  // the last, partial block
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (i0 + e < n) {
        const float xv = Elt<T>::ld(x, i0 + e);
        Elt<T>::st(y, i0 + e, drop_keep(o.w[e >> 2], e & 3, site.thr) ? xv * site.scale : 0.f);
      }
  }
}

// bool mask, flat layout: thread per 4-element word, exactly as a LayerNorm lane asks for it
__global__ __launch_bounds__(256) void dropout_mask_flat_kernel(uint8_t* __restrict__ out, int64_t n,
                                                                const int64_t* __restrict__ ticket, int stream,
                                                                int thr) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  const DropSite site = drop_site(ticket, stream, thr);
  const uint32_t w = drop_flat_word(site, (uint64_t)i0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (i0 + r < n) out[i0 + r] = drop_keep(w, r, site.thr) ? 1 : 0;
}

// bool mask, attention layout [B*H, T, T]: thread per 4 x 4 patch
__global__ __launch_bounds__(256) void dropout_mask_attn_kernel(uint8_t* __restrict__ out, int64_t BH, int T,
                                                                const int64_t* __restrict__ ticket, int stream,
                                                                int thr) {
  const int TP = (T + 3) >> 2;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= BH * TP * TP) return;
  const int kp = (int)(id % TP), qp = (int)((id / TP) % TP);
  const int64_t bh = id / ((int64_t)TP * TP);
  const DropSite site = drop_site(ticket, stream, thr);
  const PhiloxOut o = drop_block(site, drop_attn_block((uint64_t)bh, TP, 4 * qp, 4 * kp));
#pragma unroll
  for (int qi = 0; qi < 4; ++qi)
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const int q = 4 * qp + qi, k = 4 * kp + ki;
      if (q < T && k < T) out[(bh * T + q) * T + k] = drop_keep(o.w[qi], ki, site.thr) ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int pdt_dropout_begin(int64_t* state, int64_t* ticket, hipStream_t s) {
  hipLaunchKernelGGL(dropout_begin_kernel, dim3(1), dim3(64), 0, s, state, ticket);
  return 0;
}

// x, y: n elements, 16-byte aligned; dtype 0 fp32, 1 bf16. thr in 1..255.
int pdt_dropout(const void* x, void* y, int dtype, int64_t n, const int64_t* ticket, int stream, int thr,
                hipStream_t s) {
  if (thr < 1 || thr > 255) return -1;
  if (n == 0) return 0;
  const int64_t nblk = (n + 15) / 16;
  const dim3 grid((unsigned)((nblk + 255) / 256));
  with_elem(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(dropout_kernel<T>, grid, dim3(256), 0, s, (const T*)x, (T*)y, n, ticket, stream, thr);
  });
  return 0;
}

int pdt_dropout_mask_flat(uint8_t* out, int64_t n, const int64_t* ticket, int stream, int thr, hipStream_t s) {
  if (thr < 0 || thr > 255) return -1;
  if (n == 0) return 0;
  const int64_t words = (n + 3) / 4;
  hipLaunchKernelGGL(dropout_mask_flat_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, out, n, ticket,
                     stream, thr);
  return 0;
}

int pdt_dropout_mask_attn(uint8_t* out, int64_t BH, int T, const int64_t* ticket, int stream, int thr,
                          hipStream_t s) {
  if (thr < 0 || thr > 255) return -1;
  if (BH == 0 || T == 0) return 0;
  const int64_t TP = (T + 3) >> 2, patches = BH * TP * TP;
  hipLaunchKernelGGL(dropout_mask_attn_kernel, dim3((unsigned)((patches + 255) / 256)), dim3(256), 0, s, out, BH, T,
                     ticket, stream, thr);
  return 0;
}

}  // extern "C"
