// Layer-wise adaptive optimizers for gfx950: LARS (You et al. 2017) and LAMB (You et al. 2019).
//
// Both scale each tensor's update by a trust ratio built from per-tensor L2 norms. The norms are
// deterministic by construction: no atomics, no arrival order.
//
//   norm pass   one workgroup per (tensor, 16 Ki-element chunk), the multi_tensor.h map. Each thread
//               adds its up to 64 squares in index order, block_sum (fixed lane pairing) combines the
//               256 threads, and thread 0 writes the chunk's two sums to partials[2 * blockIdx.x].
//               Every slot is written on every step, so the buffer needs no zero-fill.
//                 LARS: reads w, g;               writes (sum w^2, sum g^2)
//                 LAMB: reads w, g, m, v; writes the new m, v and (sum w^2, sum u^2)
//   finalize    one launch per batch, one wave per tensor: lane l adds partials l, l + 64, ... in index
//               order, the 64 lane sums meet in a fixed xor tree; all of it in double. Writes the two
//               sums (double) and the trust ratio (float). A separate kernel on purpose: a last-arriver
//               finalize inside the norm pass pays for device-scope fences (README, design notes).
//   update      reads ratio[t] once per workgroup and applies the step: fp32 master, states and the
//               bf16 model copy in one pass. A null ratio pointer means r = 1; LAMB then also does the
//               m, v update here (single pass, no norm pass launched).
//
// LAMB recomputes u in the update pass from the stored m, v through lamb_u(), the function the norm
// pass used (22 B + 18 B per element for bf16 parameters with a master copy, no parameter-sized
// scratch). Gradients are never written: under DDP they are views of the reduce buckets.
//
// All three kernels return at once when *found_inf != 0, so a skipped AMP step leaves weights, m, v
// and the momentum buffers bit for bit. lr, the inverse loss scale, the inf flag and LAMB's step count
// are read from device memory: a captured step replays with the current values.
#include "../multi_tensor.h"
#include "../launchers.h"

using namespace pdt;

namespace {

struct Common {
  float lr;
  const float* lr_ptr;
  const float* inv_scale;   // optional: grads are multiplied by *inv_scale
  const float* found_inf;   // optional: skip the step when *found_inf != 0
  float wd;
  int maximize;
  __device__ __forceinline__ bool enabled() const { return !(found_inf && *found_inf != 0.f); }
  __device__ __forceinline__ float get_lr() const { return lr_ptr ? *lr_ptr : lr; }
  __device__ __forceinline__ float gscale() const {
    float s = inv_scale ? *inv_scale : 1.f;
    return maximize ? -s : s;
  }
};

// This workgroup's (tensor, [start, end)) of the multi_tensor.h chunk map.
template <int NL>
__device__ __forceinline__ int chunk_of(const MTMeta<NL>& meta, int64_t& start, int64_t& end) {
  const int t = mt_find(meta, blockIdx.x);
  const int64_t c = blockIdx.x - meta.chunk_start[t];
  const int64_t n = meta.numel[t];
  start = c * PDT_MT_CHUNK;
  end = start + PDT_MT_CHUNK < n ? start + PDT_MT_CHUNK : n;
  return t;
}

// mt_kernel's walk over one chunk (aligned: 4-wide vectors, two in flight per lane, scalar tail;
// otherwise scalar) for a functor that keeps per-thread state.
template <int NL, typename F>
__device__ __forceinline__ void chunk_walk(const MTMeta<NL>& meta, int t, int64_t start, int64_t end, F& f) {
  if (mt_aligned(meta, t)) {
    const int64_t vend = start + ((end - start) & ~(int64_t)3);
    int64_t i = start + threadIdx.x * 4;
    for (; i + 1024 < vend; i += 2048) {
      f.vec4(i);
      f.vec4(i + 1024);
    }
    for (; i < vend; i += 1024) f.vec4(i);
    for (int64_t j = vend + threadIdx.x; j < end; j += 256) f.scalar(j);
  } else {
    for (int64_t i = start + threadIdx.x; i < end; i += 256) f.scalar(i);
  }
}

__device__ __forceinline__ void write_partials(float a, float b, float* partials) {
  __shared__ float red[4];
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = a;
    partials[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

// ---------------------------------------------------------------- LARS
// lists: 0 param (P), 1 grad (G), 2 momentum buf (f32, may be null), 3 model copy (bf16, may be null)
struct LarsHyper {
  float momentum, dampening;
  int nesterov, first;
};

template <typename P, typename G>
struct LarsNorm {
  const P* w;
  const G* g;
  float sc, sw, sg;
  __device__ __forceinline__ void vec4(int64_t i) {
    float a[4], b[4];
    Vec4<P>::ld(w, i, a);
    Vec4<G>::ld(g, i, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = b[k] * sc;
      sw += a[k] * a[k];
      sg += gk * gk;
    }
  }
  __device__ __forceinline__ void scalar(int64_t i) {
    const float a = Elt<P>::ld(w, i), gk = Elt<G>::ld(g, i) * sc;
    sw += a * a;
    sg += gk * gk;
  }
};

template <typename P, typename G>
__global__ __launch_bounds__(256) void lars_norm_kernel(MTMeta<4> meta, Common c, float* partials) {
  if (!c.enabled()) return;
  int64_t start, end;
  const int t = chunk_of(meta, start, end);
  LarsNorm<P, G> f{(const P*)meta.ptr[0][t], (const G*)meta.ptr[1][t], c.gscale(), 0.f, 0.f};
  chunk_walk(meta, t, start, end, f);
  write_partials(f.sw, f.sg, partials);
}

template <typename P, typename G>
struct LarsUpdate {
  P* w;
  const G* g;
  float* buf;
  uint16_t* copy;
  LarsHyper h;
  float lr, sc, wd, r;
  __device__ __forceinline__ void step(float& p, float gk, float& b) const {
    float d = r * (gk + wd * p);
    if (buf) {
      b = h.first ? d : h.momentum * b + (1.f - h.dampening) * d;
      d = h.nesterov ? d + h.momentum * b : b;
    }
    p -= lr * d;
  }
  __device__ __forceinline__ void vec4(int64_t i) {
    float p[4], gk[4], b[4] = {0, 0, 0, 0};
    Vec4<P>::ld(w, i, p);
    Vec4<G>::ld(g, i, gk);
    if (buf && !h.first) Vec4<float>::ld(buf, i, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) step(p[k], gk[k] * sc, b[k]);
    Vec4<P>::st(w, i, p);
    if (buf) Vec4<float>::st(buf, i, b);
    if (copy) Vec4<uint16_t>::st(copy, i, p);
  }
  __device__ __forceinline__ void scalar(int64_t i) {
    float p = Elt<P>::ld(w, i), gk = Elt<G>::ld(g, i) * sc, b = 0.f;
    if (buf && !h.first) b = buf[i];
    step(p, gk, b);
    Elt<P>::st(w, i, p);
    if (buf) buf[i] = b;
    if (copy) Elt<uint16_t>::st(copy, i, p);
  }
};

template <typename P, typename G>
__global__ __launch_bounds__(256) void lars_update_kernel(MTMeta<4> meta, Common c, LarsHyper h,
                                                          const float* ratio) {
  if (!c.enabled()) return;
  int64_t start, end;
  const int t = chunk_of(meta, start, end);
  LarsUpdate<P, G> f{(P*)meta.ptr[0][t], (const G*)meta.ptr[1][t], (float*)meta.ptr[2][t],
                     (uint16_t*)meta.ptr[3][t], h, c.get_lr(), c.gscale(), c.wd, ratio ? ratio[t] : 1.f};
  chunk_walk(meta, t, start, end, f);
}

// ---------------------------------------------------------------- LAMB
// lists: 0 param, 1 grad, 2 exp_avg (f32), 3 exp_avg_sq (f32), 4 model copy (bf16, may be null)
struct LambHyper {
  float beta1, beta2, eps;
  const float* step_ptr;  // step count AFTER increment (device)
  float step_host;
};

struct LambCoef {
  float beta1, beta2, eps, wd, bc1, bc2;
  __device__ __forceinline__ LambCoef(const LambHyper& h, float wd_) {
    beta1 = h.beta1;
    beta2 = h.beta2;
    eps = h.eps;
    wd = wd_;
    const float st = h.step_ptr ? *h.step_ptr : h.step_host;
    bc1 = 1.f - powf(beta1, st);
    bc2 = 1.f - powf(beta2, st);
  }
  __device__ __forceinline__ void moments(float g, float& m, float& v) const {
    m = m + (1.f - beta1) * (g - m);
    v = beta2 * v + (1.f - beta2) * g * g;
  }
};

// The update direction. The norm pass and the update pass both call this on the same stored m, v: one
// explicit instruction sequence (no contraction left to the optimiser), so both see the same bits.
__device__ __forceinline__ float lamb_u(float w, float m, float v, const LambCoef& k) {
  const float q = __fdiv_rn(__fdiv_rn(m, k.bc1), __fadd_rn(__fsqrt_rn(__fdiv_rn(v, k.bc2)), k.eps));
  return __fmaf_rn(k.wd, w, q);
}

template <typename P, typename G>
struct LambNorm {
  const P* w;
  const G* g;
  float* m;
  float* v;
  LambCoef k;
  float sc, sw, su;
  __device__ __forceinline__ void vec4(int64_t i) {
    float a[4], b[4], mm[4], vv[4];
    Vec4<P>::ld(w, i, a);
    Vec4<G>::ld(g, i, b);
    Vec4<float>::ld(m, i, mm);
    Vec4<float>::ld(v, i, vv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k.moments(b[j] * sc, mm[j], vv[j]);
      const float u = lamb_u(a[j], mm[j], vv[j], k);
      sw += a[j] * a[j];
      su += u * u;
    }
    Vec4<float>::st(m, i, mm);
    Vec4<float>::st(v, i, vv);
  }
  __device__ __forceinline__ void scalar(int64_t i) {
    const float a = Elt<P>::ld(w, i);
    float mm = m[i], vv = v[i];
    k.moments(Elt<G>::ld(g, i) * sc, mm, vv);
    const float u = lamb_u(a, mm, vv, k);
    sw += a * a;
    su += u * u;
    m[i] = mm;
    v[i] = vv;
  }
};

template <typename P, typename G>
__global__ __launch_bounds__(256) void lamb_norm_kernel(MTMeta<5> meta, Common c, LambHyper h, float* partials) {
  if (!c.enabled()) return;
  int64_t start, end;
  const int t = chunk_of(meta, start, end);
  LambNorm<P, G> f{(const P*)meta.ptr[0][t], (const G*)meta.ptr[1][t], (float*)meta.ptr[2][t],
                   (float*)meta.ptr[3][t], LambCoef(h, c.wd), c.gscale(), 0.f, 0.f};
  chunk_walk(meta, t, start, end, f);
  write_partials(f.sw, f.su, partials);
}

// MOMENTS: no norm pass ran (r = 1), so m and v are updated here.
template <typename P, typename G, bool MOMENTS>
struct LambUpdate {
  P* w;
  const G* g;
  float* m;
  float* v;
  uint16_t* copy;
  LambCoef k;
  float sc, lr_r;
  __device__ __forceinline__ void vec4(int64_t i) {
    float p[4], mm[4], vv[4];
    Vec4<P>::ld(w, i, p);
    Vec4<float>::ld(m, i, mm);
    Vec4<float>::ld(v, i, vv);
    if constexpr (MOMENTS) {
      float b[4];
      Vec4<G>::ld(g, i, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) k.moments(b[j] * sc, mm[j], vv[j]);
      Vec4<float>::st(m, i, mm);
      Vec4<float>::st(v, i, vv);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] -= lr_r * lamb_u(p[j], mm[j], vv[j], k);
    Vec4<P>::st(w, i, p);
    if (copy) Vec4<uint16_t>::st(copy, i, p);
  }
  __device__ __forceinline__ void scalar(int64_t i) {
    float p = Elt<P>::ld(w, i), mm = m[i], vv = v[i];
    if constexpr (MOMENTS) {
      k.moments(Elt<G>::ld(g, i) * sc, mm, vv);
      m[i] = mm;
      v[i] = vv;
    }
    p -= lr_r * lamb_u(p, mm, vv, k);
    Elt<P>::st(w, i, p);
    if (copy) Elt<uint16_t>::st(copy, i, p);
  }
};

template <typename P, typename G, bool MOMENTS>
__global__ __launch_bounds__(256) void lamb_update_kernel(MTMeta<5> meta, Common c, LambHyper h,
                                                          const float* ratio) {
  if (!c.enabled()) return;
  int64_t start, end;
  const int t = chunk_of(meta, start, end);
  LambUpdate<P, G, MOMENTS> f{(P*)meta.ptr[0][t], (const G*)meta.ptr[1][t], (float*)meta.ptr[2][t],
                              (float*)meta.ptr[3][t], (uint16_t*)meta.ptr[4][t], LambCoef(h, c.wd), c.gscale(),
                              c.get_lr() * (ratio ? ratio[t] : 1.f)};
  chunk_walk(meta, t, start, end, f);
}

// ---------------------------------------------------------------- finalize
struct ChunkMap {
  int chunk_start[PDT_MT_MAX_TENSORS + 1];
};

// kind 0 (LARS): (a, b) = (sum w^2, sum g^2), r = tc |w| / (|g| + wd |w| + eps)
// kind 1 (LAMB): (a, b) = (sum w^2, sum u^2), r = |w| / |u|
// r = 1 when either norm is zero.
__global__ __launch_bounds__(64) void finalize_kernel(ChunkMap cm, const float* partials, double* sums,
                                                      float* ratio, const float* found_inf, int kind, float tc,
                                                      float wd, float eps) {
  if (found_inf && *found_inf != 0.f) return;
  const int t = blockIdx.x, lane = threadIdx.x;
  const float2* p = reinterpret_cast<const float2*>(partials);
  double a = 0.0, b = 0.0;
  for (int i = cm.chunk_start[t] + lane; i < cm.chunk_start[t + 1]; i += 64) {
    const float2 x = p[i];
    a += (double)x.x;
    b += (double)x.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (lane == 0) {
    sums[2 * t] = a;
    sums[2 * t + 1] = b;
    double r = 1.0;
    if (a > 0.0 && b > 0.0) {
      const double wn = sqrt(a), on = sqrt(b);
      r = kind == 0 ? (double)tc * wn / (on + (double)wd * wn + (double)eps) : wn / on;
    }
    ratio[t] = (float)r;
  }
}

template <int NL>
ChunkMap chunk_map(const MTMeta<NL>& meta) {
  ChunkMap cm;
  for (int i = 0; i <= PDT_MT_MAX_TENSORS; ++i) cm.chunk_start[i] = i <= meta.ntensors ? meta.chunk_start[i] : 0;
  return cm;
}

bool any_empty(int n, const int64_t* numel) {
  for (int i = 0; i < n; ++i)
    if (numel[i] <= 0) return true;
  return false;
}

}  // namespace

extern "C" {

// Chunks (= norm-pass workgroups = partial slots of two floats) of a tensor list.
int64_t pdt_layerwise_chunks(int n, const int64_t* numel) {
  int64_t c = 0;
  for (int i = 0; i < n; ++i) c += (numel[i] + PDT_MT_CHUNK - 1) / PDT_MT_CHUNK;
  return c;
}

// partials: 2 * pdt_layerwise_chunks floats; sums: 2 n doubles; ratio: n floats (tensor order).
// Zero-element tensors are refused (-2): mt_batches skips them, and ratio slots would shift.
// ratio == nullptr: r = 1, update pass only. norms_only: norm pass and finalize, no update.
int pdt_lars(int n, void* const* p, void* const* g, void* const* buf, void* const* copy, const int64_t* numel,
             int p_dtype, int g_dtype, float lr, const float* lr_ptr, float momentum, float dampening, float wd,
             int nesterov, int first, float tc, float eps, int maximize, const float* inv_scale,
             const float* found_inf, float* partials, double* sums, float* ratio, int norms_only, hipStream_t s) {
  if (any_empty(n, numel)) return -2;
  if (!ratio && norms_only) return -3;
  void* const* lists[4] = {p, g, buf, copy};
  const Common c{lr, lr_ptr, inv_scale, found_inf, wd, maximize};
  const LarsHyper h{momentum, dampening, nesterov, first};
  int64_t cbase = 0;
  int tbase = 0;
#define PDT_CASE(PT, GT)                                                                                        \
  mt_batches<4>(n, lists, numel, [&](const MTMeta<4>& meta, int nblocks) {                                      \
    if (ratio) {                                                                                                \
      hipLaunchKernelGGL((lars_norm_kernel<PT, GT>), dim3(nblocks), dim3(256), 0, s, meta, c,                   \
                         partials + 2 * cbase);                                                                 \
      hipLaunchKernelGGL(finalize_kernel, dim3(meta.ntensors), dim3(64), 0, s, chunk_map(meta),                 \
                         (const float*)(partials + 2 * cbase), sums + 2 * tbase, ratio + tbase, found_inf, 0,   \
                         tc, wd, eps);                                                                          \
    }                                                                                                           \
    if (!norms_only)                                                                                            \
      hipLaunchKernelGGL((lars_update_kernel<PT, GT>), dim3(nblocks), dim3(256), 0, s, meta, c, h,              \
                         (const float*)(ratio ? ratio + tbase : nullptr));                                      \
    cbase += nblocks;                                                                                           \
    tbase += meta.ntensors;                                                                                     \
  });                                                                                                           \
  return 0;
  if (p_dtype == 0 && g_dtype == 0) { PDT_CASE(float, float) }
  if (p_dtype == 0 && g_dtype == 1) { PDT_CASE(float, uint16_t) }
  if (p_dtype == 1 && g_dtype == 1) { PDT_CASE(uint16_t, uint16_t) }
  if (p_dtype == 1 && g_dtype == 0) { PDT_CASE(uint16_t, float) }
#undef PDT_CASE
  return -1;
}

int pdt_lamb(int n, void* const* p, void* const* g, void* const* m, void* const* v, void* const* copy,
             const int64_t* numel, int p_dtype, int g_dtype, float lr, const float* lr_ptr, float beta1, float beta2,
             float eps, float wd, const float* step_ptr, float step_host, int maximize, const float* inv_scale,
             const float* found_inf, float* partials, double* sums, float* ratio, int norms_only, hipStream_t s) {
  if (any_empty(n, numel)) return -2;
  if (!ratio && norms_only) return -3;
  void* const* lists[5] = {p, g, m, v, copy};
  const Common c{lr, lr_ptr, inv_scale, found_inf, wd, maximize};
  const LambHyper h{beta1, beta2, eps, step_ptr, step_host};
  int64_t cbase = 0;
  int tbase = 0;
#define PDT_CASE(PT, GT)                                                                                        \
  mt_batches<5>(n, lists, numel, [&](const MTMeta<5>& meta, int nblocks) {                                      \
    if (ratio) {                                                                                                \
      hipLaunchKernelGGL((lamb_norm_kernel<PT, GT>), dim3(nblocks), dim3(256), 0, s, meta, c, h,                \
                         partials + 2 * cbase);                                                                 \
      hipLaunchKernelGGL(finalize_kernel, dim3(meta.ntensors), dim3(64), 0, s, chunk_map(meta),                 \
                         (const float*)(partials + 2 * cbase), sums + 2 * tbase, ratio + tbase, found_inf, 1,   \
                         0.f, 0.f, 0.f);                                                                        \
      if (!norms_only)                                                                                          \
        hipLaunchKernelGGL((lamb_update_kernel<PT, GT, false>), dim3(nblocks), dim3(256), 0, s, meta, c, h,     \
                           (const float*)(ratio + tbase));                                                      \
    } else {                                                                                                    \
      hipLaunchKernelGGL((lamb_update_kernel<PT, GT, true>), dim3(nblocks), dim3(256), 0, s, meta, c, h,        \
                         (const float*)nullptr);                                                                \
    }                                                                                                           \
    cbase += nblocks;                                                                                           \
    tbase += meta.ntensors;                                                                                     \
  });                                                                                                           \
  return 0;
  if (p_dtype == 0 && g_dtype == 0) { PDT_CASE(float, float) }
  if (p_dtype == 0 && g_dtype == 1) { PDT_CASE(float, uint16_t) }
  if (p_dtype == 1 && g_dtype == 1) { PDT_CASE(uint16_t, uint16_t) }
  if (p_dtype == 1 && g_dtype == 0) { PDT_CASE(uint16_t, float) }
#undef PDT_CASE
  return -1;
}

}  // extern "C"
