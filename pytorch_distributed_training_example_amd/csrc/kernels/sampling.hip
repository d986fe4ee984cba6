// Fused temperature / top-k / top-p token sampler for gfx950: one launch turns logits [B, V] into tokens [B].
//
// Not in the reference (it has no generation); serves Llama.generate(sampler="fused") and ops/sampling.py,
// whose CPU implementation states the same semantics in torch:
//   1. NaN counts as -inf, +inf as the largest finite value of the dtype; a row with nothing above -inf
//      gives token 0 and a zero probs row.
//   2. M = row maximum; temperature 0 -> the lowest index with l == M (probs: one-hot).
//   3. top-k on the raw logits: t_k = k-th largest with multiplicity, K = {l >= t_k}, ties kept whole.
//   4. q_i = floor(exp((l_i - M) / T) * 2^32) as a 64-bit integer: every sum of masses below is an integer
//      sum, so no result depends on the order lanes, waves or atomics add in.
//   5. top-p: t_p = the largest value t with mass{K, l >= t} >= p * mass(K) (compared in fp64, exact for
//      masses < 2^53), P = {l >= t_p}. Every l >= t_k is in K, so the descent needs no K restriction.
//   6. r = floor(u * mass(P)) (fp64); token = lowest index of P whose inclusive prefix mass exceeds r.
//   7. probs = q / mass(P) on P (fp64 quotient rounded to fp32), 0 elsewhere.
//
// Work split: one workgroup of 1024 lanes per row. A lane owns chunks of 8 consecutive logits, chunk
// c = j * 1024 + tid in iteration j, so a wave covers 512 consecutive logits per iteration and (j, wave)
// blocks are in index order. The row is read from global memory once into an LDS image in its own dtype
// (bf16 stays packed: 64 KB at V = 32000 fp32, 32 KB in bf16), up to 128 KB; every later pass reads the
// image, each lane the chunks it wrote itself, so the image needs no barrier. Rows above 128 KB (bf16 past
// 65536 logits, fp32 past 32768) do not fit a CU's 160 KB and take the LDS = false instantiation, which
// re-reads the row through L2 on every pass. (A register-resident row was tried first: the passes unroll
// over it, and at 1024 lanes the 128-VGPR budget spilt to scratch from 32 logits a lane on.)
// A row may start at any element: chunks are cut at 16-byte boundaries of the address, `mis` elements
// before the row's first; whole chunks take 16-byte loads and edge chunks guarded element loads.
//
// Selection: a first histogram of (count, mass) over 256 bins of floor((M - l) * 8) - monotone in l, and
// spread over the bins where LLM logits crowd into two or three exponent bins of the raw key - then an
// exact radix descent over the monotone 16 / 32-bit key inside the bin that holds the threshold, 8 bits a
// pass, on LDS integer atomics only. Top-k descends by count and yields mass(K); top-p descends by mass
// from the same first histogram. A wave whose 64 elements all fall into one bin adds one pre-summed pair
// instead of 64 same-address atomics (constant or masked rows). The inverse CDF is two-level: per (j, wave)
// block masses, one wave scan over them, one wave scan inside the block that holds r.
#include <math.h>

#include "../common.h"
#include "../launchers.h"
#include "../philox.h"

using namespace pdt;

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 256;
constexpr int kMaxV = 131072;
constexpr int kMaxBlocks = ((kMaxV + 7) / 8 + 1 + kThreads - 1) / kThreads * kWaves;  // 17 iterations of 16 waves
constexpr int kBlocksPerLane = (kMaxBlocks + 63) / 64;
constexpr float kBinScale = 8.f;
constexpr int kMaxRowLds = 128 * 1024;  // the row image; the histograms and block masses add 8.5 KB (160 KB per CU)

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {  // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, int lane) {  // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct ScanOut {
  int found, bin;
  uint32_t cnt_above, cnt_bin;
  u64 mass_above, mass_bin;
};

struct Smem {
  u64 mass1[kBins], mass2[kBins];
  uint32_t cnt1[kBins], cnt2[kBins];
  u64 blk[kMaxBlocks];
  float redf[kWaves];
  int redi[kWaves];
  ScanOut out;
  int bstar;
  u64 rem, total;
};

template <typename T> struct Lim;
template <> struct Lim<float> {
  static constexpr int kKeyBits = 32;
  __device__ static float top() { return 3.402823466e+38f; }
};
template <> struct Lim<uint16_t> {
  static constexpr int kKeyBits = 16;
  __device__ static float top() { return __uint_as_float(0x7F7F0000u); }
};

// Monotone unsigned key of a sanitised logit (no NaN, no -0): larger logit, larger key.
template <typename T>
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t k = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
  return Lim<T>::kKeyBits == 16 ? k >> 16 : k;
}

__device__ __forceinline__ int bin_of(float v, float M) { return (int)fminf((M - v) * kBinScale, (float)(kBins - 1)); }

__device__ __forceinline__ u64 mass_of(float v, float M, float T) { return (u64)(expf((v - M) / T) * 4294967296.f); }

// The row of one workgroup. LDS = true: copied once into `lds` (chunk c at word c * kWords, the lane that
// wrote a chunk is the only one that reads it: no barrier). LDS = false: re-read from global every pass.
template <typename T, bool LDS>
struct Row {
  static constexpr int kWords = sizeof(T) == 2 ? 4 : 8;  // 32-bit words of a chunk of 8
  const T* row;
  uint4* lds;
  int V, mis, nchunks, niter;

  __device__ __forceinline__ void load_chunk(int c, uint32_t (&w)[kWords]) const {
    const int i0 = c * 8 - mis;
    if (i0 >= 0 && i0 + 8 <= V) {  // 16-byte aligned by the choice of mis
      if constexpr (sizeof(T) == 2) {
        const uint4 t = *reinterpret_cast<const uint4*>(row + i0);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
      } else {
        const uint4 a = *reinterpret_cast<const uint4*>(row + i0), b = *reinterpret_cast<const uint4*>(row + i0 + 4);
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      }
    } else {  // an edge of the row, or past it: absent elements are -inf
      uint32_t e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k;
        e[k] = sizeof(T) == 2 ? 0xFF80u : 0xFF800000u;
        if (i >= 0 && i < V) {
          if constexpr (sizeof(T) == 2) e[k] = (uint32_t)row[i];
          else e[k] = __float_as_uint(row[i]);
        }
      }
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = e[2 * k] | (e[2 * k + 1] << 16);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = e[k];
      }
    }
  }

  __device__ __forceinline__ static void unpack(const uint32_t (&w)[kWords], float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = __uint_as_float(w[k] << 16);
        v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = __uint_as_float(w[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // NaN -> -inf, +inf -> largest finite, -0 -> +0
      const float x = v[k];
      v[k] = x != x ? -INFINITY : fminf(x, Lim<T>::top()) + 0.f;
    }
  }

  __device__ __forceinline__ void init(const T* row_, int V_, uint4* lds_) {
    row = row_;
    V = V_;
    lds = lds_;
    mis = (int)((reinterpret_cast<uintptr_t>(row_) & 15) / sizeof(T));
    nchunks = (V + mis + 7) / 8;
    niter = (nchunks + kThreads - 1) / kThreads;
    if constexpr (LDS) {
      for (int c = threadIdx.x; c < nchunks; c += kThreads) {
        uint32_t w[kWords];
        load_chunk(c, w);
        lds[c * (kWords / 4)] = make_uint4(w[0], w[1], w[2], w[3]);
        if constexpr (kWords == 8) lds[c * 2 + 1] = make_uint4(w[4], w[5], w[6], w[7]);
      }
    }
  }

  // f(j, c, v): iteration, chunk index, the chunk's 8 sanitised logits (element e has index c * 8 + e - mis;
  // a chunk past the row is all -inf). Every lane runs every iteration, so f may use wave-wide operations.
  template <class F>
  __device__ __forceinline__ void for_chunks(F&& f) const {
    for (int j = 0; j < niter; ++j) {
      const int c = j * kThreads + (int)threadIdx.x;
      uint32_t w[kWords];
      if constexpr (LDS) {
        if (c < nchunks) {
          const uint4 a = lds[c * (kWords / 4)];
          w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
          if constexpr (kWords == 8) {
            const uint4 b = lds[c * 2 + 1];
            w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
          }
        } else {
#pragma unroll
          for (int k = 0; k < kWords; ++k) w[k] = sizeof(T) == 2 ? 0xFF80FF80u : 0xFF800000u;
        }
      } else {
        load_chunk(c, w);
      }
      float v[8];
      unpack(w, v);
      f(j, c, v);
    }
  }
};

// One element per lane into the (count, mass) histogram; called by whole waves.
__device__ __forceinline__ void hist_add(bool member, uint32_t bin, u64 q, uint32_t* cnt, u64* mass, int lane) {
  const u64 m = __ballot(member);
  if (m == 0) return;
  const int first = __ffsll((long long)m) - 1;
  const uint32_t b0 = (uint32_t)__shfl((int)bin, first, 64);
  if (__ballot(member && bin == b0) == m) {  // one bin for the whole wave: one pre-summed pair
    const u64 s = wave_sum_u64(member ? q : 0);
    if (lane == first) {
      atomicAdd(&cnt[b0], (uint32_t)__popcll(m));
      atomicAdd(&mass[b0], s);
    }
  } else if (member) {
    atomicAdd(&cnt[bin], 1u);
    atomicAdd(&mass[bin], q);
  }
}

// Wave 0: the first bin (ascending = logits descending) at which the running count reaches kneed, or the
// running mass reaches mneed; base_* is what lies above bin 0. Not found: the totals in *_above.
__device__ __forceinline__ void scan_bins(const uint32_t* cnt, const u64* mass, bool by_count, uint32_t kneed,
                                          double mneed, uint32_t base_cnt, u64 base_mass, ScanOut* out, int lane) {
  uint32_t c[4], lc = 0;
  u64 m[4], lm = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c[q] = cnt[4 * lane + q];
    m[q] = mass[4 * lane + q];
    lc += c[q];
    lm += m[q];
  }
  const uint32_t ic = wave_scan_u32(lc, lane) + base_cnt;
  const u64 im = wave_scan_u64(lm, lane) + base_mass;
  const bool hit = by_count ? ic >= kneed : (double)im >= mneed;
  const u64 b = __ballot(hit);
  if (b == 0) {
    if (lane == 63) *out = ScanOut{0, kBins - 1, ic, 0u, im, 0ull};
    return;
  }
  if (lane == __ffsll((long long)b) - 1) {
    uint32_t ec = ic - lc;
    u64 em = im - lm;
    bool done = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool h = by_count ? ec + c[q] >= kneed : (double)(em + m[q]) >= mneed;
      if (h && !done) {
        *out = ScanOut{1, 4 * lane + q, ec, c[q], em, m[q]};
        done = true;
      }
      ec += c[q];
      em += m[q];
    }
  }
}

// The threshold key whose tail {key >= tkey} first reaches kneed elements or mneed mass, and that tail's
// mass; tkey 0 (every finite logit) when the whole row does not reach it. Needs the first histogram in sm.
template <typename T, bool LDS>
__device__ __forceinline__ void select(const Row<T, LDS>& row, Smem& sm, float M, float Tm, bool by_count,
                                       uint32_t kneed, double mneed, uint32_t& tkey, u64& mass_ge) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int KB = Lim<T>::kKeyBits;
  __syncthreads();
  if (wid == 0) scan_bins(sm.cnt1, sm.mass1, by_count, kneed, mneed, 0u, 0ull, &sm.out, lane);
  __syncthreads();
  ScanOut o = sm.out;
  if (!o.found) {
    tkey = 0;
    mass_ge = o.mass_above;
    return;
  }
  const int B1 = o.bin;
  uint32_t prefix = 0;
  for (int shift = KB - 8; shift >= 0; shift -= 8) {
    __syncthreads();
    if (tid < kBins) {
      sm.cnt2[tid] = 0;
      sm.mass2[tid] = 0;
    }
    __syncthreads();
    row.for_chunks([&](int, int, const float(&v)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t key = key_of<T>(v[e]);
        const bool mem = v[e] > -INFINITY && bin_of(v[e], M) == B1 && (uint32_t)((u64)key >> (shift + 8)) == prefix;
        const u64 q = mem ? mass_of(v[e], M, Tm) : 0;
        hist_add(mem, 255u - ((key >> shift) & 255u), q, sm.cnt2, sm.mass2, lane);  // digit 255 first
      }
    });
    __syncthreads();
    if (wid == 0) scan_bins(sm.cnt2, sm.mass2, by_count, kneed, mneed, o.cnt_above, o.mass_above, &sm.out, lane);
    __syncthreads();
    o = sm.out;
    prefix = (prefix << 8) | (uint32_t)(255 - o.bin);
  }
  tkey = prefix;
  mass_ge = o.mass_above + o.mass_bin;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(kThreads) void sample_kernel(const T* __restrict__ logits, int V,
                                                          const float* __restrict__ temperature,
                                                          const int* __restrict__ top_k,
                                                          const float* __restrict__ top_p, const float* __restrict__ u,
                                                          const int64_t* __restrict__ ticket, int philox_stream,
                                                          int64_t* __restrict__ tokens, float* __restrict__ probs) {
  __shared__ Smem sm;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x;
  float* prow = probs ? probs + (int64_t)b * V : nullptr;

  extern __shared__ __attribute__((aligned(16))) char dyn[];
  Row<T, LDS> row;
  row.init(logits + (int64_t)b * V, V, reinterpret_cast<uint4*>(dyn));
  const int mis = row.mis;

  float M = -INFINITY;
  row.for_chunks([&](int, int, const float(&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) M = fmaxf(M, v[e]);
  });
  M = block_max(M, sm.redf);

  const float Tm = temperature[b];
  if (!(M > -INFINITY) || !(Tm > 0.f)) {  // nothing to draw from, or greedy: the lowest index at the maximum
    int best = 0x7fffffff;
    if (M > -INFINITY)
      row.for_chunks([&](int, int c, const float(&v)[8]) {
#pragma unroll
        for (int e = 7; e >= 0; --e)
          if (v[e] == M) best = min(best, c * 8 + e - mis);
      });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if (lane == 0) sm.redi[wid] = best;
    __syncthreads();
    best = sm.redi[0];
    for (int w = 1; w < kWaves; ++w) best = min(best, sm.redi[w]);
    if (best == 0x7fffffff) best = -1;  // no finite logit: token 0, zero probs
    if (tid == 0) tokens[b] = best < 0 ? 0 : best;
    if (prow)
      for (int i = tid; i < V; i += kThreads) prow[i] = i == best ? 1.f : 0.f;
    return;
  }

  int k = top_k[b];
  k = k < 0 ? 0 : k;
  const float p = fminf(fmaxf(top_p[b], 1.17549435e-38f), 1.f);  // NaN -> the smallest p
  const bool need_k = k > 0 && k < V, need_p = p < 1.f;

  uint32_t tkey = 0;  // P = {finite, key >= tkey}
  if (need_k || need_p) {
    if (tid < kBins) {
      sm.cnt1[tid] = 0;
      sm.mass1[tid] = 0;
    }
    __syncthreads();
    row.for_chunks([&](int, int, const float(&v)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool mem = v[e] > -INFINITY;
        const u64 q = mem ? mass_of(v[e], M, Tm) : 0;
        hist_add(mem, (uint32_t)(mem ? bin_of(v[e], M) : 0), q, sm.cnt1, sm.mass1, lane);
      }
    });
    u64 massK = 0;
    if (need_k) select(row, sm, M, Tm, true, (uint32_t)k, 0.0, tkey, massK);
    if (need_p) {
      if (!need_k) {  // mass(K) = the whole row's: a count no row reaches leaves the totals
        uint32_t unused;
        select(row, sm, M, Tm, true, 0xffffffffu, 0.0, unused, massK);
      }
      u64 massP;
      select(row, sm, M, Tm, false, 0u, (double)p * (double)massK, tkey, massP);
    }
  }

  // Inverse CDF in index order, level 1: the mass of P in each (iteration, wave) block of 512 logits.
  __syncthreads();
  row.for_chunks([&](int j, int, const float(&v)[8]) {
    u64 s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (v[e] > -INFINITY && key_of<T>(v[e]) >= tkey) s += mass_of(v[e], M, Tm);
    s = wave_sum_u64(s);
    if (lane == 0) sm.blk[j * kWaves + wid] = s;
  });
  __syncthreads();
  if (wid == 0) {
    const int nblk = row.niter * kWaves;
    float uu;
    if (u) {
      uu = u[b];
    } else {
      const uint64_t key = (uint64_t)ticket[0], step = (uint64_t)ticket[1];
      const PhiloxOut o = philox4x32_10((uint32_t)b, 0u, (uint32_t)philox_stream, (uint32_t)step, (uint32_t)key,
                                        (uint32_t)(key >> 32));
      uu = (float)(o.w[0] >> 8) * 5.9604644775390625e-8f;  // 2^-24
    }
    u64 bm[kBlocksPerLane], ls = 0;
#pragma unroll
    for (int q = 0; q < kBlocksPerLane; ++q) {
      const int i = lane * kBlocksPerLane + q;
      bm[q] = i < nblk ? sm.blk[i] : 0;
      ls += bm[q];
    }
    const u64 inc = wave_scan_u64(ls, lane);
    const u64 total = __shfl(inc, 63, 64);  // > 0: the maximum itself weighs 2^32 and is in P
    u64 r = (u64)((double)fminf(fmaxf(uu, 0.f), 1.f) * (double)total);
    r = r >= total ? total - 1 : r;
    u64 exc = inc - ls;
    if (r >= exc && r < inc) {
      bool done = false;
#pragma unroll
      for (int q = 0; q < kBlocksPerLane; ++q) {
        if (!done && r < exc + bm[q]) {
          sm.bstar = lane * kBlocksPerLane + q;
          sm.rem = r - exc;
          done = true;
        }
        exc += bm[q];
      }
    }
    if (lane == 0) sm.total = total;
  }
  __syncthreads();
  const int bstar = sm.bstar;
  const u64 rem = sm.rem, total = sm.total;

  // Level 2: the wave that owns the block scans its 64 lane masses, the lane that holds r its 8 elements.
  row.for_chunks([&](int j, int c, const float(&v)[8]) {
    if (j * kWaves + wid != bstar) return;
    u64 qs[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qs[e] = v[e] > -INFINITY && key_of<T>(v[e]) >= tkey ? mass_of(v[e], M, Tm) : 0;
      s += qs[e];
    }
    const u64 inc = wave_scan_u64(s, lane);
    u64 exc = inc - s;
    if (rem >= exc && rem < inc) {
      bool done = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (!done && rem < exc + qs[e]) {
          tokens[b] = c * 8 + e - mis;
          done = true;
        }
        exc += qs[e];
      }
    }
  });

  if (prow) {
    const double inv_total = (double)total;
    row.for_chunks([&](int, int c, const float(&v)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = c * 8 + e - mis;
        if (i >= 0 && i < V) {
          const bool in = v[e] > -INFINITY && key_of<T>(v[e]) >= tkey;
          prow[i] = in ? (float)((double)mass_of(v[e], M, Tm) / inv_total) : 0.f;
        }
      }
    });
  }
}

template <typename T, bool LDS>
int launch(const void* logits, int B, int V, int lds, const float* temperature, const int* top_k, const float* top_p,
           const float* u, const int64_t* ticket, int philox_stream, int64_t* tokens, float* probs, hipStream_t s) {
  static bool attr = false;
  if (LDS && !attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<T, LDS>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxRowLds) != hipSuccess)
      return -4;
    attr = true;
  }
  hipLaunchKernelGGL((sample_kernel<T, LDS>), dim3(B), dim3(kThreads), LDS ? lds : 0, s, (const T*)logits, V,
                     temperature, top_k, top_p, u, ticket, philox_stream, tokens, probs);
  return 0;
}

}  // namespace

extern "C" {

int pdt_sample_logits(const void* logits, int dtype, int B, int V, const float* temperature, const int* top_k,
                      const float* top_p, const float* u, const int64_t* ticket, int philox_stream, int64_t* tokens,
                      float* probs, hipStream_t s) {
  if (B < 1 || B > 65535 || V < 1 || V > kMaxV || (dtype != 0 && dtype != 1)) return -1;
  if ((u == nullptr) == (ticket == nullptr)) return -2;
  if (reinterpret_cast<uintptr_t>(logits) % 16 != 0) return -3;
  const int es = dtype == 1 ? 2 : 4;
  // chunks are cut at 16-byte boundaries: rows that start off one need up to a chunk more
  const int span = V + (((int64_t)V * es) % 16 == 0 || B == 1 ? 0 : 16 / es - 1);
  const int lds = (span + 7) / 8 * 8 * es;
#define PDT_SAMPLE(T, L) \
  launch<T, L>(logits, B, V, lds, temperature, top_k, top_p, u, ticket, philox_stream, tokens, probs, s)
  if (dtype == 1) return lds <= kMaxRowLds ? PDT_SAMPLE(uint16_t, true) : PDT_SAMPLE(uint16_t, false);
  return lds <= kMaxRowLds ? PDT_SAMPLE(float, true) : PDT_SAMPLE(float, false);
#undef PDT_SAMPLE
}

}  // extern "C"
