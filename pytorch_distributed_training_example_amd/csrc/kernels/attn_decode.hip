// KV-cache decoding for gfx950, head dim 64, bf16: the cache append (rotary embedding at a per-sequence
// offset fused with the cache write), split-KV decode attention, and the merge of the splits.
//
// Cache: k, v [B, Hkv, capacity, 64] bf16, contiguous (one key row = one 128-byte line), K stored after
// rotation. lens: int32 [B] on the device, the number of valid positions per sequence. Nothing here reads
// lens on the host, so a captured graph replays with whatever the device holds; every kernel clamps the
// positions it derives from lens to the cache, so no value of lens can produce an out-of-bounds access.
//
// pdt_rope_kv_append: qkv [B, Tn, (H + 2 Hkv) 64] (c_attn's output for Tn new tokens). Row (b, t) sits at
// position p = lens[b] + t: the H query heads and the Hkv key heads are rotated in place with cos/sin[p]
// (rope_math.h: the bits of rope.hip at row p), the rotated keys also go to k[b, :, p] and the value heads,
// read once and not written in qkv, to v[b, :, p]. (K in place costs Hkv 128 bytes per token and lets a
// prefill run the causal flash forward on qkv as it stands.) A row with p outside [0, min(capacity, T_max))
// does nothing.
//
// pdt_attn_decode: one query row per (sequence, head), n[b] = lens[b] + 1 keys (the new token is already
// appended). Grid (S, Hkv, B): a workgroup owns one K/V head of one sequence and the C keys [s C, s C + C),
// C % 64 == 0, S = ceil(capacity / C) (pdt_attn_decode_geo: a function of the capacity, never of lens, so the
// grid of a captured graph never changes). It serves all G = H / Hkv query heads of the group from the same
// K/V fragments: the heads are the columns of the swapped S^T = K Q^T (attention.hip's layout: a lane owns
// one query head and 4 keys of a 16-key subtile), up to 16 per pass; G > 16 runs further passes over the
// chunk, which the workgroup has just pulled through L2. Wave w takes the 16-key subtiles w, w + 4, ... of
// the chunk, two per step:
//   K   straight to registers as the MFMA A operand (2 x 16 B per lane and subtile), no LDS;
//   V   through a wave-private LDS tile and ds_read_b64_tr_b16, because O^T = V^T P^T wants V^T with keys
//       along k and V is stored with d contiguous. P^T goes from the score accumulators to the B operand of
//       v_mfma_f32_16x16x16_bf16 unpermuted (accumulator row 4g + r is key 4g + r is k index 4g + r).
// All of a step's loads are issued before its first use. They are raw buffer loads over a resource of
// n[b] rows: a row at or past n[b] reads as zero in hardware, so whatever the cache holds there (NaN
// included) never reaches an MFMA, and the scores of those keys are set to -inf before the softmax.
// The four waves' (m, l, O) are merged through LDS in wave order, then either written as the split's fp32
// partial (o_part [B, H, S, 64] unnormalised, ml_part [B, H, S, 2] = (m, l), m in log2 units as the forward
// keeps it) or, for S == 1, normalised and stored as the bf16 output directly.
//
// pdt_attn_decode_combine: m = max_s m_s, l = sum_s l_s 2^(m_s - m), O = sum_s O_s 2^(m_s - m) / l, s in
// ascending order by one thread per output element: no atomics, the same bits every run.
// Output [B, 1, H 64] bf16 (what c_proj consumes) and optionally the LSE [B, H] (natural log).
#include "../common.h"
#include "../launchers.h"
#include "../rope_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int D = 64;
constexpr int ROW_BYTES = D * 2;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int U = 2;                       // 16-key subtiles per wave and step
constexpr int SUB_BYTES = 16 * ROW_BYTES;  // one subtile of V in LDS
constexpr uint32_t OOB = 0x80000000u;      // a buffer offset past any cache slice: the load returns zero

// ---------------------------------------------------------------- cache append
__global__ __launch_bounds__(256) void rope_kv_append_kernel(uint16_t* __restrict__ qkv, const float* __restrict__ cs,
                                                             const float* __restrict__ sn,
                                                             uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                             const int* __restrict__ lens, int64_t items, int Tn, int H,
                                                             int Hkv, int cap, int Tmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int AH = H + 2 * Hkv, per_tok = 4 * AH;  // 4 lanes per head, as in rope.hip
  const int64_t tok = i / per_tok;
  const int r = (int)(i - tok * per_tok);
  const int head = r >> 2, q = r & 3;
  const int b = (int)(tok / Tn), t = (int)(tok - (int64_t)b * Tn);
  const int64_t p = (int64_t)lens[b] + t;
  if (p < 0 || p >= cap || p >= Tmax) return;  // the device-side guard: such a row writes nothing
  uint16_t* src = qkv + tok * (int64_t)D * AH + head * D + q * 8;
  if (head >= H + Hkv) {  // V: copied, not rotated
    uint16_t* dst = vc + (((int64_t)b * Hkv + (head - H - Hkv)) * cap + p) * D + q * 8;
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    *reinterpret_cast<uint4*>(dst + 32) = *reinterpret_cast<const uint4*>(src + 32);
    return;
  }
  float lo[8], hi[8], olo[8], ohi[8];
  ld8_bf16(src, lo);
  ld8_bf16(src + 32, hi);
  rope_rotate8(lo, hi, cs + p * 32 + q * 8, sn + p * 32 + q * 8, 1.f, olo, ohi);
  st8_bf16(src, olo);  // in place, K included: a prefill's causal forward reads the rotated K from qkv
  st8_bf16(src + 32, ohi);
  if (head >= H) {
    uint16_t* dst = kc + (((int64_t)b * Hkv + (head - H)) * cap + p) * D + q * 8;
    st8_bf16(dst, olo);
    st8_bf16(dst + 32, ohi);
  }
}

// ---------------------------------------------------------------- decode attention
// LDS tile of V rows, 16-B chunks XOR-swizzled and read transposed: attention.hip's forward recipe.
__device__ __forceinline__ int swz(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Rows r0..r0+3, columns col0 + (lane & 15): element q of the result is row r0 + q.
__device__ __forceinline__ s4 lds_tr4(const char* tile, int r0, int col0, int lane) {
  const int li = lane & 15;
  const int row = r0 + (li >> 2);
  const int col = col0 + 4 * (li & 3);
  const int off = swz(row, col >> 3) + ((col & 4) << 1);
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(tile + off));
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// 2^(ms - m) as the weight of a partial with maximum ms under the merged maximum m: exactly 1 for the
// partial that holds the maximum, exactly 0 for an empty one (ms = -inf, also when m = -inf).
__device__ __forceinline__ float merge_weight(float ms, float m) {
  return ms == -INFINITY ? 0.f : (ms == m ? 1.f : fast_exp2(ms - m));
}

// Orders a wave's own LDS stores and loads around this point for the compiler (hardware keeps them in order).
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bf16x8 load8(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}

__global__ __launch_bounds__(256) void attn_decode_kernel(const uint16_t* __restrict__ qkv, int64_t q_sb,
                                                          const uint16_t* __restrict__ kc,
                                                          const uint16_t* __restrict__ vc, const int* __restrict__ lens,
                                                          float* __restrict__ o_part, float* __restrict__ ml_part,
                                                          uint16_t* __restrict__ out, float* __restrict__ lse, int H,
                                                          int Hkv, int cap, int C, float sl2) {
  __shared__ __attribute__((aligned(16))) char vs[4][U * SUB_BYTES];
  __shared__ __attribute__((aligned(16))) float mo[4][16][D];
  __shared__ float mm[4][16], ml[4][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = gridDim.x, sp = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = H / Hkv;
  const int n = min(max(lens[b] + 1, 0), cap);  // keys of this sequence, clamped to the cache
  const int c0 = sp * C, cend = min(c0 + C, n);
  const int nit = cend > c0 ? (cend - c0 + 63) >> 6 : 0;  // 64-key groups of the chunk that hold a valid key
  const int64_t slice = ((int64_t)b * Hkv + hk) * cap * D;
  // n rows of the slice: a load of row >= n is out of range and returns zero
  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(kc + slice), (short)0, n * ROW_BYTES, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(vc + slice), (short)0, n * ROW_BYTES, 0x00020000);
  char* vw = vs[w];

  for (int pass0 = 0; pass0 < G; pass0 += 16) {
    // Q^T as the B operand: lane (c, g) holds head pass0 + c, elements 32 s + 8 g .. + 8
    const int hq = pass0 + c;
    bf16x8 bq[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (hq < G) {
        bq[s] = *reinterpret_cast<const bf16x8*>(qkv + (int64_t)b * q_sb + (int64_t)(hk * G + hq) * D + 32 * s + 8 * g);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) bq[s][j] = (__bf16)0.f;
      }
    }
    f4 oacc[4];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) oacc[nn] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    for (int it = 0; it < nit; it += U) {
      // ---- all loads of the step first: K fragments, then V rows for the LDS tile
      bf16x8 ka[U][2], vr[U][2];
      int key0[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        key0[u] = c0 + 64 * (it + u) + 16 * w;  // >= cend when it + u >= nit: fully masked below
        const uint32_t base = it + u < nit ? (uint32_t)key0[u] * ROW_BYTES : OOB;
#pragma unroll
        for (int s = 0; s < 2; ++s) ka[u][s] = load8(krs, base + (uint32_t)(c * ROW_BYTES + (32 * s + 8 * g) * 2));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t base = it + u < nit ? (uint32_t)key0[u] * ROW_BYTES : OOB;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int id = lane + 64 * j;
          vr[u][j] = load8(vrs, base + (uint32_t)((id >> 3) * ROW_BYTES + (id & 7) * 16));
        }
      }
      // The tile is wave-private and a wave's LDS operations execute in program order, so no workgroup barrier
      // is needed: the wavefront-scope fences only keep the compiler from moving the tile's stores across the
      // transposed reads of this step or the previous one. They are expected to emit no instruction
      // (profiles/r18/decode_attention.txt records the loop's checked ISA).
      wave_lds_order();
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int id = lane + 64 * j;
          *reinterpret_cast<bf16x8*>(vw + u * SUB_BYTES + swz(id >> 3, id & 7)) = vr[u][j];
        }
      wave_lds_order();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        f4 st = {0.f, 0.f, 0.f, 0.f};
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[u][0], bq[0], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[u][1], bq[1], st, 0, 0, 0);
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (key0[u] + 4 * g + r >= cend) st[r] = -INFINITY;
          mt = fmaxf(mt, st[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt * sl2);
        const float alpha = (mn == -INFINITY) ? 1.f : fast_exp2(m - mn);
        const float msub = (mn == -INFINITY) ? 0.f : mn;
        float ls = 0.f;
        s4 pb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = fast_exp2(fmaf(st[r], sl2, -msub));
          ls += p;
          pb[r] = __builtin_bit_cast(short, (__bf16)p);
        }
        l = l * alpha + ls;
        m = mn;
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          oacc[nn] *= alpha;
          const s4 va = lds_tr4(vw + u * SUB_BYTES, 4 * g, 16 * nn, lane);
          oacc[nn] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(va, pb, oacc[nn], 0, 0, 0);
        }
      }
    }
    // ---- merge the four waves in wave order
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (g == 0) {
      mm[w][c] = m;
      ml[w][c] = l;
    }
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) *reinterpret_cast<f4*>(&mo[w][c][16 * nn + 4 * g]) = oacc[nn];
    __syncthreads();
    {
      const int qh = tid >> 4, d4 = (tid & 15) * 4;
      float M = -INFINITY;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, mm[ww][qh]);
      float L = 0.f;
      f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const float wt = merge_weight(mm[ww][qh], M);
        L += ml[ww][qh] * wt;
        o += *reinterpret_cast<const f4*>(&mo[ww][qh][d4]) * wt;
      }
      if (pass0 + qh < G) {
        const int64_t row = (int64_t)b * H + hk * G + pass0 + qh;
        if (S == 1) {
          const float inv = L > 0.f ? 1.f / L : 0.f;
          const float v4[4] = {o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv};
          Vec4<uint16_t>::st(out, row * D + d4, v4);
          if (lse && d4 == 0) lse[row] = (M + log2f(L)) * LN2;
        } else {
          *reinterpret_cast<f4*>(o_part + (row * S + sp) * D + d4) = o;
          if (d4 == 0) {
            ml_part[(row * S + sp) * 2] = M;
            ml_part[(row * S + sp) * 2 + 1] = L;
          }
        }
      }
    }
    __syncthreads();  // mo / mm / ml are rewritten by the next pass
  }
}

// One thread per output element; 4 (b, h) rows per workgroup.
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ o_part,
                                                                  const float* __restrict__ ml_part,
                                                                  uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                  int64_t rows, int S) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int d = threadIdx.x & 63;
  if (row >= rows) return;
  const float* mlr = ml_part + row * S * 2;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, mlr[2 * s]);
  float L = 0.f, o = 0.f;
  for (int s = 0; s < S; ++s) {
    const float wt = merge_weight(mlr[2 * s], M);
    L += mlr[2 * s + 1] * wt;
    o += o_part[(row * S + s) * D + d] * wt;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  out[row * D + d] = f2bf(o * inv);
  if (lse && d == 0) lse[row] = (M + log2f(L)) * LN2;
}

}  // namespace

extern "C" {

// Append the Tn new rows of qkv [B, Tn, (H + 2 Hkv) 64] at positions lens[b] + t of k, v [B, Hkv, cap, 64];
// Q is rotated in place. cos, sin: fp32 [Tmax, 32]. Everything contiguous and 16-byte aligned.
int pdt_rope_kv_append(uint16_t* qkv, const float* cos, const float* sin, uint16_t* k_cache, uint16_t* v_cache,
                       const int* lens, int B, int Tn, int H, int Hkv, int capacity, int Tmax, hipStream_t s) {
  if (B < 0 || Tn < 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || capacity <= 0 || Tmax <= 0) return -1;
  const int64_t items = (int64_t)B * Tn * 4 * (H + 2 * Hkv);
  if (items == 0) return 0;
  const int64_t grid = (items + 255) / 256;
  if (grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(rope_kv_append_kernel, dim3((unsigned)grid), dim3(256), 0, s, qkv, cos, sin, k_cache, v_cache,
                     lens, items, Tn, H, Hkv, capacity, Tmax);
  return 0;
}

// (S, C) into geo2 for a cache of `capacity` positions: C keys per workgroup (a multiple of 64), S =
// ceil(capacity / C) splits. splits_override > 0 asks for that many splits (fewer come out when 64-key
// granules do not divide that far). The default aims at two workgroups per CU (512) when B Hkv alone gives
// fewer, under three caps that keep the merge small next to the K/V read: a split writes and the combine
// reads G 264 bytes of fp32 partials per K/V head against the chunk's C 256 bytes of K and V, so
// C >= 16 G holds that traffic to an eighth; C >= 256, two steps per wave, because at 64 keys a workgroup's
// fixed cost (Q, the wave merge, the partial's store) outweighs its stream (measured: tools/decode_bench.py,
// 16 splits of 64 against 4 of 256 at 4 K/V heads); and S <= 64. G = H / Hkv.
int pdt_attn_decode_geo(int B, int Hkv, int capacity, int splits_override, int G, int* geo2) {
  if (B <= 0 || Hkv <= 0 || capacity <= 0 || G <= 0 || splits_override < 0) return -1;
  const int64_t granules = ((int64_t)capacity + 63) / 64;
  int64_t want = splits_override;
  int64_t cmin = 1;  // in granules
  if (want == 0) {
    want = (512 + (int64_t)B * Hkv - 1) / ((int64_t)B * Hkv);
    if (want > 64) want = 64;
    cmin = (16 * (int64_t)G + 63) / 64;
    if (cmin < 4) cmin = 4;
  }
  if (want > granules) want = granules;
  int64_t cg = (granules + want - 1) / want;
  if (cg < cmin) cg = cmin;
  if (cg > granules) cg = granules;
  const int64_t C = cg * 64;
  if (C > 0x7fffffffLL) return -1;
  geo2[0] = (int)((granules + cg - 1) / cg);
  geo2[1] = (int)C;
  return 0;
}

// qkv [B, 1, (H + 2 Hkv) 64] with Q rotated (row stride q_sb elements), caches [B, Hkv, capacity, 64], lens
// int32 [B] (the count before this token: lens[b] + 1 keys are read). S > 1: writes o_part [B, H, S, 64] and
// ml_part [B, H, S, 2] for pdt_attn_decode_combine; S == 1: writes out [B, H 64] (and lse [B, H] unless null).
// (S, C) must be what pdt_attn_decode_geo returns for this capacity.
int pdt_attn_decode(const uint16_t* qkv, int64_t q_sb, const uint16_t* k_cache, const uint16_t* v_cache,
                    const int* lens, float* o_part, float* ml_part, uint16_t* out, float* lse, int B, int H, int Hkv,
                    int capacity, int S, int C, float scale, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || capacity <= 0) return -1;
  if (S <= 0 || C <= 0 || C % 64 != 0 || (int64_t)S * C < capacity || (int64_t)(S - 1) * C >= capacity) return -2;
  if ((int64_t)capacity * ROW_BYTES > 0x7fffffffLL || Hkv > 65535 || B > 65535) return -3;
  if (S > 1 && (!o_part || !ml_part)) return -4;
  hipLaunchKernelGGL(attn_decode_kernel, dim3(S, Hkv, B), dim3(256), 0, s, qkv, q_sb, k_cache, v_cache, lens, o_part,
                     ml_part, out, lse, H, Hkv, capacity, C, scale * LOG2E);
  return 0;
}

int pdt_attn_decode_combine(const float* o_part, const float* ml_part, uint16_t* out, float* lse, int B, int H, int S,
                            hipStream_t s) {
  if (B <= 0 || H <= 0 || S <= 0) return -1;
  const int64_t rows = (int64_t)B * H;
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, o_part, ml_part,
                     out, lse, rows, S);
  return 0;
}

}  // extern "C"
