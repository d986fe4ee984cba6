// Paged KV-cache decoding for gfx950, head dim 64, bf16: the cache append and the split-KV decode attention of
// attn_decode.hip with the K/V rows in fixed-size pages of a shared pool, found through a block table.
//
// Layout. PAGE = 64 keys. Per layer two pools, k_pool and v_pool [n_pages, Hkv, 64, 64] bf16, contiguous: a
// (page, head) pair is one 8 KB slab, a key row still one 128-byte line, K stored after rotation. One
// block_table int32 [B, max_pages] on the device serves all layers: entry j of row b is the page that holds
// positions [64 j, 64 j + 64) of slot b, or -1. lens int32 [B] on the device as in attn_decode.hip. Nothing is
// read on the host and the grid depends on (B, Hkv, max_pages) only, so a captured step replays whatever the
// table and lens hold by then.
//
// pdt_rope_kv_append_paged: rope_kv_append_kernel with the destination row looked up. Row (b, t) sits at
// p = lens[b] + t, in page table[b, p >> 6] at row p & 63. Q and K are rotated in place in qkv through
// rope_math.h (the contiguous kernel's bits, so a prefill runs the causal flash forward on qkv as it stands).
// A row with p outside [0, min(64 max_pages, Tmax)) does nothing, as in the contiguous kernel; a row whose page
// id is outside [0, n_pages) is rotated in qkv and writes nothing to the pools.
//
// pdt_attn_decode_paged: one query token per slot, n[b] = clamp(lens[b] + 1, 0, 64 max_pages) keys. Grid
// (S, Hkv, B) with (S, C) from pdt_attn_decode_geo(B, Hkv, 64 max_pages, splits, G): C % 64 == 0, so a chunk is
// a whole number of pages. The key loop is attn_decode_kernel's, expression for expression: swapped K Q^T with
// the G heads of the group as MFMA columns, K straight from global memory to the v_mfma_f32_16x16x32_bf16
// operand registers, V through the wave-private swizzled LDS tile and ds_read_b64_tr_b16, U = 2 subtiles per
// step, all of a step's loads issued before their first use, no workgroup barrier in the loop, the four waves
// merged in wave order, fp32 partials for pdt_attn_decode_combine or a direct store when S == 1, further
// passes for G > 16. What paging changes:
//   * a workgroup's 64-key step is exactly one page, and wave w takes rows 16 w .. 16 w + 15 of it: no
//     fragment straddles a page, and a lane's byte offset into the page never changes (it is loop invariant);
//   * the chunk's page ids are loaded by one coalesced load, lane i holding table[b, c0 / 64 + i], and again
//     every 64 pages where C > 4096. (A departure from "once per pass, ahead of the key loop": the first 64 are
//     loaded once per workgroup, at the kernel's top beside lens[b], and serve every pass. They do not depend on
//     lens, and behind it the load's latency adds to every workgroup's: profiles/r23/paged_attention.txt.);
//   * a step takes its page id with a wave-uniform readlane, so the chain table -> address -> K is off the
//     loop's critical path and the resource words stay in SGPRs;
//   * one buffer resource per (page, step): base pool + (page Hkv + hk) 8192 bytes as a 64-bit address (the
//     pool may exceed 4 GB), num_records = clamp(n - first_key_of_page, 0, 64) 128. A row at or past n[b]
//     therefore reads as zero in hardware, as under the contiguous kernel's one resource of n rows: stale page
//     contents, NaN included, never reach an MFMA (the scores of those keys are still set to -inf). A page id
//     outside [0, n_pages) gets num_records = 0 over the pool's base: a bad table costs a wrong answer, never
//     an out-of-range access;
//   * a chunk that starts at or past n[b] runs no step and writes the empty partial (m = -inf, l = 0).
#include "../common.h"
#include "../launchers.h"
#include "../rope_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int D = 64;
constexpr int PAGE = 64;
constexpr int ROW_BYTES = D * 2;
constexpr int64_t SLAB = (int64_t)PAGE * D;  // elements of one (page, head) slab
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int U = 2;                       // pages per workgroup step, one 16-key subtile of each per wave
constexpr int SUB_BYTES = 16 * ROW_BYTES;  // one subtile of V in LDS
constexpr int MAX_PAGES = 1 << 23;         // per slot: key indices, a chunk's overhang included, stay below 2^31

// ---------------------------------------------------------------- cache append
__global__ __launch_bounds__(256) void rope_kv_append_paged_kernel(
    uint16_t* __restrict__ qkv, const float* __restrict__ cs, const float* __restrict__ sn,
    uint16_t* __restrict__ kp, uint16_t* __restrict__ vp, const int* __restrict__ table,
    const int* __restrict__ lens, int64_t items, int Tn, int H, int Hkv, int n_pages, int max_pages, int Tmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int AH = H + 2 * Hkv, per_tok = 4 * AH;  // 4 lanes per head, as in rope.hip
  const int64_t tok = i / per_tok;
  const int r = (int)(i - tok * per_tok);
  const int head = r >> 2, q = r & 3;
  const int b = (int)(tok / Tn), t = (int)(tok - (int64_t)b * Tn);
  const int64_t p = (int64_t)lens[b] + t;
  if (p < 0 || p >= (int64_t)max_pages * PAGE || p >= Tmax) return;  // as the contiguous kernel: nothing at all
  const int page = table[(int64_t)b * max_pages + (int)(p >> 6)];
  const bool store = page >= 0 && page < n_pages;  // a slot without that page keeps its rotation and stores nothing
  const int64_t row = (int64_t)page * Hkv * SLAB + (p & 63) * D + q * 8;  // + kv head * SLAB
  uint16_t* src = qkv + tok * (int64_t)D * AH + head * D + q * 8;
  if (head >= H + Hkv) {  // V: copied, not rotated
    if (!store) return;
    uint16_t* dst = vp + row + (head - H - Hkv) * SLAB;
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
  if (head >= H && store) {
    uint16_t* dst = kp + row + (head - H) * SLAB;
    st8_bf16(dst, olo);
    st8_bf16(dst + 32, ohi);
  }
}

// ---------------------------------------------------------------- decode attention
// The device helpers of attn_decode.hip, repeated here so that file's bits stay what its tests pin.
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

__device__ __forceinline__ float merge_weight(float ms, float m) {
  return ms == -INFINITY ? 0.f : (ms == m ? 1.f : fast_exp2(ms - m));
}

__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bf16x8 load8(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}

// The resource over the valid rows of one (page, head) slab: `rows` of them (0: every load returns zero).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t page_rsrc(const uint16_t* pool, int64_t slab, int rows) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(pool + slab * SLAB), (short)0, rows * ROW_BYTES,
                                           0x00020000);
}

__global__ __launch_bounds__(256) void attn_decode_paged_kernel(
    const uint16_t* __restrict__ qkv, int64_t q_sb, const uint16_t* __restrict__ kp, const uint16_t* __restrict__ vp,
    const int* __restrict__ table, const int* __restrict__ lens, float* __restrict__ o_part,
    float* __restrict__ ml_part, uint16_t* __restrict__ out, float* __restrict__ lse, int H, int Hkv, int n_pages,
    int max_pages, int C, float sl2) {
  __shared__ __attribute__((aligned(16))) char vs[4][U * SUB_BYTES];
  __shared__ __attribute__((aligned(16))) float mo[4][16][D];
  __shared__ float mm[4][16], ml[4][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = gridDim.x, sp = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = H / Hkv;
  const int c0 = sp * C;
  const int pg0 = c0 >> 6;  // the chunk's first table entry
  const int* trow = table + (int64_t)b * max_pages;
  // The chunk's first 64 page ids, one per lane (an entry past the table's row reads as no page). They do not
  // depend on lens, so the load is issued here, beside the load of lens, not behind it.
  const int pgs0 = pg0 + lane < max_pages ? trow[pg0 + lane] : -1;
  const int n = min(max(lens[b] + 1, 0), max_pages * PAGE);  // keys of this slot, clamped to its table
  const int cend = min(c0 + C, n);
  const int nit = cend > c0 ? (cend - c0 + 63) >> 6 : 0;  // pages of the chunk that hold a valid key
  // a lane's bytes within any page: K row 16 w + c, elements 32 s + 8 g ..; V rows 16 w + (id >> 3)
  const uint32_t koff = (uint32_t)((16 * w + c) * ROW_BYTES + 8 * g * 2);
  const uint32_t voff = (uint32_t)((16 * w + (lane >> 3)) * ROW_BYTES + (lane & 7) * 16);
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

    for (int blk = 0; blk < nit; blk += 64) {
      // the next 64 page ids of the chunk: loaded again only where C > 4096
      const int pgs = blk == 0 ? pgs0 : (pg0 + blk + lane < max_pages ? trow[pg0 + blk + lane] : -1);
      const int itend = min(nit, blk + 64);
      for (int it = blk; it < itend; it += U) {
        // ---- the step's two pages: a resource each for K and V over the page's valid rows
        __amdgpu_buffer_rsrc_t krs[U], vrs[U];
        int key0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // it - blk is even and at most 62, so the lane index is within 0 .. 63; an id taken for a page past
          // nit (u = 1 on an odd last step) is whatever that lane holds and is neutralised by ok
          const int page = __builtin_amdgcn_readlane(pgs, (it + u - blk) & 63);
          const int first = c0 + 64 * (it + u);
          const bool ok = it + u < nit && page >= 0 && page < n_pages;
          // first < cend <= n when it + u < nit, so this is clamp(n - first, 0, 64); kept to scalar min / select
          // (a three-way clamp is selected as a vector med3 and drags the resource into VGPRs and a waterfall loop)
          const int rows = __builtin_amdgcn_readfirstlane(ok ? min(n - first, PAGE) : 0);
          const int64_t slab = ok ? (int64_t)page * Hkv + hk : 0;
          krs[u] = page_rsrc(kp, slab, rows);
          vrs[u] = page_rsrc(vp, slab, rows);
          key0[u] = first + 16 * w;  // >= cend when it + u >= nit: fully masked below
        }
        // ---- all loads of the step first: K fragments, then V rows for the LDS tile
        bf16x8 ka[U][2], vr[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int s = 0; s < 2; ++s) ka[u][s] = load8(krs[u], koff + (uint32_t)(32 * s * 2));
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int j = 0; j < 2; ++j) vr[u][j] = load8(vrs[u], voff + (uint32_t)(8 * j * ROW_BYTES));
        wave_lds_order();  // the tile is wave-private: see attn_decode_kernel
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

}  // namespace

extern "C" {

// Append the Tn new rows of qkv [B, Tn, (H + 2 Hkv) 64] at positions lens[b] + t of the pools
// [n_pages, Hkv, 64, 64] through block_table int32 [B, max_pages]; Q and K are rotated in place. cos, sin:
// fp32 [Tmax, 32]. Everything contiguous and 16-byte aligned.
int pdt_rope_kv_append_paged(uint16_t* qkv, const float* cos, const float* sin, uint16_t* k_pool, uint16_t* v_pool,
                             const int* block_table, const int* lens, int B, int Tn, int H, int Hkv, int n_pages,
                             int max_pages, int Tmax, hipStream_t s) {
  if (B < 0 || Tn < 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || Tmax <= 0) return -1;
  if (n_pages <= 0 || max_pages <= 0 || max_pages > MAX_PAGES) return -1;
  const int64_t items = (int64_t)B * Tn * 4 * (H + 2 * Hkv);
  if (items == 0) return 0;
  const int64_t grid = (items + 255) / 256;
  if (grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(rope_kv_append_paged_kernel, dim3((unsigned)grid), dim3(256), 0, s, qkv, cos, sin, k_pool,
                     v_pool, block_table, lens, items, Tn, H, Hkv, n_pages, max_pages, Tmax);
  return 0;
}

// qkv [B, 1, (H + 2 Hkv) 64] with Q rotated (row stride q_sb elements), pools [n_pages, Hkv, 64, 64],
// block_table int32 [B, max_pages], lens int32 [B] (the count before this token: lens[b] + 1 keys are read).
// S > 1: writes o_part [B, H, S, 64] and ml_part [B, H, S, 2] for pdt_attn_decode_combine; S == 1: writes out
// [B, H 64] (and lse [B, H] unless null). (S, C) must be what pdt_attn_decode_geo returns for a capacity of
// 64 max_pages.
int pdt_attn_decode_paged(const uint16_t* qkv, int64_t q_sb, const uint16_t* k_pool, const uint16_t* v_pool,
                          const int* block_table, const int* lens, float* o_part, float* ml_part, uint16_t* out,
                          float* lse, int B, int H, int Hkv, int n_pages, int max_pages, int S, int C, float scale,
                          hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0) return -1;
  if (n_pages <= 0 || max_pages <= 0) return -1;
  const int64_t capacity = (int64_t)max_pages * PAGE;
  if (S <= 0 || C <= 0 || C % 64 != 0 || (int64_t)S * C < capacity || (int64_t)(S - 1) * C >= capacity) return -2;
  if (Hkv > 65535 || B > 65535 || max_pages > MAX_PAGES) return -3;
  if (S > 1 && (!o_part || !ml_part)) return -4;
  hipLaunchKernelGGL(attn_decode_paged_kernel, dim3(S, Hkv, B), dim3(256), 0, s, qkv, q_sb, k_pool, v_pool,
                     block_table, lens, o_part, ml_part, out, lse, H, Hkv, n_pages, max_pages, C, scale * LOG2E);
  return 0;
}

}  // extern "C"
