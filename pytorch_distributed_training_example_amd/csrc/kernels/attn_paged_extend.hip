// Multi-token append attention on the paged KV cache for gfx950, head dim 64, bf16: pdt_attn_extend of
// attn_decode.hip with the K/V rows read through the block table of attn_paged.hip.
//
// pdt_attn_extend_paged: Tn >= 1 new tokens per slot b, already appended (pdt_rope_kv_append_paged) at positions
// lens[b] + t of the pools [n_pages, Hkv, 64, 64], found through block_table int32 [B, max_pages]. Query (b, t, h)
// sees keys 0 .. n(b, t) - 1 of K/V head h / G, n(b, t) = clamp(lens[b] + t + 1, 0, 64 max_pages).
//
// Work split: attn_extend_kernel<NT>'s. The MFMA columns are (token, head) pairs, q = t G + hq < R = G Tn,
// token-major; a workgroup owns 16 NT columns (NT in 1, 2, 4) and C keys of one (b, hk); grid (S, Hkv NB, B) with
// (S, C, NB, NT) from pdt_attn_extend_geo for a capacity of 64 max_pages. C % 64 == 0: a chunk is whole pages.
//
// Data movement: attn_decode_paged_kernel's. A workgroup's 64-key step is one page, wave w takes its rows
// 16 w .. 16 w + 15, and a lane's byte offset inside a page is loop invariant. K goes straight from global memory
// to the v_mfma_f32_16x16x32_bf16 A operand, V through the wave-private swizzled LDS tile and ds_read_b64_tr_b16;
// both are fetched once per subtile and serve all NT tiles, each with its own Q registers, mask, (m, l) and
// accumulators. U = 2 pages per step, all of a step's loads before the first use, no workgroup barrier in the loop.
// The chunk's first 64 page ids come from one coalesced load at the kernel's top, beside lens[b] (again every 64
// pages where C > 4096); a step takes its id with a wave-uniform readlane.
//
// Where the two meet: one buffer resource per (page, step), in SGPRs. Base pool + (page Hkv + hk) 8192 bytes as a
// 64-bit address, num_records = clamp(n_blk - first_key_of_page, 0, 64) 128, with n_blk the key limit of the
// block's last valid column (the contiguous append kernel's), not the slot's. So
//   * rows at or past n_blk (stale page contents, NaN included) read as zero in hardware;
//   * a block of early tokens neither walks nor reads pages that only later tokens see;
//   * rows between a column's own limit and n_blk are the finite rows just appended: their scores are computed
//     and masked per column, p = 0 exactly, and a step a column sees nothing of leaves its state (alpha = 2^0);
//   * a page id outside [0, n_pages), and the page past the block's last one on an odd last step, get zero
//     records over the pool's base: a bad table costs a wrong answer, never an out-of-range access.
// The row count is formed with scalar min / select (a three-way clamp becomes a vector med3 and drags the
// resource into VGPRs, with a waterfall loop around every load).
//
// Arithmetic: compiled without the packed fp32 operations, with xor_lanes and block_barrier for the HIP header's
// functions, as attn_extend_kernel is: a column's arithmetic is that kernel's, expression for expression.
// The four waves are merged tile after tile through the one mo / mm / ml buffer. Partials o_part
// [B, Tn, H, S, 64] and ml_part [B, Tn, H, S, 2] for pdt_attn_decode_combine over B Tn rows; S == 1 stores the
// bf16 output and the LSE directly. No atomics, the same bits every run.
#include "../common.h"
#include "../launchers.h"

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

#if defined(__HIP_DEVICE_COMPILE__)
#define PDT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PDT_NO_PACKED_F32
#endif

// The device helpers of attn_decode.hip and attn_paged.hip, repeated here so those files' bits stay what their
// tests pin.
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

__device__ __forceinline__ float xor_lanes(float x, int mask, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, __builtin_bit_cast(int, x)));
}

__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The register budget is the contiguous twin's occupancy: 4, 3, 2 workgroups per CU at NT 1, 2, 4 (the page
// resources cost SGPRs, not VGPRs; without the hint NT = 2 lands one register past three waves).
template <int NT>
PDT_NO_PACKED_F32 __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(NT == 1 ? 4 : (NT == 2 ? 3 : 2)))) void attn_extend_paged_kernel(
    const uint16_t* __restrict__ qkv, int64_t q_sb, int64_t q_st, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const int* __restrict__ table, const int* __restrict__ lens,
    float* __restrict__ o_part, float* __restrict__ ml_part, uint16_t* __restrict__ out, float* __restrict__ lse,
    int Tn, int H, int Hkv, int NB, int n_pages, int max_pages, int C, float sl2) {
  __shared__ __attribute__((aligned(16))) char vs[4][U * SUB_BYTES];
  __shared__ __attribute__((aligned(16))) float mo[4][16][D];
  __shared__ float mm[4][16], ml[4][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = gridDim.x, sp = blockIdx.x, b = blockIdx.z;
  const int hk = blockIdx.y / NB, q0 = (blockIdx.y - hk * NB) * (16 * NT);
  const int G = H / Hkv, R = G * Tn;
  const int c0 = sp * C;
  const int pg0 = c0 >> 6;  // the chunk's first table entry
  const int* trow = table + (int64_t)b * max_pages;
  // The chunk's first 64 page ids, one per lane (an entry past the table's row reads as no page). They do not
  // depend on lens, so the load is issued here, beside the load of lens, not behind it.
  const int pgs0 = pg0 + lane < max_pages ? trow[pg0 + lane] : -1;
  const int64_t len = lens[b];
  const int64_t cap = (int64_t)max_pages * PAGE;
  // the block's last valid column bounds the pages that are walked and the rows that are read at all
  const int n_blk = (int)min(max(len + (min(q0 + 16 * NT, R) - 1) / G + 1, (int64_t)0), cap);
  const int cend_blk = min(c0 + C, n_blk);
  const int nit = cend_blk > c0 ? (cend_blk - c0 + 63) >> 6 : 0;  // pages of the chunk that hold a key of the block
  // a lane's bytes within any page: K row 16 w + c, elements 32 s + 8 g ..; V rows 16 w + (id >> 3)
  const uint32_t koff = (uint32_t)((16 * w + c) * ROW_BYTES + 8 * g * 2);
  const uint32_t voff = (uint32_t)((16 * w + (lane >> 3)) * ROW_BYTES + (lane & 7) * 16);
  char* vw = vs[w];

  // Q^T as the B operand, per tile: lane (c, g) holds column q0 + 16 j + c, elements 32 s + 8 g .. + 8, and
  // that column's key limit within the chunk (0 for a column past R: everything masked, nothing stored)
  bf16x8 bq[NT][2];
  int cend[NT];
  f4 oacc[NT][4];
  float m[NT], l[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int q = q0 + 16 * j + c;
    const int t = q / G, hq = q - t * G;
    cend[j] = q < R ? min(c0 + C, (int)min(max(len + t + 1, (int64_t)0), cap)) : 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (q < R) {
        bq[j][s] = *reinterpret_cast<const bf16x8*>(qkv + (int64_t)b * q_sb + (int64_t)t * q_st +
                                                    (int64_t)(hk * G + hq) * D + 32 * s + 8 * g);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) bq[j][s][e] = (__bf16)0.f;
      }
    }
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) oacc[j][nn] = f4{0.f, 0.f, 0.f, 0.f};
    m[j] = -INFINITY;
    l[j] = 0.f;
  }

  for (int blk = 0; blk < nit; blk += 64) {
    // the next 64 page ids of the chunk: loaded again only where C > 4096
    const int pgs = blk == 0 ? pgs0 : (pg0 + blk + lane < max_pages ? trow[pg0 + blk + lane] : -1);
    const int itend = min(nit, blk + 64);
    for (int it = blk; it < itend; it += U) {
      // ---- the step's two pages: a resource each for K and V over the rows of the page that the block reads
      __amdgpu_buffer_rsrc_t krs[U], vrs[U];
      int key0[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // it - blk is even and at most 62, so the lane index is within 0 .. 63; an id taken for a page past
        // nit (u = 1 on an odd last step) is whatever that lane holds and is neutralised by ok
        const int page = __builtin_amdgcn_readlane(pgs, (it + u - blk) & 63);
        const int first = c0 + 64 * (it + u);
        const bool ok = it + u < nit && page >= 0 && page < n_pages;
        // first < cend_blk <= n_blk when it + u < nit, so this is clamp(n_blk - first, 0, 64); kept to scalar
        // min / select (a three-way clamp is selected as a vector med3: see the file's head)
        const int rows = __builtin_amdgcn_readfirstlane(ok ? min(n_blk - first, PAGE) : 0);
        const int64_t slab = ok ? (int64_t)page * Hkv + hk : 0;
        krs[u] = page_rsrc(kp, slab, rows);
        vrs[u] = page_rsrc(vp, slab, rows);
        key0[u] = first + 16 * w;  // >= cend_blk when it + u >= nit: masked in every column
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
        for (int i = 0; i < 2; ++i) vr[u][i] = load8(vrs[u], voff + (uint32_t)(8 * i * ROW_BYTES));
      wave_lds_order();  // the tile is wave-private: see attn_decode_kernel
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int id = lane + 64 * i;
          *reinterpret_cast<bf16x8*>(vw + u * SUB_BYTES + swz(id >> 3, id & 7)) = vr[u][i];
        }
      wave_lds_order();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s4 va[4];  // V^T of the subtile, once for all NT tiles
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) va[nn] = lds_tr4(vw + u * SUB_BYTES, 4 * g, 16 * nn, lane);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          f4 st = {0.f, 0.f, 0.f, 0.f};
          st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[u][0], bq[j][0], st, 0, 0, 0);
          st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[u][1], bq[j][1], st, 0, 0, 0);
          float mt = -INFINITY;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (key0[u] + 4 * g + r >= cend[j]) st[r] = -INFINITY;
            mt = fmaxf(mt, st[r]);
          }
          mt = fmaxf(mt, xor_lanes(mt, 16, lane));
          mt = fmaxf(mt, xor_lanes(mt, 32, lane));
          const float mn = fmaxf(m[j], mt * sl2);
          const float alpha = (mn == -INFINITY) ? 1.f : fast_exp2(m[j] - mn);
          const float msub = (mn == -INFINITY) ? 0.f : mn;
          float ls = 0.f;
          s4 pb;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = fast_exp2(fmaf(st[r], sl2, -msub));
            ls += p;
            pb[r] = __builtin_bit_cast(short, (__bf16)p);
          }
          l[j] = l[j] * alpha + ls;
          m[j] = mn;
#pragma unroll
          for (int nn = 0; nn < 4; ++nn) {
            oacc[j][nn] *= alpha;
            oacc[j][nn] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(va[nn], pb, oacc[j][nn], 0, 0, 0);
          }
        }
      }
    }
  }
  // ---- merge the four waves in wave order, one tile at a time through the one buffer
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    float lj = l[j];
    lj += xor_lanes(lj, 16, lane);
    lj += xor_lanes(lj, 32, lane);
    if (g == 0) {
      mm[w][c] = m[j];
      ml[w][c] = lj;
    }
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) *reinterpret_cast<f4*>(&mo[w][c][16 * nn + 4 * g]) = oacc[j][nn];
    block_barrier();
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
      const int q = q0 + 16 * j + qh;
      if (q < R) {
        const int t = q / G, hq = q - t * G;
        const int64_t row = ((int64_t)b * Tn + t) * H + hk * G + hq;
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
    if (j + 1 < NT) block_barrier();  // mo / mm / ml are rewritten by the next tile
  }
}

}  // namespace

extern "C" {

// qkv [B, Tn, (H + 2 Hkv) 64] with Q rotated (batch stride q_sb, row stride q_st, in elements), pools
// [n_pages, Hkv, 64, 64] already holding the Tn tokens at lens[b] + t, block_table int32 [B, max_pages], lens
// int32 [B], the count before the append. S > 1: writes o_part [B, Tn, H, S, 64] and ml_part [B, Tn, H, S, 2]
// for pdt_attn_decode_combine (B Tn rows of heads); S == 1: writes out [B, Tn, H 64] (and lse [B, Tn, H] unless
// null). (S, C, NB, NT) must be what pdt_attn_extend_geo returns for a capacity of 64 max_pages.
int pdt_attn_extend_paged(const uint16_t* qkv, int64_t q_sb, int64_t q_st, const uint16_t* k_pool,
                          const uint16_t* v_pool, const int* block_table, const int* lens, float* o_part,
                          float* ml_part, uint16_t* out, float* lse, int B, int Tn, int H, int Hkv, int n_pages,
                          int max_pages, int S, int C, int NB, int NT, float scale, hipStream_t s) {
  if (B <= 0 || Tn < 1 || H <= 0 || Hkv <= 0 || H % Hkv != 0) return -1;
  if (n_pages <= 0 || max_pages <= 0) return -1;
  const int64_t capacity = (int64_t)max_pages * PAGE;
  if (S <= 0 || C <= 0 || C % 64 != 0 || (int64_t)S * C < capacity || (int64_t)(S - 1) * C >= capacity) return -2;
  const int64_t R = (int64_t)(H / Hkv) * Tn;
  if ((NT != 1 && NT != 2 && NT != 4) || NB != (R + 16 * NT - 1) / (16 * NT)) return -2;
  if (max_pages > MAX_PAGES || (int64_t)Hkv * NB > 65535 || B > 65535 || R > 0x7fffffffLL) return -3;
  if (S > 1 && (!o_part || !ml_part)) return -4;
  const dim3 grid(S, Hkv * NB, B);
  const float sl2 = scale * LOG2E;
#define PDT_EXTEND_PAGED(N)                                                                                        \
  hipLaunchKernelGGL(attn_extend_paged_kernel<N>, grid, dim3(256), 0, s, qkv, q_sb, q_st, k_pool, v_pool,          \
                     block_table, lens, o_part, ml_part, out, lse, Tn, H, Hkv, NB, n_pages, max_pages, C, sl2)
  if (NT == 1) PDT_EXTEND_PAGED(1);
  else if (NT == 2) PDT_EXTEND_PAGED(2);
  else PDT_EXTEND_PAGED(4);
#undef PDT_EXTEND_PAGED
  return 0;
}

}  // extern "C"
