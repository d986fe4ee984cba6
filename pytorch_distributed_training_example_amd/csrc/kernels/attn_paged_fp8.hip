// The paged KV cache in OCP e4m3 for gfx950, head dim 64: the quantising cache append and the split-KV decode
// attention of attn_paged.hip on one-byte rows with one fp32 scale per stored (position, K/V head) row.
//
// Layout. PAGE = 64 keys. Per layer two byte pools, k_pool and v_pool [n_pages, Hkv, 64, 64] e4m3fn, contiguous: a
// (page, head) slab is 4 KB and a key row one 64-byte line; and two scale pools k_scale, v_scale [n_pages, Hkv, 64]
// fp32, 256 bytes per slab. block_table, lens and everything the host knows are attn_paged.hip's. A stored row is
// quantize_rows_e4m3's of the 64-element row the bf16 cache would hold (K: the rotated row after its bf16
// rounding): amax = max |x|, scale = amax / 448 (1 for a zero row), q = e4m3_rne(clamp(x (448 / amax), +-448)),
// through fp8_pack.h's e4m3_row_scale / e4m3_row_inv / pack4_fp8, the functions quant_rows_e4m3_kernel uses.
// Attention on such a cache is attention on K^ = float(kq) k_scale[row], V^ = float(vq) v_scale[row].
//
// pdt_rope_kv_append_paged_fp8: rope_kv_append_paged_kernel with a quantising store. The four lanes that own a
// head's row (16 elements each: 8 q .. 8 q + 7 and 32 + 8 q ..) are a DPP quad: the row's amax is two quad_perm
// steps, no LDS. Each lane converts its two 8-element runs and writes two 8-byte stores, lane 0 of the quad
// the scale. Q and K are rotated in place in the bf16 qkv with rope_math.h's bits, so a prefill's causal flash
// forward runs on qkv as it stands. Rows out of range behave as in the bf16 kernel.
//
// pdt_attn_decode_paged_fp8: attn_decode_paged_kernel's work split, kept: grid (S, Hkv, B), (S, C) of
// pdt_attn_decode_geo at 64 max_pages, one page per 64-key step and U = 2 pages per loop turn, wave w on rows
// 16 w .. 16 w + 15, the G heads of a group as MFMA columns (further passes for G > 16), the page ids loaded at the
// kernel's top and taken per step by a wave-uniform readlane, the four-wave merge in wave order, the combine
// kernel for S > 1, no atomics and no workgroup barrier in the key loop. How one-byte rows reach the matrix cores
// is this file's own:
//   K   global -> registers -> MFMA, no LDS. A key row is 64 bytes, so lane (c, g) = (lane & 15, lane >> 4) takes
//       row c's bytes [16 g, 16 g + 16) with ONE 16-byte buffer load per subtile (the bf16 kernel needs two), and
//       the subtile's two v_mfma_f32_16x16x32_bf16 contract over k = 16 g + 0..7 and 16 g + 8..15. Q is loaded with
//       the same assignment (head c, elements 16 g + 8 s ..): a dot product does not care where its terms sit as
//       long as A and B agree. e4m3 -> bf16 (v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32, exact) happens in registers
//       right before the MFMA.
//   V   one 16-byte load per lane and subtile as well: row lane >> 2 of the wave's 16, bytes [16 (lane & 3), + 16).
//       Converted to bf16 BEFORE the store into the wave-private swizzled LDS tile (two 16-byte writes, chunks
//       2 (lane & 3) and 2 (lane & 3) + 1 of the row), so the tile, ds_read_b64_tr_b16 and the 16x16x16 PV MFMA
//       are the bf16 kernel's. The alternative, e4m3 in LDS read back through ds_read_b64_tr_b8, was weighed on the
//       ISA and not built: the b8 transpose hands a lane 8 consecutive k of one column, the operand shape of the
//       K = 32 MFMAs, where the PV product here contracts over the 16 keys of a subtile, 4 per lane, in the layout
//       the score MFMA leaves P in. Taking it means a 32-key PV step, P exchanged between lanes through LDS and
//       an MFMA half of whose k is another subtile's: it halves 8 KB of LDS traffic per step that is not the
//       loop's limit (the loop waits on global memory) and puts a cross-lane exchange on the critical path. It
//       was not timed.
//   scales never touch the elements. st[r] = (sum q float(kq)) k_scale[key r], one fp32 multiply per score before
//       sl2 and the maximum; P enters the PV MFMA as bf16(p v_scale[key r]); the row sum l adds the unscaled p.
//       A lane's four score rows are keys 4 g .. 4 g + 3 of the subtile: their scales are one 16-byte load per
//       pool and subtile.
//   pipeline. The loads of step i + 1 (per lane 2 x (K 16 B, V 16 B, two scale quads)) are issued before step i's
//       bytes are converted: two register sets, the loop unrolled by two so that neither is copied.
//   resources per (page, step), in SGPRs: the data pools with num_records = clamp(n - first_key_of_page, 0, 64) 64,
//       the scale pools with clamp(...) 4 (range-checked per dword), so a stale row, NaN bytes included, and its
//       stale scale both read as zero; a page id outside [0, n_pages) gets zero records over the pool's base. The
//       scores of keys at or past n[b] are set to -inf and their PV weights to zero besides.
// Compiled like attn_paged.hip (packed fp32 left on). Registers, LDS and occupancy: profiles/r25/paged_fp8.txt.
#include "../common.h"
#include "../fp8_pack.h"
#include "../launchers.h"
#include "../rope_math.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int D = 64;
constexpr int PAGE = 64;
constexpr int ROW_BYTES = D;                 // a stored row: 64 e4m3 bytes
constexpr int64_t SLAB = (int64_t)PAGE * D;  // bytes of one (page, head) slab; its scales are PAGE floats
constexpr int LROW = D * 2;                  // a row of the LDS tile: bf16
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int U = 2;                  // pages per workgroup step, one 16-key subtile of each per wave
constexpr int SUB_BYTES = 16 * LROW;  // one subtile of V in LDS
constexpr int MAX_PAGES = 1 << 23;    // per slot: key indices, a chunk's overhang included, stay below 2^31

// ---------------------------------------------------------------- cache append
// max over the four lanes of a quad: quad_perm [1, 0, 3, 2], then [2, 3, 0, 1]
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
  return v;
}

// The lane's 16 elements of a row (lo: 8 q .., hi: 32 + 8 q ..) -> bytes and, from lane q == 0, the row's scale.
// All four lanes of the quad call it together.
__device__ __forceinline__ void store_row_e4m3(const float (&lo)[8], const float (&hi)[8], uint8_t* dst, float* sc,
                                               int q) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fmaxf(fabsf(lo[j]), fabsf(hi[j])));
  amax = quad_max(amax);
  const float inv = e4m3_row_inv(amax);
  uint2 a, b;
  a.x = pack4_fp8(lo[0] * inv, lo[1] * inv, lo[2] * inv, lo[3] * inv);
  a.y = pack4_fp8(lo[4] * inv, lo[5] * inv, lo[6] * inv, lo[7] * inv);
  b.x = pack4_fp8(hi[0] * inv, hi[1] * inv, hi[2] * inv, hi[3] * inv);
  b.y = pack4_fp8(hi[4] * inv, hi[5] * inv, hi[6] * inv, hi[7] * inv);
  *reinterpret_cast<uint2*>(dst) = a;
  *reinterpret_cast<uint2*>(dst + 32) = b;
  if (q == 0) *sc = e4m3_row_scale(amax);
}

__global__ __launch_bounds__(256) void rope_kv_append_paged_fp8_kernel(
    uint16_t* __restrict__ qkv, const float* __restrict__ cs, const float* __restrict__ sn, uint8_t* __restrict__ kp,
    uint8_t* __restrict__ vp, float* __restrict__ ksc, float* __restrict__ vsc, const int* __restrict__ table,
    const int* __restrict__ lens, int64_t items, int Tn, int H, int Hkv, int n_pages, int max_pages, int Tmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;  // items % 4 == 0 and every condition below is the quad's: a quad leaves or stays as one
  const int AH = H + 2 * Hkv, per_tok = 4 * AH;  // 4 lanes per head, as in rope.hip
  const int64_t tok = i / per_tok;
  const int r = (int)(i - tok * per_tok);
  const int head = r >> 2, q = r & 3;
  const int b = (int)(tok / Tn), t = (int)(tok - (int64_t)b * Tn);
  const int64_t p = (int64_t)lens[b] + t;
  if (p < 0 || p >= (int64_t)max_pages * PAGE || p >= Tmax) return;  // as the bf16 kernel: nothing at all
  const int page = table[(int64_t)b * max_pages + (int)(p >> 6)];
  const bool store = page >= 0 && page < n_pages;  // a slot without that page keeps its rotation and stores nothing
  const int64_t slab = (int64_t)page * Hkv;        // + kv head
  const int prow = (int)(p & 63);
  uint16_t* src = qkv + tok * (int64_t)D * AH + head * D + q * 8;
  float lo[8], hi[8];
  ld8_bf16(src, lo);
  ld8_bf16(src + 32, hi);
  if (head >= H + Hkv) {  // V: quantised as it stands, not rotated
    if (!store) return;
    const int64_t sl = slab + (head - H - Hkv);
    store_row_e4m3(lo, hi, vp + sl * SLAB + prow * ROW_BYTES + q * 8, vsc + sl * PAGE + prow, q);
    return;
  }
  float olo[8], ohi[8];
  rope_rotate8(lo, hi, cs + p * 32 + q * 8, sn + p * 32 + q * 8, 1.f, olo, ohi);
  st8_bf16(src, olo);  // in place, K included: a prefill's causal forward reads the rotated K from qkv
  st8_bf16(src + 32, ohi);
  if (head >= H && store) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the row the bf16 cache would hold
      olo[j] = bf2f(f2bf(olo[j]));
      ohi[j] = bf2f(f2bf(ohi[j]));
    }
    const int64_t sl = slab + (head - H);
    store_row_e4m3(olo, ohi, kp + sl * SLAB + prow * ROW_BYTES + q * 8, ksc + sl * PAGE + prow, q);
  }
}

// ---------------------------------------------------------------- decode attention
// The device helpers of attn_paged.hip, repeated here so that file's bits stay what its tests pin.
__device__ __forceinline__ int swz(int row, int chunk) { return row * LROW + ((chunk ^ ((row >> 1) & 7)) << 4); }

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

__device__ __forceinline__ u4 load16(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
}

// 8 e4m3 bytes (two words) -> 8 bf16, exactly, in byte order (gemm_skinny_w8.hip's)
__device__ __forceinline__ bf16x8 cvt8(uint32_t lo, uint32_t hi) {
  const bf16x2 a = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), bf16x2);
  const bf16x2 b = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true), bf16x2);
  const bf16x2 c = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), bf16x2);
  const bf16x2 d = __builtin_convertvector(__builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true), bf16x2);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// The resource over the first `bytes` bytes of slab `slab` of a pool of `unit`-byte slabs (0: every load is zero).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(const void* pool, int64_t slab, int unit, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(pool)) + slab * unit, (short)0,
                                           bytes, 0x00020000);
}

// One step's bytes as they arrive: per page u the lane's 16 bytes of a K row and of a V row and the scales of its
// four score rows; key0[u] is the first key of the wave's subtile.
struct StepRegs {
  u4 k[U], v[U];
  f4 ks[U], vs[U];
  int key0[U];
};

__global__ __launch_bounds__(256, 3) void attn_decode_paged_fp8_kernel(
    const uint16_t* __restrict__ qkv, int64_t q_sb, const uint8_t* __restrict__ kp, const uint8_t* __restrict__ vp,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int* __restrict__ table,
    const int* __restrict__ lens, float* __restrict__ o_part, float* __restrict__ ml_part, uint16_t* __restrict__ out,
    float* __restrict__ lse, int H, int Hkv, int n_pages, int max_pages, int C, float sl2) {
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
  // The chunk's first 64 page ids, one per lane (an entry past the table's row reads as no page), issued beside
  // the load of lens, not behind it.
  const int pgs0 = pg0 + lane < max_pages ? trow[pg0 + lane] : -1;
  const int n = min(max(lens[b] + 1, 0), max_pages * PAGE);  // keys of this slot, clamped to its table
  const int cend = min(c0 + C, n);
  const int nit = cend > c0 ? (cend - c0 + 63) >> 6 : 0;  // pages of the chunk that hold a valid key
  // a lane's bytes within any page: K row 16 w + c, bytes 16 g ..; V row 16 w + (lane >> 2), bytes 16 (lane & 3) ..;
  // the scales of keys 16 w + 4 g .. + 3
  const uint32_t koff = (uint32_t)((16 * w + c) * ROW_BYTES + 16 * g);
  const uint32_t voff = (uint32_t)((16 * w + (lane >> 2)) * ROW_BYTES + 16 * (lane & 3));
  const uint32_t soff = (uint32_t)((16 * w + 4 * g) * 4);
  char* vw = vs[w];
  const int vl0 = swz(lane >> 2, 2 * (lane & 3)), vl1 = swz(lane >> 2, 2 * (lane & 3) + 1);

  for (int pass0 = 0; pass0 < G; pass0 += 16) {
    // Q^T as the B operand: lane (c, g) holds head pass0 + c, elements 16 g + 8 s .. + 8 (K's assignment)
    const int hq = pass0 + c;
    bf16x8 bq[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (hq < G) {
        bq[s] = *reinterpret_cast<const bf16x8*>(qkv + (int64_t)b * q_sb + (int64_t)(hk * G + hq) * D + 16 * g + 8 * s);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) bq[s][j] = (__bf16)0.f;
      }
    }
    f4 oacc[4];
#pragma unroll
    for (int nn = 0; nn < 4; ++nn) oacc[nn] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    int pgs = pgs0;

    // ---- issue every load of step `it` (pages it, it + 1 of the chunk); called with it = 0, U, 2 U, ... in order
    auto issue = [&](int it, StepRegs& x) {
      if ((it & 63) == 0 && it > 0)  // the next 64 page ids of the chunk: only where C > 4096
        pgs = pg0 + it + lane < max_pages ? trow[pg0 + it + lane] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // it is even, so the lane index is within 0 .. 63; an id taken for a page past nit (u = 1 on an odd last
        // step) is whatever that lane holds and is neutralised by ok
        const int page = __builtin_amdgcn_readlane(pgs, (it + u) & 63);
        const int first = c0 + 64 * (it + u);
        const bool ok = it + u < nit && page >= 0 && page < n_pages;
        // first < cend <= n when it + u < nit, so this is clamp(n - first, 0, 64); scalar min / select as in the
        // bf16 kernel (a vector med3 would drag the resources into VGPRs and a waterfall loop)
        const int rows = __builtin_amdgcn_readfirstlane(ok ? min(n - first, PAGE) : 0);
        const int64_t slab = ok ? (int64_t)page * Hkv + hk : 0;
        x.k[u] = load16(slab_rsrc(kp, slab, (int)SLAB, rows * ROW_BYTES), koff);
        x.ks[u] = __builtin_bit_cast(f4, load16(slab_rsrc(ksc, slab, PAGE * 4, rows * 4), soff));
        x.v[u] = load16(slab_rsrc(vp, slab, (int)SLAB, rows * ROW_BYTES), voff);
        x.vs[u] = __builtin_bit_cast(f4, load16(slab_rsrc(vsc, slab, PAGE * 4, rows * 4), soff));
        x.key0[u] = first + 16 * w;  // >= cend when it + u >= nit: fully masked below
      }
    };
    // ---- one step on bytes that have arrived
    auto compute = [&](const StepRegs& x) {
      wave_lds_order();  // the tile is wave-private: see attn_decode_kernel
#pragma unroll
      for (int u = 0; u < U; ++u) {
        *reinterpret_cast<bf16x8*>(vw + u * SUB_BYTES + vl0) = cvt8(x.v[u][0], x.v[u][1]);
        *reinterpret_cast<bf16x8*>(vw + u * SUB_BYTES + vl1) = cvt8(x.v[u][2], x.v[u][3]);
      }
      wave_lds_order();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        f4 st = {0.f, 0.f, 0.f, 0.f};
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(x.k[u][0], x.k[u][1]), bq[0], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(x.k[u][2], x.k[u][3]), bq[1], st, 0, 0, 0);
        float mt = -INFINITY;
        bool dead[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dead[r] = x.key0[u] + 4 * g + r >= cend;
          st[r] = dead[r] ? -INFINITY : st[r] * x.ks[u][r];
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
          pb[r] = __builtin_bit_cast(short, (__bf16)(dead[r] ? 0.f : p * x.vs[u][r]));
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
    };

    StepRegs ra, rb;
    if (nit > 0) issue(0, ra);
    for (int it = 0; it < nit; it += 2 * U) {
      const bool more = it + U < nit;
      if (more) issue(it + U, rb);
      compute(ra);
      if (more) {
        if (it + 2 * U < nit) issue(it + 2 * U, ra);
        compute(rb);
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

// pdt_rope_kv_append_paged with a quantising store: pools [n_pages, Hkv, 64, 64] e4m3, scale pools
// [n_pages, Hkv, 64] fp32. Everything contiguous and 16-byte aligned.
int pdt_rope_kv_append_paged_fp8(uint16_t* qkv, const float* cos, const float* sin, uint8_t* k_pool, uint8_t* v_pool,
                                 float* k_scale, float* v_scale, const int* block_table, const int* lens, int B, int Tn,
                                 int H, int Hkv, int n_pages, int max_pages, int Tmax, hipStream_t s) {
  if (B < 0 || Tn < 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || Tmax <= 0) return -1;
  if (n_pages <= 0 || max_pages <= 0 || max_pages > MAX_PAGES) return -1;
  const int64_t items = (int64_t)B * Tn * 4 * (H + 2 * Hkv);
  if (items == 0) return 0;
  const int64_t grid = (items + 255) / 256;
  if (grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(rope_kv_append_paged_fp8_kernel, dim3((unsigned)grid), dim3(256), 0, s, qkv, cos, sin, k_pool,
                     v_pool, k_scale, v_scale, block_table, lens, items, Tn, H, Hkv, n_pages, max_pages, Tmax);
  return 0;
}

// pdt_attn_decode_paged on e4m3 pools and their fp32 scale pools; every other argument and the outputs as there.
int pdt_attn_decode_paged_fp8(const uint16_t* qkv, int64_t q_sb, const uint8_t* k_pool, const uint8_t* v_pool,
                              const float* k_scale, const float* v_scale, const int* block_table, const int* lens,
                              float* o_part, float* ml_part, uint16_t* out, float* lse, int B, int H, int Hkv,
                              int n_pages, int max_pages, int S, int C, float scale, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0) return -1;
  if (n_pages <= 0 || max_pages <= 0) return -1;
  const int64_t capacity = (int64_t)max_pages * PAGE;
  if (S <= 0 || C <= 0 || C % 64 != 0 || (int64_t)S * C < capacity || (int64_t)(S - 1) * C >= capacity) return -2;
  if (Hkv > 65535 || B > 65535 || max_pages > MAX_PAGES) return -3;
  if (S > 1 && (!o_part || !ml_part)) return -4;
  hipLaunchKernelGGL(attn_decode_paged_fp8_kernel, dim3(S, Hkv, B), dim3(256), 0, s, qkv, q_sb, k_pool, v_pool, k_scale,
                     v_scale, block_table, lens, o_part, ml_part, out, lse, H, Hkv, n_pages, max_pages, C,
                     scale * LOG2E);
  return 0;
}

}  // extern "C"
