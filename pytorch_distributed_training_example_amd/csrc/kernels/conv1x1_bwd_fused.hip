// Fused backward of a ResNet bottleneck's LAST 1x1 convolution and the BatchNorm that follows it
// (gfx950, NHWC bf16, fp32 accumulate). One pass over the incoming gradient produces everything:
//
//   dz[m, c]  = A[c] * dy[m, c] * relu_mask[m, c] + B[c] * (z[m, c] - mean[c]) + D[c]
//               (the BatchNorm's backward apply, bn3: never written to memory)
//   dxa[m, k] = sum_c dz[m, c] * W[c, k]            (data gradient of the conv, k < CW)
//   dW[c, k]  = sum_m dz[m, c] * xa[m, k]           (weight gradient of the conv)
//   part      = per-workgroup sum(g), sum(g * (xb - mean_b)) with g = dxa * relu_mask_b
//               (the backward reduction of the BatchNorm that produced xa, bn2 — optional)
//
// Not in the reference (LeNet has no BN or residual blocks, /root/reference/cnn.py:9-23). Unfused,
// the same work is four HBM passes: the BN backward apply (read dy, z, mask; write dz), the dgrad GEMM
// (read dz, write dxa; its epilogue re-reads xb for the bn2 reduction) and the wgrad GEMM (read dz and
// xa) — 22 "T" of traffic per layer-1 block (T = one 64-channel activation) against 10.3 T here.
//
// Structure (one persistent workgroup per CU, memory bound by design):
//   * a stage = KP pixels (32 at C4 = 256, 16 at C4 = 512). dy, z (C4-channel rows), the bn3 mask bits,
//     xa and xb (one 128-B row per 64-channel slice, XOR-swizzled by permuting each lane's DMA source
//     chunk) and the bn2 mask bits are staged by LDS-DMA (global_load_lds, 16 / 4 bytes per lane)
//     through a 3-slot ring, two stages in flight, counted vmcnt, raw s_barrier
//     (cdna_hip_programming.md §5 "Pipelining across barriers");
//   * a transform pass turns (dy, z, mask) into dz in a separate LDS tile whose rows are swizzled
//     with chunk ^ (((r & 3) << 2) | ((r >> 2) & 2)): conflict-free for BOTH readers, the dgrad's
//     ds_read_b128 (16 pixel rows, one 16-B chunk) and the wgrad's ds_read_b64_tr_b16 (4 rows x 64 B);
//   * a workgroup covers one 64-channel slice of CW ("role"; NR = CW / 64 roles per pixel group, placed
//     on one XCD: blocks b, b + 8, ... — the second role's reads of dy / z can hit L2; speed only).
//     At CW = 128 (layer 2) that pairing measured 904 us against a 434 us floor — the pairs drift
//     apart and both read HBM — but one workgroup for both slices does not fit: W^T (128 KB) and the
//     wgrad accumulators (256 KB) need 384 registers per lane at 4 waves, 8 waves spill at two per
//     SIMD, and neither fits LDS beside the ring. NG (slices per workgroup) stays 1;
//   * dgrad: v_mfma_f32_16x16x32_bf16 with W^T as the A operand held in VGPRs for the whole kernel
//     (a wave owns 16 output channels x all C4 inputs), dz as B;
//   * wgrad: v_mfma_f32_32x32x16_bf16, dz^T and xa through transposed reads, a wave owns a C4/4 x 64
//     block of dW in accumulators for the whole kernel; fp32 partials per workgroup summed afterwards
//     in a fixed order (deterministic);
//   * the dgrad tile leaves through an LDS staging tile as 16-B rows; the bn2 reduction is taken from
//     the rounded bf16 values, exactly as conv1x1.hip's BSTATS epilogue does.
//   * RECOMP: bn2's apply was deferred in the forward (conv3 read relu(a2 xb + b2) on load, conv1x1.hip
//     ATR), so xa = relu(a2 xb + b2) is formed here from xb — in registers, on the wgrad's B fragments
//     (one channel per lane: two coefficients) — with the same fma and rounding as the forward, and
//     bn2's ReLU mask is computed from xb and WRITTEN here (bn2's backward apply reads it next): xa and
//     the mask bits are never read.
#include "../common.h"
#include "../launchers.h"
#include "../tile_stats.h"

using namespace pdt;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef short s4v __attribute__((ext_vector_type(4)));
#define PDT_LDS __attribute__((address_space(3)))

__device__ __attribute__((aligned(256))) uint4 g_fb_zero[64];  // zero page for pixels past M (never written)
__device__ uint4 g_fb_sink[1024];  // epilogue stores of rows past M land here (keeps the vmcnt count exact)

// C4: the BatchNorm's channels (conv output), CW: the conv's input channels (NR = CW / 64 roles).
template <int C4_, int CW_, bool BSTATS_, bool RECOMP_ = false>
struct FB {
  static constexpr int C4 = C4_, CW = CW_, NG = 1, NR = CW / 64, kSlots = 3;
  static constexpr int kWaves = 4, kThreads = 256;
  static constexpr int KP = C4 >= 512 ? 16 : 32;  // pixels per stage (LDS: 3 slots + the dz tile)
  static constexpr bool BSTATS = BSTATS_ || RECOMP_, RECOMP = RECOMP_;
  // the transform coefficients: kernel-lifetime VGPRs, or an LDS table when the wgrad accumulators
  // of all NG slices need the registers
  static constexpr bool kCoefLds = NG > 1;
  static constexpr int kRowY = C4 * 2, kRowX = 128;  // LDS rows: dy / z / dz; a 64-channel slice
  static constexpr int kY = KP * kRowY, kMZ = KP * C4 / 8, kXA = KP * kRowX;
  static constexpr int kMBRow = 8 * NG;              // bn2 mask bytes per pixel (this role's slices)
  // 16-B DMA pieces (1 KB per wave instruction): Y, Z, XA (NG slices), XB (NG slices), dummies
  static constexpr int pY = kY / 1024, pX = kXA / 1024;
  static constexpr int nXsrc = RECOMP ? 1 : (BSTATS ? 2 : 1);  // xa and / or xb staged
  static constexpr int p16 = 2 * pY + pX * NG * nXsrc;
  static constexpr int n16 = (p16 + kWaves - 1) / kWaves;
  // 4-B DMA pieces (256 B per wave instruction; a sub-dword LDS-DMA does not land at lane x size —
  // measured): bn3's mask rows, and bn2's mask bytes (one instruction: <= 64 / (2 NG) rows)
  static constexpr int pMZ = kMZ / 256;
  static constexpr int pMB = (BSTATS && !RECOMP) ? 1 : 0;
  static constexpr int n4 = (pMZ + pMB + kWaves - 1) / kWaves;
  static constexpr int oY = 0, oZ = kY, oMZ = 2 * kY, oXA = oMZ + kMZ;
  static constexpr int oXB = RECOMP ? oXA : oXA + NG * kXA;  // RECOMP: only xb is staged (xa formed from it)
  static constexpr int oMB = oXB + (BSTATS ? NG * kXA : 0);
  static constexpr int oPad = oMB + (pMB ? 256 : 0);        // dummy pieces land here
  static constexpr bool kPad = n16 * kWaves > p16 || n4 * kWaves > pMZ + pMB;
  static constexpr int kSlot = (oPad + (kPad ? 1024 : 0) + 255) / 256 * 256;
  static constexpr int oDZ = kSlots * kSlot;
  static constexpr int oXC = oDZ + kY;                     // RECOMP: bn2's coefficients, [2][CW] fp32
  static constexpr int oCT = oXC + (RECOMP ? 8 * CW : 0);  // kCoefLds: mean, A, B, D [4][C4] fp32
  static constexpr int kLds = oCT + (kCoefLds ? 16 * C4 : 0);
  static constexpr int kG = n16 + n4;  // DMA instructions per wave per stage
  // epilogue: one 16-B chunk of the dgrad slice per thread per stage (threads past the tile store to
  // a sink: every thread stores once, so the vmcnt counts are exact) + the bn2 mask byte (RECOMP)
  static constexpr int kStageOps = kG + 1 + (RECOMP ? 1 : 0);
  static constexpr int kStgStride = kRowX + 16;  // staging rows padded: conflict-free 8-B writes
  static constexpr int kKS = C4 / 32;            // 16x16x32 k-steps of the dgrad (W^T fragments in VGPRs)
  static constexpr int kPB = KP / 16;            // pixel blocks of the dgrad tile
  static constexpr int kWR = C4 / 4;             // dW rows per wave (4 waves cover C4), all CW columns
  static constexpr int kMI = kWR / 32, kNJ = 2 * NG;
  static constexpr int kEpiPer = KP * 8;         // epilogue chunks per slice (one thread each)
  static_assert(CW % 64 == 0 && C4 % 256 == 0 && NG <= 2, "shapes");
  static_assert(NG * KP * 8 <= kThreads, "one epilogue chunk per thread at most");
  static_assert(kEpiPer % 64 == 0, "an epilogue wave stays in one slice");
  static_assert(KP * 2 * NG <= 64, "bn2 mask: one 4-B DMA instruction per stage");
  static_assert(KP * C4 / 8 % kThreads == 0, "transform chunks");
  static_assert(NG * KP * kStgStride <= kY, "staging fits the dead z region");
  static_assert(kLds <= 160 * 1024, "LDS");
};

// dz tile swizzle (16-B chunk index ^= g(row)), an involution within the row.
__device__ __forceinline__ int swz_dz(int row, int ch) { return ch ^ (((row & 3) << 2) | ((row >> 2) & 2)); }
// 128-B rows of the transposed-read operands (conv1x1_wgrad.hip): rows r, r+1 are the two halves of
// a 256-B bank row, r+2, r+3 flip chunk bit 2.
__device__ __forceinline__ int swz128(int row, int ch) { return ch ^ (((row >> 1) & 1) << 2); }

__device__ __forceinline__ s4v tr_read(const char* p) {
  s4v r;
  const uint32_t a = (uint32_t)(uintptr_t)(PDT_LDS const char*)p;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(a) : "memory");
  return r;
}
__device__ __forceinline__ bf16x8 cat2(s4v a, s4v b) {
  typedef short s8 __attribute__((ext_vector_type(8)));
  s8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, r);
}
// LDS-DMA (lane i's SZ bytes land at M0 + SZ i) issued from inline asm: the builtin makes the
// compiler assume the DMA may alias every later LDS access and put a vmcnt(0) in front of the
// transform pass's reads and writes — i.e. wait for the prefetch it was meant to overlap (seen in
// this kernel's ISA; conv_stem.hip has the same note). Ordering is by the counted vmcnt waits and
// barriers below instead.
template <int SZ>
__device__ __forceinline__ void dma(const void* src, char* lds_wave_base) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(PDT_LDS const char*)lds_wave_base);
  static_assert(SZ == 16 || SZ == 4, "16-B or 4-B pieces");
  if constexpr (SZ == 16)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0) : "memory");
  else
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(src), "s"(m0) : "memory");
}
// s_waitcnt vmcnt(N) leaving expcnt / lgkmcnt unconstrained (gfx9 simm16 encoding)
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

struct FBArgs {
  const uint16_t* dy;   // [M][C4] gradient at the BatchNorm output
  const uint16_t* z;    // [M][C4] BatchNorm input (= conv output)
  const uint8_t* mz;    // [M*C4/8] BatchNorm ReLU bits
  const float* mean;    // [C4]
  const float* A;       // [C4] dz = A dy m + B (z - mean) + D
  const float* B;
  const float* D;
  const uint16_t* wt;   // [CW][C4] conv weight transposed (W^T)
  const uint16_t* xa;   // [M][CW] conv input
  BnSrc bs;             // bn2: input xb [M][CW], mask, mean; part [2][G][CW]
  const float* xcoef;   // RECOMP: bn2's forward apply [2][CW] (a, b): xa = relu(a xb + b)
  uint8_t* mask_out;    // RECOMP: bn2's ReLU bits [M*CW/8], written here
  uint16_t* dxa;        // [M][CW]
  float* ws;            // [G][C4][CW] wgrad partials
  int M, ntiles, G;     // G: pixel groups (workgroups per role)
};

template <class Cf>
__global__ __launch_bounds__(Cf::kThreads, 1) void conv1x1_bwd_fused_kernel(FBArgs a) {
  constexpr int C4 = Cf::C4, CW = Cf::CW, KP = Cf::KP, RY = Cf::kRowY, RX = Cf::kRowX, NT = Cf::kThreads;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  // wid through readfirstlane: the compiler then keeps everything derived from it (the DMA pieces'
  // bases, strides, LDS destinations) in SGPRs
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wid;                      // dW rows / dgrad channels of this wave (in every slice)
  // block -> (pixel group, role): the NR roles of a pixel group are blocks b, b + 8, ... (one XCD
  // under round-robin placement — speed only, never correctness)
  constexpr int NR = Cf::NR;
  const int b = blockIdx.x;
  const int role = (b / 8) % NR, g = (b % 8) + 8 * (b / (8 * NR));
  const int G = a.G, cs = role * 64 * Cf::NG;  // pixel groups; this workgroup's first channel of CW
  if (g >= G) return;  // the grid is rounded up to whole XCD pairings (uniform exit, no barrier yet)
  const int S = (a.ntiles - g + G - 1) / G;  // tiles g, g + G, ... (G <= ntiles: S >= 1)

  // ---- kernel-lifetime registers: W^T fragments (dgrad A operand), the transform coefficients
  bf16x8 wf[Cf::NG][Cf::kKS];
#pragma unroll
  for (int sl = 0; sl < Cf::NG; ++sl)
#pragma unroll
    for (int ks = 0; ks < Cf::kKS; ++ks)
      wf[sl][ks] = *reinterpret_cast<const bf16x8*>(a.wt + (int64_t)(cs + sl * 64 + 16 * wq + (lane & 15)) * C4 +
                                                    32 * ks + 8 * (lane >> 4));
  const int tc = tid % (C4 / 8);  // transform pass: this thread's 8-channel chunk (fixed)
  float cm[8], cA[8], cB[8], cD[8];
  float* const ctab = reinterpret_cast<float*>(lds + Cf::oCT);
  if constexpr (Cf::kCoefLds) {
    for (int i = tid; i < C4; i += NT) {
      ctab[i] = a.mean[i]; ctab[C4 + i] = a.A[i]; ctab[2 * C4 + i] = a.B[i]; ctab[3 * C4 + i] = a.D[i];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { cm[k] = 0.f; cA[k] = 0.f; cB[k] = 0.f; cD[k] = 0.f; }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      cm[k] = a.mean[tc * 8 + k]; cA[k] = a.A[tc * 8 + k]; cB[k] = a.B[tc * 8 + k]; cD[k] = a.D[tc * 8 + k];
    }
  }
  const int eg = tid / Cf::kEpiPer, el = tid % Cf::kEpiPer;  // epilogue: slice, then chunk / pixel row
  const int ec = el % 8, er = el / 8;
  const int ecs = cs + eg * 64;               // the epilogue thread's slice
  float bmu[8], bs1[8], bs2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { bs1[k] = 0.f; bs2[k] = 0.f; bmu[k] = 0.f; }
  if constexpr (Cf::BSTATS) {
    if (eg < Cf::NG) {
#pragma unroll
      for (int k = 0; k < 8; ++k) bmu[k] = a.bs.mean[ecs + ec * 8 + k];
    }
  }
  // RECOMP: bn2's forward coefficients of this lane's wgrad B columns (32 j + lane % 32); the
  // epilogue's 8-channel coefficients come from an LDS copy, filled here
  float xca[Cf::kNJ], xcb[Cf::kNJ];
#pragma unroll
  for (int j = 0; j < Cf::kNJ; ++j) { xca[j] = 0.f; xcb[j] = 0.f; }
  float* const xct = reinterpret_cast<float*>(lds + Cf::oXC);
  if constexpr (Cf::RECOMP) {
#pragma unroll
    for (int j = 0; j < Cf::kNJ; ++j) {
      xca[j] = a.xcoef[cs + 32 * j + (lane & 31)];
      xcb[j] = a.xcoef[CW + cs + 32 * j + (lane & 31)];
    }
    for (int i = tid; i < 2 * CW; i += NT) xct[i] = a.xcoef[i];  // [a | b]
  }
  // the loads above complete before any DMA is issued (no vmcnt(0) inside the ring); the LDS tables
  // are visible to every wave after the first stage's barrier
#pragma unroll
  for (int j = 0; j < Cf::kNJ; ++j) asm volatile("" : "+v"(xca[j]), "+v"(xcb[j]));
#pragma unroll
  for (int sl = 0; sl < Cf::NG; ++sl)
#pragma unroll
    for (int ks = 0; ks < Cf::kKS; ++ks) asm volatile("" : "+v"(wf[sl][ks]));
#pragma unroll
  for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(cm[k]), "+v"(cA[k]), "+v"(cB[k]), "+v"(cD[k]), "+v"(bmu[k]));

  // ---- per-lane 16-B DMA pieces (stage independent). Piece q = wid + kWaves * i of the stage's
  // list [Y][Z][XA slices][XB slices][dummies]: source = base + p0 * stride + off, valid while the
  // pixel row is < M (else the zero page), LDS destination = slot + dst.
  const uint16_t* pbase[Cf::n16];
  int pstride[Cf::n16], prow[Cf::n16], poff[Cf::n16], pdst[Cf::n16];
#pragma unroll
  for (int i = 0; i < Cf::n16; ++i) {
    const int q = wid + Cf::kWaves * i;
    if (q < 2 * Cf::pY) {  // dy / z: linear C4-channel rows
      const int o = (q % Cf::pY) * 1024 + lane * 16;
      pbase[i] = q < Cf::pY ? a.dy : a.z;
      pstride[i] = C4;
      prow[i] = o / RY;
      poff[i] = prow[i] * C4 + ((o % RY) >> 4) * 8;
      pdst[i] = (q < Cf::pY ? Cf::oY : Cf::oZ) + (q % Cf::pY) * 1024;
    } else if (q < 2 * Cf::pY + Cf::nXsrc * Cf::NG * Cf::pX) {  // xa / xb slices: swizzled 128-B rows
      const int qq = q - 2 * Cf::pY;
      const int src = qq / (Cf::NG * Cf::pX), sl = (qq / Cf::pX) % Cf::NG, k = qq % Cf::pX;
      const bool is_xa = !Cf::RECOMP && src == 0;
      const int o = k * 1024 + lane * 16;
      pbase[i] = (is_xa ? a.xa : a.bs.x) + cs + sl * 64;
      pstride[i] = CW;
      prow[i] = o / RX;
      poff[i] = prow[i] * CW + swz128(prow[i], (o % RX) >> 4) * 8;
      pdst[i] = (is_xa ? Cf::oXA : Cf::oXB) + sl * Cf::kXA + k * 1024;
    } else {  // dummy: zero page -> the slot's pad area (keeps every wave's DMA count equal)
      pbase[i] = reinterpret_cast<const uint16_t*>(g_fb_zero);
      pstride[i] = 0;
      prow[i] = 0;
      poff[i] = 0;
      pdst[i] = Cf::oPad;
    }
  }
  auto issue = [&](int s) {
    char* slot = lds + (s % Cf::kSlots) * Cf::kSlot;
    const int p0 = (g + s * G) * KP;
#pragma unroll
    for (int i = 0; i < Cf::n16; ++i) {
      const bool ok = p0 + prow[i] < a.M;
      dma<16>(ok ? (const void*)(pbase[i] + (int64_t)p0 * pstride[i] + poff[i]) : (const void*)g_fb_zero,
              slot + pdst[i]);
    }
#pragma unroll
    for (int i = 0; i < Cf::n4; ++i) {
      const int q = wid + Cf::kWaves * i;
      if (q < Cf::pMZ) {  // bn3's mask rows: 256 B = 256 / (C4/8) pixel rows
        const int o = q * 256 + lane * 4;
        const bool ok = p0 + o / (C4 / 8) < a.M;
        dma<4>(ok ? (const void*)(a.mz + (int64_t)p0 * (C4 / 8) + o) : (const void*)g_fb_zero,
               slot + Cf::oMZ + q * 256);
      } else if (q < Cf::pMZ + Cf::pMB) {  // bn2's mask bytes of every slice: lane = 4 B of a row
        const int row = lane / (2 * Cf::NG), wd = lane % (2 * Cf::NG);
        const bool ok = a.bs.mask != nullptr && row < KP && p0 + row < a.M;
        dma<4>(ok ? (const void*)(a.bs.mask + (int64_t)(p0 + row) * (CW / 8) + cs / 8 + wd * 4) : (const void*)g_fb_zero,
               slot + (a.bs.mask != nullptr ? Cf::oMB : Cf::oPad));
      } else {
        dma<4>((const void*)g_fb_zero, slot + Cf::oPad);
      }
    }
  };

  // ---- wgrad lane roles (transposed reads; conv1x1_wgrad.hip)
  const int grp = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  const int prw = 8 * (grp >> 1) + q4, half8 = (p4 & 1) * 8;
  int ya[Cf::kMI], xa[Cf::kNJ];
#pragma unroll
  for (int i = 0; i < Cf::kMI; ++i)
    ya[i] = prw * RY + (swz_dz(prw, (wq * Cf::kWR + 32 * i + 16 * (grp & 1) + 4 * p4) >> 3) << 4) + half8;
#pragma unroll
  for (int j = 0; j < Cf::kNJ; ++j)  // column block j: slice j / 2, its columns 32 (j % 2) ..
    xa[j] = (j / 2) * Cf::kXA + prw * RX + (swz128(prw, (32 * (j % 2) + 16 * (grp & 1) + 4 * p4) >> 3) << 4) + half8;
  f16v acc[Cf::kMI][Cf::kNJ];
#pragma unroll
  for (int i = 0; i < Cf::kMI; ++i)
#pragma unroll
    for (int j = 0; j < Cf::kNJ; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

  char* const dzs = lds + Cf::oDZ;
#pragma unroll
  for (int s = 0; s < Cf::kSlots - 1; ++s)
    if (s < S) issue(s);
  for (int s = 0; s < S; ++s) {
    // stage s's DMA is done once only the next stage's DMA (+ the previous stage's epilogue stores,
    // issued after it) is pending; every count is exact
    if (s + 1 >= S) wait_vm<0>();
    else if (s == 0) wait_vm<Cf::kG>();
    else wait_vm<Cf::kStageOps>();
    lds_barrier();  // B1: DMA(s) visible to all waves; every wave is past stage s-1
    if (s + Cf::kSlots - 1 < S) issue(s + Cf::kSlots - 1);  // its slot was last used in stage s-1
    const char* slot = lds + (s % Cf::kSlots) * Cf::kSlot;
    const int p0 = (g + s * G) * KP;

    // ---- transform: dz = A dy m + B (z - mean) + D -> swizzled dz tile (rows past M: zero)
#pragma unroll
    for (int i = 0; i < KP * C4 / 8 / NT; ++i) {
      const int r = tid / (C4 / 8) + i * (NT / (C4 / 8));
      if constexpr (Cf::kCoefLds) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          *reinterpret_cast<float4*>(cm + 4 * h) = *reinterpret_cast<const float4*>(ctab + tc * 8 + 4 * h);
          *reinterpret_cast<float4*>(cA + 4 * h) = *reinterpret_cast<const float4*>(ctab + C4 + tc * 8 + 4 * h);
          *reinterpret_cast<float4*>(cB + 4 * h) = *reinterpret_cast<const float4*>(ctab + 2 * C4 + tc * 8 + 4 * h);
          *reinterpret_cast<float4*>(cD + 4 * h) = *reinterpret_cast<const float4*>(ctab + 3 * C4 + tc * 8 + 4 * h);
        }
      }
      const uint4 gv = *reinterpret_cast<const uint4*>(slot + Cf::oY + r * RY + tc * 16);
      const uint4 zv = *reinterpret_cast<const uint4*>(slot + Cf::oZ + r * RY + tc * 16);
      const unsigned mk = *reinterpret_cast<const uint8_t*>(slot + Cf::oMZ + r * (C4 / 8) + tc);
      const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w}, zw[4] = {zv.x, zv.y, zv.z, zv.w};
      float o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gk = __uint_as_float(k & 1 ? (gw[k >> 1] & 0xffff0000u) : (gw[k >> 1] << 16));
        const float zk = __uint_as_float(k & 1 ? (zw[k >> 1] & 0xffff0000u) : (zw[k >> 1] << 16));
        const float gm = (mk >> k) & 1u ? gk : 0.f;
        o[k] = cA[k] * gm + cB[k] * (zk - cm[k]) + cD[k];
      }
      uint4 ov;
      if (p0 + r < a.M) {
        ov.x = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
        ov.y = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
        ov.z = (uint32_t)f2bf(o[4]) | ((uint32_t)f2bf(o[5]) << 16);
        ov.w = (uint32_t)f2bf(o[6]) | ((uint32_t)f2bf(o[7]) << 16);
      } else {
        ov = make_uint4(0u, 0u, 0u, 0u);
      }
      *reinterpret_cast<uint4*>(dzs + r * RY + (swz_dz(r, tc) << 4)) = ov;
    }
    lds_barrier();  // B2: dz tile complete; z region of this slot is dead (reused as staging)

    // ---- dgrad: D[ci][px] = sum_c W^T[ci][c] dz[px][c]; lane holds 4 consecutive ci of one pixel
    f4 dacc[Cf::NG][Cf::kPB];
#pragma unroll
    for (int sl = 0; sl < Cf::NG; ++sl)
#pragma unroll
      for (int pb = 0; pb < Cf::kPB; ++pb) dacc[sl][pb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < Cf::kKS; ++ks) {
#pragma unroll
      for (int pb = 0; pb < Cf::kPB; ++pb) {
        const int row = 16 * pb + (lane & 15), ch = 4 * ks + (lane >> 4);
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(dzs + row * RY + (swz_dz(row, ch) << 4));
#pragma unroll
        for (int sl = 0; sl < Cf::NG; ++sl)
          dacc[sl][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[sl][ks], bv, dacc[sl][pb], 0, 0, 0);
      }
    }
    // ---- wgrad: dW[c][k] += sum_px dz[px][c] xa[px][k]
    const char* xas = slot + (Cf::RECOMP ? Cf::oXB : Cf::oXA);
#pragma unroll
    for (int kk = 0; kk < KP / 16; ++kk) {
      bf16x8 fa[Cf::kMI], fb[Cf::kNJ];
#pragma unroll
      for (int i = 0; i < Cf::kMI; ++i) {
        const char* pp = dzs + ya[i] + kk * 16 * RY;
        fa[i] = cat2(tr_read(pp), tr_read(pp + 4 * RY));
      }
#pragma unroll
      for (int j = 0; j < Cf::kNJ; ++j) {
        const char* pp = xas + xa[j] + kk * 16 * RX;
        fb[j] = cat2(tr_read(pp), tr_read(pp + 4 * RX));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < Cf::kMI; ++i) asm volatile("" : "+v"(fa[i]));
#pragma unroll
      for (int j = 0; j < Cf::kNJ; ++j) asm volatile("" : "+v"(fb[j]));
      if constexpr (Cf::RECOMP) {  // xa = relu(a xb + b): 8 pixels of ONE channel per lane
#pragma unroll
        for (int j = 0; j < Cf::kNJ; ++j) {
          typedef unsigned u4 __attribute__((ext_vector_type(4)));
          const u4 w = __builtin_bit_cast(u4, fb[j]);
          u4 o;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float t0 = __uint_as_float(w[k] << 16) * xca[j] + xcb[j];
            const float t1 = __uint_as_float(w[k] & 0xffff0000u) * xca[j] + xcb[j];
            o[k] = (uint32_t)f2bf(t0 > 0.f ? t0 : 0.f) | ((uint32_t)f2bf(t1 > 0.f ? t1 : 0.f) << 16);
          }
          fb[j] = __builtin_bit_cast(bf16x8, o);
        }
      }
#pragma unroll
      for (int i = 0; i < Cf::kMI; ++i)
#pragma unroll
        for (int j = 0; j < Cf::kNJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }

    // ---- epilogue: stage each slice's bf16 dgrad tile [KP][64] in the dead z region, 16-B rows out
    char* stg = const_cast<char*>(slot) + Cf::oZ;
#pragma unroll
    for (int sl = 0; sl < Cf::NG; ++sl)
#pragma unroll
      for (int pb = 0; pb < Cf::kPB; ++pb) {
        const int px = 16 * pb + (lane & 15), ci = 16 * wq + 4 * (lane >> 4);
        const f4 v = dacc[sl][pb];
        uint2 pk;
        pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
        pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
        *reinterpret_cast<uint2*>(stg + (sl * KP + px) * Cf::kStgStride + ci * 2) = pk;
      }
    lds_barrier();  // B3
    {
      const bool in_tile = eg < Cf::NG && er < KP;  // (threads past the tile: the sink store only)
      const uint4 v = *reinterpret_cast<const uint4*>(stg + (in_tile ? eg * KP + er : 0) * Cf::kStgStride + ec * 16);
      if (in_tile && p0 + er < a.M) {
        const char* xbp = slot + Cf::oXB + eg * Cf::kXA + er * RX + (swz128(er, ec) << 4);
        if constexpr (Cf::RECOMP) {  // bn2's mask from its input, same fma as its forward apply
          const uint4 xb = *reinterpret_cast<const uint4*>(xbp);
          const uint32_t xw[4] = {xb.x, xb.y, xb.z, xb.w};
          float eca[8], ecb[8];
          *reinterpret_cast<float4*>(eca) = *reinterpret_cast<const float4*>(xct + ecs + ec * 8);
          *reinterpret_cast<float4*>(eca + 4) = *reinterpret_cast<const float4*>(xct + ecs + ec * 8 + 4);
          *reinterpret_cast<float4*>(ecb) = *reinterpret_cast<const float4*>(xct + CW + ecs + ec * 8);
          *reinterpret_cast<float4*>(ecb + 4) = *reinterpret_cast<const float4*>(xct + CW + ecs + ec * 8 + 4);
          unsigned mk = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float xv = __uint_as_float(k & 1 ? (xw[k >> 1] & 0xffff0000u) : (xw[k >> 1] << 16));
            mk |= (xv * eca[k] + ecb[k] > 0.f ? 1u : 0u) << k;
          }
          bn_bwd_accum8(v, xb, mk, bmu, bs1, bs2);
          a.mask_out[((int64_t)(p0 + er) * CW + ecs) / 8 + ec] = (uint8_t)mk;
        } else if constexpr (Cf::BSTATS) {
          const uint4 xb = *reinterpret_cast<const uint4*>(xbp);
          const unsigned mk = *reinterpret_cast<const uint8_t*>(slot + Cf::oMB + er * Cf::kMBRow + eg * 8 + ec);
          bn_bwd_accum8(v, xb, a.bs.mask ? mk : 0xffu, bmu, bs1, bs2);
        }
        *reinterpret_cast<uint4*>(a.dxa + (int64_t)(p0 + er) * CW + ecs + ec * 8) = v;
      } else {
        g_fb_sink[tid] = v;  // one store per thread per stage, always (exact vmcnt counts)
        if constexpr (Cf::RECOMP) reinterpret_cast<uint8_t*>(g_fb_sink)[8192 + tid] = 0;
      }
    }
  }
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- wgrad partials ws[g][c][k]; 32x32 accumulator: lane holds k = l % 32,
  // c = 8 (v / 4) + 4 (l / 32) + v % 4 for v = 0..15
  float* wsp = a.ws + (int64_t)g * C4 * CW + cs;
#pragma unroll
  for (int i = 0; i < Cf::kMI; ++i)
#pragma unroll
    for (int j = 0; j < Cf::kNJ; ++j) {
      const int k = 32 * j + (lane & 31);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int c = wq * Cf::kWR + 32 * i + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        wsp[(int64_t)c * CW + k] = acc[i][j][v];
      }
    }
  if constexpr (Cf::BSTATS) {
    // bn2 partials of this workgroup: lanes holding one chunk differ in lane bits 3..5 (a wave stays
    // in one slice); then the waves of a slice in order (fixed-order: deterministic)
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // v += v[lane ^ 8], [lane ^ 16], [lane ^ 32] (common.h xor_add)
      bs1[k] = xor_add<32>(xor_add<16>(xor_add<8>(bs1[k])));
      bs2[k] = xor_add<32>(xor_add<16>(xor_add<8>(bs2[k])));
    }
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
    if (lane < 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        red[wid * 128 + lane * 8 + k] = bs1[k];
        red[wid * 128 + 64 + lane * 8 + k] = bs2[k];
      }
    }
    __syncthreads();
    constexpr int kWps = Cf::kEpiPer / 64;  // waves per slice in the epilogue
    for (int t = tid; t < Cf::NG * 128; t += NT) {
      const int sl = t / 128, st = (t / 64) % 2, ch = t % 64;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < kWps; ++w) sum += red[(sl * kWps + w) * 128 + st * 64 + ch];
      a.bs.part[((int64_t)st * G + g) * CW + cs + sl * 64 + ch] = sum;
    }
  }
}

// dw[c][k] (bf16) = sum over the G workgroup partials in a fixed order (conv1x1_wgrad.hip's scheme:
// 16 groups take the partials round-robin, then one fixed-order pass over the group sums).
constexpr int kRedCols = 16, kRedGroups = 16;
__global__ __launch_bounds__(256) void fb_reduce_kernel(const float* __restrict__ ws, uint16_t* __restrict__ dw,
                                                        int nsplit, int64_t n4) {
  __shared__ float4 part[kRedGroups][kRedCols];
  const int col = threadIdx.x % kRedCols, grp = threadIdx.x / kRedCols;
  const int64_t i = (int64_t)blockIdx.x * kRedCols + col;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4)
    for (int k = grp; k < nsplit; k += kRedGroups) {
      const float4 v = reinterpret_cast<const float4*>(ws + (int64_t)k * n4 * 4)[i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0 && i < n4) {
    float4 t = part[0][col];
#pragma unroll
    for (int k = 1; k < kRedGroups; ++k) {
      const float4 v = part[k][col];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    const uint32_t lo = (uint32_t)f2bf(t.x) | ((uint32_t)f2bf(t.y) << 16);
    const uint32_t hi = (uint32_t)f2bf(t.z) | ((uint32_t)f2bf(t.w) << 16);
    reinterpret_cast<uint2*>(dw)[i] = make_uint2(lo, hi);
  }
}

int g_grid = 0;  // 0: one workgroup per CU

// pixel groups: one workgroup per CU in all (NR roles each), a multiple of 8 (XCD pairing)
inline int groups_of(int ntiles, int nr) {
  int want = g_grid > 0 ? g_grid : 256;
  want = want / nr / 8 * 8;
  if (want < 8) want = 8;
  return ntiles < want ? ntiles : want;
}

template <class Cf>
int launch(const FBArgs& a0, uint16_t* dw, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_bwd_fused_kernel<Cf>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, Cf::kLds) != hipSuccess)
      return -3;
    attr = true;
  }
  // every role of every pixel group with the pairing of the block map (the grid is rounded up to a
  // multiple of 8 * NR; groups past G exit at once)
  const int nblk = ((a0.G + 7) / 8) * 8 * Cf::NR;
  hipLaunchKernelGGL(conv1x1_bwd_fused_kernel<Cf>, dim3(nblk), dim3(Cf::kThreads), Cf::kLds, s, a0);
  const int64_t n4 = (int64_t)Cf::C4 * Cf::CW / 4;
  hipLaunchKernelGGL(fb_reduce_kernel, dim3((unsigned)((n4 + kRedCols - 1) / kRedCols)), dim3(kRedCols * kRedGroups),
                     0, s, a0.ws, dw, a0.G, n4);
  return 0;
}

inline int kp_of(int C4) { return C4 >= 512 ? 16 : 32; }

}  // namespace

extern "C" {

// Shapes the fused kernel takes: (C4, CW) = (256, 64) and (512, 128) (ResNet-50 layers 1 and 2).
int pdt_conv1x1_bwd_fused_ok(int C4, int CW) { return (C4 == 256 && CW == 64) || (C4 == 512 && CW == 128); }

// Workgroups of a call = wgrad partial slabs (workspace G*C4*CW floats) = bn2 partial rows ([2][G][CW]).
int pdt_conv1x1_bwd_fused_grid(int M, int C4, int CW) {
  const int kp = kp_of(C4);
  return groups_of((M + kp - 1) / kp, CW / 64);
}

// See the header. dy, z: [M][C4]; mz: M*C4/8 bytes; mean/A/B/D: [C4]; wt: [CW][C4]; xa: [M][CW];
// bx / bm / bmean / bpart (all null = no bn2 reduction; bm may be null = no ReLU): bn2's input
// [M][CW], mask, mean [CW] and the [2][G][CW] partials out; dxa: [M][CW]; dw: [C4][CW] bf16;
// ws: G*C4*CW floats. xcoef / mask_out (RECOMP, both or neither): xa is NOT read — it is
// relu(xcoef[0] bx + xcoef[1]) (bn2's deferred forward apply; xa may be null) — and bn2's ReLU bits are
// computed and written to mask_out (bm unused); needs bx / bmean / bpart. Returns 0, -1 for an
// unsupported shape.
int pdt_conv1x1_bwd_fused(const uint16_t* dy, const uint16_t* z, const uint8_t* mz, const float* mean, const float* A,
                          const float* B, const float* D, const uint16_t* wt, const uint16_t* xa, const uint16_t* bx,
                          const uint8_t* bm, const float* bmean, float* bpart, const float* xcoef, uint8_t* mask_out,
                          uint16_t* dxa, uint16_t* dw, float* ws, int M, int C4, int CW, hipStream_t s) {
  if (!pdt_conv1x1_bwd_fused_ok(C4, CW) || M < 1 || (int64_t)M * C4 >= ((int64_t)1 << 31)) return -1;
  if ((bx != nullptr) != (bpart != nullptr) || (bx && !bmean)) return -1;
  const bool rc = xcoef != nullptr;
  if (rc != (mask_out != nullptr) || (rc && !bx) || (!rc && !xa)) return -1;
  const int kp = kp_of(C4), ntiles = (M + kp - 1) / kp;
  FBArgs a{dy, z, mz, mean, A, B, D, wt, xa, BnSrc{bx, bm, bmean, bpart}, xcoef, mask_out, dxa, ws, M, ntiles,
           pdt_conv1x1_bwd_fused_grid(M, C4, CW)};
  if (C4 == 256) {
    if (rc) return launch<FB<256, 64, true, true>>(a, dw, s);
    if (bx) return launch<FB<256, 64, true>>(a, dw, s);
    return launch<FB<256, 64, false>>(a, dw, s);
  }
  if (rc) return launch<FB<512, 128, true, true>>(a, dw, s);
  if (bx) return launch<FB<512, 128, true>>(a, dw, s);
  return launch<FB<512, 128, false>>(a, dw, s);
}

// Tuning hook: workgroups per call (0 = one per CU).
void pdt_conv1x1_bwd_fused_tune(int grid) {
  if (grid >= 0) g_grid = grid;
}

}  // extern "C"
