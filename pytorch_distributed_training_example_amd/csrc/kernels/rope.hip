// Rotary position embedding, in place on the Q and K heads of the packed QKV tensor (gfx950).
//
// qkv: [B, T, H + 2 Hkv, 64] bf16: H query heads, then Hkv key heads, then Hkv value heads (the c_attn
// GEMM output, or the packed gradient attention's backward returns; Hkv == H is multi-head attention,
// three equal thirds); cos, sin: fp32 [T_max, 32] with T <= T_max. Half-split convention (HF's rotate_half): for
// every head of Q and K, position t and j < 32
//   x'[j]      = x[j]      * cos[t, j] - x[j + 32] * sin[t, j]
//   x'[j + 32] = x[j + 32] * cos[t, j] + x[j]      * sin[t, j]
// in fp32 with one rounding to bf16 per output. conj negates the sine: the inverse rotation, which is
// also the backward (the rotation is orthogonal). The V heads are neither read nor written, so the op
// costs one read and one write of the H + Hkv rotated heads.
//
// A lane owns 8 pairs of one head: x[8q .. 8q+8) and x[32+8q .. 32+8q+8), two 16-byte loads and two
// 16-byte stores, plus 2 x 32 bytes of each table row (L2-resident: T_max x 256 B). Nobody else touches
// those 16 elements, so the update is safe in place.
#include "../common.h"
#include "../launchers.h"
#include "../rope_math.h"

using namespace pdt;

namespace {

__global__ __launch_bounds__(256) void rope_qkv_kernel(uint16_t* __restrict__ qkv, const float* __restrict__ cs,
                                                       const float* __restrict__ sn, int64_t items, int T, int RH,
                                                       int AH, float sign) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= items) return;
  const int per_tok = 4 * RH;  // RH = H + Hkv rotated heads (Q then K) x 4 lanes; AH = H + 2 Hkv heads per token
  const int64_t tok = i / per_tok;
  const int r = (int)(i - tok * per_tok);
  const int head = r >> 2, q = r & 3;
  const int t = (int)(tok % T);
  uint16_t* p = qkv + tok * (int64_t)64 * AH + head * 64 + q * 8;
  float lo[8], hi[8];
  ld8_bf16(p, lo);
  ld8_bf16(p + 32, hi);
  float olo[8], ohi[8];  // the arithmetic is rope_math.h's, shared with the cache append (attn_decode.hip)
  rope_rotate8(lo, hi, cs + (int64_t)t * 32 + q * 8, sn + (int64_t)t * 32 + q * 8, sign, olo, ohi);
  st8_bf16(p, olo);
  st8_bf16(p + 32, ohi);
}

}  // namespace

extern "C" {

// In place on the first H + Hkv heads of qkv [B, T, (H + 2 Hkv) * 64] (contiguous, 16-byte aligned).
// conj != 0 rotates by -theta. The caller guarantees T <= the tables' row count.
int pdt_rope_qkv_gqa(uint16_t* qkv, const float* cos, const float* sin, int B, int T, int H, int Hkv, int conj,
                     hipStream_t s) {
  if (B < 0 || T < 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0) return -1;
  const int64_t items = (int64_t)B * T * 4 * (H + Hkv);
  if (items == 0) return 0;
  const int64_t grid = (items + 255) / 256;
  if (grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(rope_qkv_kernel, dim3((unsigned)grid), dim3(256), 0, s, qkv, cos, sin, items, T,
                     H + Hkv, H + 2 * Hkv, conj ? -1.f : 1.f);
  return 0;
}

// Multi-head form: Hkv == H, the first two thirds of qkv [B, T, 3 * H * 64].
int pdt_rope_qkv(uint16_t* qkv, const float* cos, const float* sin, int B, int T, int H, int conj, hipStream_t s) {
  return pdt_rope_qkv_gqa(qkv, cos, sin, B, T, H, H, conj, s);
}

}  // extern "C"
