// The rotary embedding's arithmetic, shared by rope.hip (in place on a whole sequence) and
// attn_decode.hip (at a per-sequence offset, into the K/V cache), so that both give the same bits for
// the same position: fp32 products and one rounding to bf16 per output by the caller's store.
#pragma once
#include "common.h"

namespace pdt {

// A lane's 8 pairs (lo[j], hi[j]) = (x[8q + j], x[32 + 8q + j]) of one head, rotated by the table rows
// cr / sr (the 8 cosines / sines of those pairs: cos + t * 32 + 8q). sign = -1 is the inverse rotation.
__device__ __forceinline__ void rope_rotate8(const float (&lo)[8], const float (&hi)[8], const float* cr,
                                             const float* sr, float sign, float (&olo)[8], float (&ohi)[8]) {
  float c[8], s[8];
  Vec4<float>::ld(cr, 0, *reinterpret_cast<float(*)[4]>(c));
  Vec4<float>::ld(cr, 4, *reinterpret_cast<float(*)[4]>(c + 4));
  Vec4<float>::ld(sr, 0, *reinterpret_cast<float(*)[4]>(s));
  Vec4<float>::ld(sr, 4, *reinterpret_cast<float(*)[4]>(s + 4));
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sj = s[j] * sign;
    olo[j] = lo[j] * c[j] - hi[j] * sj;
    ohi[j] = hi[j] * c[j] + lo[j] * sj;
  }
}

}  // namespace pdt
