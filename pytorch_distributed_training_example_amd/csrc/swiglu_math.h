// SwiGLU and its gradients on value pairs, shared by the SwiGLU kernels (kernels/swiglu.hip) and the fused
// SwiGLU + fp8 cast kernels (kernels/fp8.hip) so both produce the same fp32 values bit for bit.
#pragma once
#include "gelu_math.h"

namespace pdt {

// e^-g and sigma(g) of a pair. e^-g = 2^(-g log2 e) overflows to inf below g ~ -88.7: sigma = 0, cleanly.
// (Just above that, down from g ~ -87.3, sigma is subnormal and v_rcp_f32 may return 0 for it: |g sigma| < 1e-35.)
__device__ __forceinline__ void sigmoid2(gf2 g, gf2& e, gf2& sg) {
  e = exp2_2(g2(-1.4426950408889634f) * g);
  sg = rcp2(g2(1.f) + e);
}

// y = g sigma(g) u
__device__ __forceinline__ gf2 swiglu_fwd2(gf2 g, gf2 u) {
  gf2 e, sg;
  sigmoid2(g, e, sg);
  return g * sg * u;
}

// dg = dy u sigma(g) (1 + g (1 - sigma(g))), du = dy g sigma(g). 1 - sigma is formed as e^-g sigma for g > 0,
// where the subtraction would cancel.
__device__ __forceinline__ void swiglu_bwd2(gf2 dy, gf2 g, gf2 u, gf2& dg, gf2& du) {
  gf2 e, sg;
  sigmoid2(g, e, sg);
  const gf2 a = e * sg, b = g2(1.f) - sg;  // 1 - sg two ways
  const gf2 oms{g.x > 0.f ? a.x : b.x, g.y > 0.f ? a.y : b.y};
  dg = dy * u * sg * fma2(g, oms, g2(1.f));
  du = dy * g * sg;
}

}  // namespace pdt
