// The second pass of every deterministic column reduction (LayerNorm dgamma/dbeta, RMSNorm dw, the
// bias-GELU / Linear bias gradients): fixed-order column sums of per-workgroup partial slabs.
#pragma once
#include "common.h"

namespace pdt {

// part[blk][NS][D] fp32, blk < nblk -> NS sums per column: slab 0 to out0, slab 1 (NS == 2 only) to out1.
// 16 columns x 16 slab groups per workgroup, so each thread sums only nblk/16 independent values
// (latency-bound otherwise): group g adds blocks g, g + 16, ..., then group 0 adds the 16 group sums in
// order. nblk == 0 writes zeros. Launch with (D + 15) / 16 workgroups of 256 threads.
template <int NS, typename TO>
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* __restrict__ part, int nblk, int D,
                                                              TO* __restrict__ out0, TO* __restrict__ out1) {
  static_assert(NS == 1 || NS == 2, "colsum_finalize_kernel: one or two interleaved slabs");
  __shared__ float red[NS][16][17];
  const int grp = threadIdx.x >> 4, cl = threadIdx.x & 15;
  const int c = blockIdx.x * 16 + cl;
  float a[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) a[n] = 0.f;
  if (c < D)
    for (int blk = grp; blk < nblk; blk += 16) {
      a[0] += part[((int64_t)blk * NS + 0) * D + c];
      if constexpr (NS == 2) a[1] += part[((int64_t)blk * NS + 1) * D + c];
    }
#pragma unroll
  for (int n = 0; n < NS; ++n) red[n][grp][cl] = a[n];
  __syncthreads();
  if (grp == 0 && c < D) {
    float sum[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) sum[n] = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int n = 0; n < NS; ++n) sum[n] += red[n][q][cl];
    Elt<TO>::st(out0, c, sum[0]);
    if constexpr (NS == 2) Elt<TO>::st(out1, c, sum[1]);
  }
}

}  // namespace pdt
