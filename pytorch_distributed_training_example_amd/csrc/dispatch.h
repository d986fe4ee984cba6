// Host-side launch selection shared by the row-wise kernels' launchers (layernorm, rmsnorm, gelu, swiglu,
// softmax_ce, dropout, lenet): a runtime (dtype, width) pair picks a template instantiation, and one rule
// partitions rows over workgroups. Plain C++17 only, no device code and no HIP call, so the host self-test
// (host/host_selftest.cpp) includes it as it is.
#pragma once
#include <stdint.h>
#include <type_traits>

namespace pdt {

template <typename T> struct TypeTag { using type = T; };

// The launchers' dtype code: 0 = fp32, anything else = bf16 carried as uint16_t.
//   with_elem(dtype, [&](auto t) { using T = typename decltype(t)::type; ... });
template <typename F>
inline void with_elem(int dtype, F&& f) {
  if (dtype == 0) f(TypeTag<float>{});
  else f(TypeTag<uint16_t>{});
}

// Calls f(std::integral_constant<int, K>{}) for the listed K equal to k; false (f not called) if none is.
//   with_k<1, 2, 4>(D / 256, [&](auto kc) { constexpr int K = decltype(kc)::value; ... });
template <int... Ks, typename F>
inline bool with_k(int k, F&& f) {
  return ((k == Ks ? (f(std::integral_constant<int, Ks>{}), true) : false) || ...);
}

// Rows over workgroups: at least min_rows rows each, at most max_blocks workgroups, then evened out
// (rows_per_block = ceil(N / blocks), and blocks recounted so the last one is not empty). Returns the
// number of workgroups; an empty input has none.
inline int row_blocks(int64_t N, int64_t min_rows, int64_t max_blocks, int& rows_per_block) {
  rows_per_block = 0;
  if (N <= 0) return 0;
  int64_t nblk = (N + min_rows - 1) / min_rows;
  if (nblk > max_blocks) nblk = max_blocks;
  if (nblk < 1) nblk = 1;
  rows_per_block = (int)((N + nblk - 1) / nblk);
  return (int)((N + rows_per_block - 1) / rows_per_block);
}

}  // namespace pdt
