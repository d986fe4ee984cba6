// Dropout masks from a counter: one definition shared by every kernel (dropout.hip, layernorm.hip,
// attention.hip) and by the CPU reference (ops/dropout.py reference_mask). A mask is never stored:
// the forward and the backward regenerate it from (key, step, stream, element index).
//
// Generator: Philox4x32-10, standard constants (multipliers 0xD2511F53 / 0xCD9E8D57, key increments
// 0x9E3779B9 / 0xBB67AE85). Known answer: counter (0,0,0,0), key (0,0) ->
// 6627e8d5 e169c58d bc57ac4c 9b00dbd8. One call yields 128 bits = 16 mask bytes.
//
//   counter = (block_lo, block_hi, stream, step_lo32)      key = (key_lo, key_hi)
//
// Keep rule: element byte >= thr, thr = round(p * 256) clamped to 0..255; the EFFECTIVE probability
// p_eff = thr / 256 is what every kernel scales by (1 / (1 - p_eff)), so E[y] = x exactly.
//
// Key and rank: the 64-bit key is formed on the host (ops/dropout.py DropoutState.key) as
//   key = (seed + rank * 0x9E3779B97F4A7C15) mod 2^64
// so two ranks started with one --seed draw different masks; kernels only ever see the key. It
// travels with the step in the *ticket*, an int64[2] device tensor (key, step) written by
// dropout_begin_kernel, which also advances the device step counter (captured in a hipGraph: every
// replay draws fresh masks). `stream` numbers the dropout sites of one forward (host integer).
//
// Flat tensors (embedding output, residual-branch output), element i = row * D + col:
//   block = i >> 4, byte e = i & 15 = byte (e & 3) of word (e >> 2).
// A lane of the LayerNorm kernels owns 4 consecutive elements at a multiple of 4: one word.
//
// Attention probabilities, element (b, h, q, k) of [B, H, T, T]: 4 x 4 (query x key) patches.
//   TP    = (T + 3) >> 2                                   patches per side
//   block = ((b * H + h) * TP + (q >> 2)) * TP + (k >> 2)  (64-bit)
//   byte  = 4 * (q & 3) + (k & 3)   = byte (k & 3) of word (q & 3)
// A pure function of (b, h, q, k), H, T and the ticket: no tile size or kernel enters it.
// Why the patch and not a row of 16 keys: the forward and dQ kernels hold, per lane, one query and
// keys kv0 + 16 ks + 4 g + r (r = 0..3) -> the four keys of one patch row, i.e. ONE WORD (q & 3) of
// one call per 4 scores. The dK/dV kernel holds one key and queries 16 qs + 4 g + r -> byte (k & 3)
// of each of the four words of one call, again one call per 4 scores. A row-of-16-keys block would
// give the forward the same one call per 4 scores (a lane's 16 keys of a subtile are spread over 4
// lane groups), but the dK/dV lane would need a different block for every query: one call per score,
// 4x the Philox work of the patch layout in the kernel that already has the most VALU work.
// With patches the four lanes of a DPP quad (4 consecutive queries, resp. keys) also sit in the same
// patches in all three kernels, so attention.hip lets each quad lane compute a different block and
// passes the words round with quad-broadcast moves: one call per 16 scores, every byte used.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDT_HD __host__ __device__ __forceinline__
#else
#define PDT_HD inline
#endif

namespace pdt {

struct PhiloxOut {
  uint32_t w[4];
};

PDT_HD void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

PDT_HD PhiloxOut philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxOut{{c0, c1, c2, c3}};
}

// What a kernel needs of a dropout site: read once per thread from the ticket (uniform loads).
struct DropSite {
  uint32_t k0, k1, step, stream;
  uint32_t thr;  // keep iff byte >= thr
  float scale;   // 1 / (1 - thr / 256)
};

PDT_HD DropSite drop_site(const int64_t* ticket, int stream, int thr) {
  const uint64_t key = (uint64_t)ticket[0], step = (uint64_t)ticket[1];
  return DropSite{(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)step, (uint32_t)stream, (uint32_t)thr,
                  256.f / (float)(256 - thr)};
}

PDT_HD PhiloxOut drop_block(const DropSite& s, uint64_t block) {
  return philox4x32_10((uint32_t)block, (uint32_t)(block >> 32), s.stream, s.step, s.k0, s.k1);
}

PDT_HD bool drop_keep(uint32_t word, int byte, uint32_t thr) { return ((word >> (8 * byte)) & 0xffu) >= thr; }

// Flat layout: the word holding elements i .. i+3 (i % 4 == 0).
PDT_HD uint32_t drop_pick(const PhiloxOut& o, int word) {  // selects, not a dynamically indexed array
  return word == 0 ? o.w[0] : word == 1 ? o.w[1] : word == 2 ? o.w[2] : o.w[3];
}
PDT_HD uint32_t drop_flat_word(const DropSite& s, uint64_t i) {
  return drop_pick(drop_block(s, i >> 4), (int)((i >> 2) & 3));
}

// Attention layout: patch block index of (bh = b * H + h, q, k); TP = (T + 3) >> 2.
PDT_HD uint64_t drop_attn_block(uint64_t bh, int TP, int q, int k) {
  return (bh * (uint64_t)TP + (uint64_t)(q >> 2)) * (uint64_t)TP + (uint64_t)(k >> 2);
}

}  // namespace pdt
