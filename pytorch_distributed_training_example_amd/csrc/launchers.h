// The C ABI between the kernels and their callers: every pdt_* launcher, tuning hook and size query,
// declared once. Each kernels/*.hip includes this header before it defines its launchers, and so do the
// callers (binding.cpp; the host self-test and tools/convbench through the .hip files they include), so
// a definition and a call that disagree on a parameter list fail to compile ("conflicting types")
// instead of linking by name alone. Grouped by the .hip file that holds the definition; no PyTorch
// dependency.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// kernels/amp.hip
int pdt_amp_unscale(int n, void* const* g, const int64_t* numel, int dtype, const float* inv_scale, float* found_inf,
                    hipStream_t s);
int pdt_amp_update(float* scale, int* growth_tracker, const float* found_inf, float growth, float backoff,
                   int interval, hipStream_t s);
int pdt_mt_scale(int n, void* const* x, const int64_t* numel, int dtype, const float* scale_ptr, float scale,
                 hipStream_t s);
int pdt_mt_copy(int n, void* const* src, void* const* dst, const int64_t* numel, int sdt, int ddt,
                const float* scale_ptr, float scale, hipStream_t s);
int pdt_l2norm_sq(int n, void* const* x, const int64_t* numel, int dtype, float* out, hipStream_t s);
int pdt_clip_coef(const float* sumsq, float max_norm, float* coef, float* norm, hipStream_t s);

// kernels/attention.hip
int pdt_attn_fwd(const uint16_t* q, const int64_t* qs, const uint16_t* k, const int64_t* ks, const uint16_t* v,
                 const int64_t* vs, uint16_t* o, const int64_t* os, float* lse, int B, int H, int T, int Dh,
                 int causal, float scale, hipStream_t s);
int pdt_attn_bwd(const uint16_t* dout, const int64_t* dos, const uint16_t* q, const int64_t* qs, const uint16_t* k,
                 const int64_t* ks, const uint16_t* v, const int64_t* vs, const uint16_t* o, const int64_t* os,
                 const float* lse, float* delta, uint16_t* dq, uint16_t* dk, uint16_t* dv, const int64_t* gs, int B,
                 int H, int T, int Dh, int causal, float scale, hipStream_t s);
int pdt_attn_fwd_drop(const uint16_t* q, const int64_t* qs, const uint16_t* k, const int64_t* ks, const uint16_t* v,
                      const int64_t* vs, uint16_t* o, const int64_t* os, float* lse, int B, int H, int T, int Dh,
                      int causal, float scale, const int64_t* ticket, int dstream, int thr, hipStream_t s);
int pdt_attn_bwd_drop(const uint16_t* dout, const int64_t* dos, const uint16_t* q, const int64_t* qs,
                      const uint16_t* k, const int64_t* ks, const uint16_t* v, const int64_t* vs, const uint16_t* o,
                      const int64_t* os, const float* lse, float* delta, uint16_t* dq, uint16_t* dk, uint16_t* dv,
                      const int64_t* gs, int B, int H, int T, int Dh, int causal, float scale, const int64_t* ticket,
                      int dstream, int thr, hipStream_t s);
// Grouped-query attention: q/o/do/dq have H heads, k/v/dk/dv have Hkv (H % Hkv == 0); query head h reads
// K/V head h / (H / Hkv). lse, delta: [B, H, T].
int pdt_attn_fwd_gqa(const uint16_t* q, const int64_t* qs, const uint16_t* k, const int64_t* ks, const uint16_t* v,
                     const int64_t* vs, uint16_t* o, const int64_t* os, float* lse, int B, int H, int Hkv, int T,
                     int Dh, int causal, float scale, hipStream_t s);
int pdt_attn_bwd_gqa(const uint16_t* dout, const int64_t* dos, const uint16_t* q, const int64_t* qs,
                     const uint16_t* k, const int64_t* ks, const uint16_t* v, const int64_t* vs, const uint16_t* o,
                     const int64_t* os, const float* lse, float* delta, uint16_t* dq, uint16_t* dk, uint16_t* dv,
                     const int64_t* gs, int B, int H, int Hkv, int T, int Dh, int causal, float scale, hipStream_t s);

// kernels/attn_decode.hip: KV-cache decoding. k_cache, v_cache [B, Hkv, capacity, 64] bf16; lens int32 [B] on
// the device (valid positions per sequence), never read on the host.
int pdt_rope_kv_append(uint16_t* qkv, const float* cos, const float* sin, uint16_t* k_cache, uint16_t* v_cache,
                       const int* lens, int B, int Tn, int H, int Hkv, int capacity, int Tmax, hipStream_t s);
int pdt_attn_decode_geo(int B, int Hkv, int capacity, int splits_override, int G, int* geo2);
int pdt_attn_decode(const uint16_t* qkv, int64_t q_sb, const uint16_t* k_cache, const uint16_t* v_cache,
                    const int* lens, float* o_part, float* ml_part, uint16_t* out, float* lse, int B, int H, int Hkv,
                    int capacity, int S, int C, float scale, hipStream_t s);
int pdt_attn_decode_combine(const float* o_part, const float* ml_part, uint16_t* out, float* lse, int B, int H, int S,
                            hipStream_t s);

// kernels/batchnorm.hip
int64_t pdt_bn_workspace_floats(int64_t M, int C);
void pdt_bn_tiles_fused(int on);
int pdt_bn_tune(int variant, int target_blocks, int u_fwd, int u_bwd);
int pdt_bn_fwd_train(const uint16_t* x, const uint16_t* res, const float* res_a, const float* res_b,
                     const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, int64_t M, int C, int relu, uint16_t* y, uint8_t* mask, float* mean, float* invstd,
                     float* ws, unsigned* counters, hipStream_t s);
int64_t pdt_bn_tiles_ws_floats(int T, int C);
int pdt_bn_fwd_train_tiles(const float* part, int T, int BMt, const uint16_t* x, const uint16_t* res,
                           const float* res_a, const float* res_b, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, int64_t M, int C,
                           int relu, uint16_t* y, uint8_t* mask, float* mean, float* invstd, float* ws, hipStream_t s,
                           uint16_t* sub_y, int sub_H, int sub_W, int sub_s);
int pdt_bn_relu_maxpool_fwd_train(const uint16_t* x, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float momentum, float eps, int N, int H, int W, int C,
                                  uint16_t* y, uint8_t* code, float* mean, float* invstd, float* ws,
                                  unsigned* counters, hipStream_t s);
int64_t pdt_bn_parts_ws_floats(int P, int C);
int pdt_bn_relu_maxpool_fwd_train_parts(const float* part, int P, const uint16_t* x, const float* gamma,
                                        const float* beta, float* running_mean, float* running_var, float momentum,
                                        float eps, int N, int H, int W, int C, uint16_t* y, uint8_t* code,
                                        float* mean, float* invstd, float* ws, hipStream_t s);
int pdt_maxpool3s2_bwd(const uint16_t* dy, const uint8_t* code, uint16_t* dz, int N, int H, int W, int C,
                       hipStream_t s);
int pdt_bn_fwd_eval(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta,
                    const float* running_mean, const float* running_var, float eps, int64_t M, int C, int relu,
                    uint16_t* y, float* ws, hipStream_t s);
int pdt_bn_bwd_train(const uint16_t* dy, const uint16_t* x, const uint8_t* mask, const float* gamma,
                     const float* mean, const float* invstd, int64_t M, int C, int relu, int has_res, uint16_t* dx,
                     uint16_t* dres, float* dgamma, float* dbeta, float* ws, unsigned* counters, hipStream_t s);
int pdt_bn_bwd_coef(const uint16_t* dy, const uint16_t* x, const uint8_t* mask, const float* gamma, const float* mean,
                    const float* invstd, int64_t M, int C, int relu, float* coef, float* dgamma, float* dbeta,
                    float* ws, unsigned* counters, hipStream_t s);
int pdt_bn_bwd_coef_tiles(const float* part, int T, const float* gamma, const float* invstd, int64_t M, int C,
                          float* coef, float* dgamma, float* dbeta, float* ws, hipStream_t s);
int pdt_bn_bwd_train_tiles(const float* part, int T, int BMt, const uint16_t* dy, const uint16_t* x,
                           const uint8_t* mask, const float* gamma, const float* mean, const float* invstd, int64_t M,
                           int C, int relu, int has_res, uint16_t* dx, uint16_t* dres, float* dgamma, float* dbeta,
                           float* ws, hipStream_t s);
int pdt_gap_bwd_parts(int64_t M, int C);
int pdt_gap_bwd(const uint16_t* g, int N, int HW, int C, uint16_t* dy, const uint16_t* xb, const uint8_t* mask,
                const float* mean, float* part, hipStream_t s);
void pdt_maxpool_bwd_v2(int on);
void pdt_pool_fwd_contig(int on);
void pdt_bn_row_wgs(int n);
void pdt_bn_apply_wgs(int n);
int pdt_maxpool_bn_parts(int N, int H);
int pdt_maxpool3s2_bwd_bn(const uint16_t* dy, const uint8_t* code, uint16_t* dz, int N, int H, int W, int C,
                          const uint16_t* x, const float* gamma, const float* mean, const float* invstd, uint16_t* dx,
                          float* dgamma, float* dbeta, float* part, float* ws, hipStream_t s);
int pdt_maxpool3s2_bwd_bn_coef(const uint16_t* dy, const uint8_t* code, uint16_t* dz, int N, int H, int W, int C,
                               const uint16_t* x, const float* gamma, const float* mean, const float* invstd,
                               float* coef, float* dgamma, float* dbeta, float* part, float* ws, hipStream_t s);
int pdt_bn_sync_fwd_stats(const uint16_t* x, int64_t M, int C, float* stats, float* count, float* ws,
                          unsigned* counters, hipStream_t s);
int pdt_bn_sync_fwd_merge(const float* gathered, int W, int C, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, float* mean,
                          float* invstd, float* ab, int64_t* ntot, hipStream_t s);
int pdt_bn_apply_coef(const uint16_t* x, const uint16_t* res, const float* ab, int64_t M, int C, int relu,
                      uint16_t* y, uint8_t* mask, hipStream_t s);
int pdt_bn_sync_bwd_sums(const uint16_t* dy, const uint16_t* x, const uint8_t* mask, const float* mean, int64_t M,
                         int C, int relu, float* sums, float* ws, unsigned* counters, hipStream_t s);
int pdt_bn_sync_bwd_merge(const float* gathered, int W, int rank, int C, const float* gamma, const float* invstd,
                          const int64_t* ntot, float* coef, float* dgamma, float* dbeta, hipStream_t s);
int pdt_bn_bwd_apply_coef(const uint16_t* dy, const uint16_t* x, const uint8_t* mask, const float* mean,
                          const float* coef, int64_t M, int C, int relu, int has_res, uint16_t* dx, uint16_t* dres,
                          hipStream_t s);

// kernels/bn_alg.hip
int pdt_bn_alg_fix_s2(float* part, int T, const float* wg, const uint16_t* W, int C4, int CW, hipStream_t s);
int pdt_bn_alg_ds_part(float* part, const float* s1, const float* mean, const float* wg, const uint16_t* W, int C4,
                       int CW, hipStream_t s);
int pdt_bn_alg_small_gemm(const uint16_t* W, const uint16_t* Wt, const float* coef, const float* wg, float* G,
                          float* BWG, int C4, int CW, hipStream_t s);
int pdt_bn_alg_assemble(const uint16_t* W, const float* coef, const float* mean, const float* G, const float* wg,
                        const float* BWG, uint16_t* bcat, uint16_t* dW, int C4, int CW, int rep, hipStream_t s);

// kernels/conv1x1.hip
int pdt_conv1x1_tile_rows();
void pdt_conv1x1_probe(int probe);
int pdt_conv1x1_persist(int mode);
int pdt_conv1x1_last_persistent();
int pdt_conv1x1_gemm(const uint16_t* a, const uint16_t* b, uint16_t* y, const uint16_t* c, const uint8_t* cm,
                     float* part, int M, int K, int N, const uint16_t* bn_x, const uint8_t* bn_mask,
                     const float* bn_mean, float* bn_part, int c_s, int c_H, int c_W, const float* acoef,
                     hipStream_t s, int nostore);
int pdt_conv1x1_gemm_seg(const uint16_t* a1, int k1, const uint16_t* a2, int k2, int rep2, const uint16_t* b,
                         uint16_t* y, int M, int N, const uint16_t* bn_x, const uint8_t* bn_mask,
                         const float* bn_mean, float* bn_part, hipStream_t s);
int pdt_conv1x1_gemm_apply(const uint16_t* a, const uint16_t* b, uint16_t* y, const uint16_t* res, const float* ab,
                           const float* rab, uint8_t* mask, int M, int K, int N, const float* acoef, hipStream_t s);

// kernels/conv1x1_bwd_fused.hip
int pdt_conv1x1_bwd_fused_ok(int C4, int CW);
int pdt_conv1x1_bwd_fused_grid(int M, int C4, int CW);
int pdt_conv1x1_bwd_fused(const uint16_t* dy, const uint16_t* z, const uint8_t* mz, const float* mean, const float* A,
                          const float* B, const float* D, const uint16_t* wt, const uint16_t* xa, const uint16_t* bx,
                          const uint8_t* bm, const float* bmean, float* bpart, const float* xcoef, uint8_t* mask_out,
                          uint16_t* dxa, uint16_t* dw, float* ws, int M, int C4, int CW, hipStream_t s);
void pdt_conv1x1_bwd_fused_tune(int grid);

// kernels/conv1x1_wgrad.hip
int64_t pdt_conv1x1_wgrad_ws_floats(int M, int Ci, int Co, int* nsplit_out);
int pdt_conv1x1_wgrad(const uint16_t* x, const uint16_t* dy, uint16_t* dw, float* ws, int M, int Ci, int Co,
                      hipStream_t s);
int64_t pdt_conv1x1_wgrad_seg_ws_floats(int M, int Ci, int co1, int co2, int* rows_out);
int pdt_conv1x1_wgrad_seg(const uint16_t* x, const uint16_t* dy1, int co1, const uint16_t* dy2, int co2, float* out,
                          float* ws, int M, int Ci, hipStream_t s);
void pdt_conv1x1_wgrad_tune(int target_wgs, int variant, int interleave);

// kernels/conv3x3.hip
// the stride-1 forward kernels, as pdt_conv3x3s1_variant names them: per-tap staging (128 / 64 channels wide),
// halo staging (128 / 64), weight-stationary 64 -> 64, row-tile 64 -> 64 at W = 56
enum { PDT_C3_TAP_WIDE = 0, PDT_C3_TAP_NARROW, PDT_C3_HALO_WIDE, PDT_C3_HALO_NARROW, PDT_C3_WST, PDT_C3_WSR };
int pdt_conv3x3s1_variant(int N, int H, int W, int Ci, int Co);
int pdt_conv3x3s1_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, int N, int H, int W, int Ci, int Co,
                      hipStream_t s);
int pdt_conv3x3s1_stats_tile_rows(int N, int H, int W, int Ci, int Co);
int pdt_conv3x3s1_bnbwd_tile_rows(int N, int H, int W, int Ci, int Co);
int pdt_conv3x3s1_fwd_stats(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int N, int H, int W,
                            int Ci, int Co, hipStream_t s);
int pdt_conv3x3s1_fwd_bnbwd(const uint16_t* x, const uint16_t* w, uint16_t* y, const uint16_t* bn_x,
                            const uint8_t* bn_mask, const float* bn_mean, float* bn_part, int N, int H, int W, int Ci,
                            int Co, hipStream_t s);
int pdt_conv3x3_opt(int v);
int pdt_conv3x3_flip_weights(const uint16_t* w, uint16_t* wf, int Co, int Ci, hipStream_t s);

// kernels/conv3x3_s2.hip
int pdt_conv3x3s2_tile_rows();
int pdt_conv3x3s2_dgrad_tiles(int N, int H, int W);
int pdt_conv3x3s2_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int N, int H, int W, int Ci,
                      int Co, hipStream_t s);
int pdt_conv3x3s2_dgrad(const uint16_t* dy, const uint16_t* wf, uint16_t* dx, const uint16_t* bn_x,
                        const uint8_t* bn_mask, const float* bn_mean, float* bn_part, int N, int H, int W, int Ci,
                        int Co, hipStream_t s);

// kernels/conv3x3_wgrad.hip
int64_t pdt_conv3x3_wgrad_ws_floats(int N, int H, int W, int Ci, int Co, int* nsplit_out);
int pdt_conv3x3s1_wgrad(const uint16_t* x, const uint16_t* dy, uint16_t* dw, float* ws, int N, int H, int W, int Ci,
                        int Co, hipStream_t s);
int64_t pdt_conv3x3s2_wgrad_ws_floats(int N, int H, int W, int Ci, int Co, int* nsplit_out);
int pdt_conv3x3s2_wgrad(const uint16_t* x, const uint16_t* dy, uint16_t* dw, float* ws, int N, int H, int W, int Ci,
                        int Co, hipStream_t s);
int pdt_conv3x3_wgrad_geo(int N, int H, int W, int Ci, int Co, int stride, int* geo5);
void pdt_conv3x3_wgrad_probe(int probe);
void pdt_conv3x3_wgrad_tune(int target_wgs, int co_tile);

// kernels/conv_stem.hip
int64_t pdt_stem_conv_wprep_elems();
int pdt_stem_conv_fwd(const uint16_t* x, const uint16_t* w, uint16_t* wp, uint16_t* y, int N, int H, int W,
                      hipStream_t s);
int64_t pdt_stem_stats_parts(int N, int H, int W);
int pdt_stem_conv_fwd_stats(const uint16_t* x, const uint16_t* w, uint16_t* wp, uint16_t* y, float* part, int N,
                            int H, int W, hipStream_t s);
int64_t pdt_stem_wgrad_ws_floats();
int pdt_stem_conv_wgrad(const uint16_t* x, const uint16_t* dy, uint16_t* dw, float* ws, int N, int H, int W,
                        hipStream_t s);
int pdt_stem_conv_wgrad_bn(const uint16_t* x, const uint16_t* dz, const uint16_t* xb, const float* coef,
                           const float* mean, uint16_t* dw, float* ws, int N, int H, int W, hipStream_t s);
int pdt_stem_conv_wgrad_bn_pool(const uint16_t* x, const uint16_t* dyp, const uint8_t* code, const uint16_t* xb,
                                const float* coef, const float* mean, uint16_t* dw, float* ws, int N, int H, int W,
                                hipStream_t s);

// kernels/dropout.hip
int pdt_dropout_begin(int64_t* state, int64_t* ticket, hipStream_t s);
int pdt_dropout(const void* x, void* y, int dtype, int64_t n, const int64_t* ticket, int stream, int thr,
                hipStream_t s);
int pdt_dropout_mask_flat(uint8_t* out, int64_t n, const int64_t* ticket, int stream, int thr, hipStream_t s);
int pdt_dropout_mask_attn(uint8_t* out, int64_t BH, int T, const int64_t* ticket, int stream, int thr, hipStream_t s);

// kernels/embedding.hip
int pdt_embedding_fwd(const int64_t* idx, const uint16_t* wte, const uint16_t* wpe, uint16_t* out, int64_t n, int T,
                      int D, int V, int* err, hipStream_t s);
int64_t pdt_embedding_bwd_ws_ints(int64_t n, int V);
int pdt_embedding_bwd(const int64_t* idx, const uint16_t* dout, uint16_t* dwte, uint16_t* dwpe, int* ws, int64_t n,
                      int B, int T, int V, int D, int* err, hipStream_t s);

// kernels/fp8.hip
int pdt_fp8_cast_transpose(const uint16_t* x, int64_t M, int64_t K, const float* scale, uint8_t* out, uint8_t* out_t,
                           float* amax, int striped, hipStream_t s);
int64_t pdt_fp8_gelu_cast_workspace_floats(int64_t M, int D);
int pdt_fp8_gelu_cast(const uint16_t* h, const uint16_t* dg, const float* bias, int64_t M, int D, int tanh_form,
                      const float* scale, uint8_t* out, uint8_t* out_t, float* amax, float* part, int striped,
                      hipStream_t s);
int pdt_fp8_cast_colsum(const uint16_t* x, int64_t M, int D, const float* scale, uint8_t* out, uint8_t* out_t,
                        float* amax, float* part, int striped, hipStream_t s);
int pdt_fp8_swiglu_cast(const uint16_t* gu, const uint16_t* dy, int64_t M, int F, const float* scale, uint8_t* out,
                        uint8_t* out_t, float* amax, int striped, hipStream_t s);
int pdt_fp8_cast_multi(int n, const uint16_t* const* x, const int* M, const int* K, float* const* st,
                       const int* striped, uint8_t* const* out, uint8_t* const* out_t, hipStream_t s);
int pdt_fp8_update_scales(float* state, int n, int L, float margin_scale, int striped, hipStream_t s);

// kernels/gelu.hip
int64_t pdt_gelu_workspace_floats(int64_t N, int D);
int pdt_bias_gelu_fwd(const void* x, int dtype, const void* bias, void* y, int64_t N, int D, int tanh_form,
                      hipStream_t s, int bias_bf16);
int pdt_bias_gelu_bwd(const void* dy, const void* x, int dtype, const void* bias, void* dx, void* dbias, int64_t N,
                      int D, int tanh_form, float* ws, hipStream_t s, int bias_bf16);
int pdt_colsum_finalize(const float* part, int nblk, int D, void* out, int odtype, hipStream_t s);
int pdt_colsum(const void* x, int dtype, int64_t N, int D, void* out, int odtype, float* ws, hipStream_t s);

// kernels/gemm.hip
int pdt_gemm_nt(const uint16_t* A, const uint16_t* B, uint16_t* C, uint16_t* G, const void* bias, int bias_f32,
                int epi, int tanh_form, int M, int N, int K, hipStream_t s);
int pdt_gemm_nt_tile_n(int M, int N);
int pdt_gemm_nt_fp8_ksplit(int M, int N, int K);
int pdt_gemm_nt_fp8(const uint8_t* A, const uint8_t* B, uint16_t* C, const float* sa, const float* sb,
                    const void* bias, int bias_f32, int epi, int M, int N, int K, float* ws, int ksplit,
                    hipStream_t s);

// kernels/layernorm.hip
int64_t pdt_ln_workspace_floats(int64_t N, int D);
int pdt_ln_fwd(const void* x, const void* res, int dtype, const float* w, const float* b, void* y, void* sum_out,
               float* mean, float* rstd, int64_t N, int D, float eps, hipStream_t s);
int pdt_ln_fwd_fp8(const uint16_t* x, const uint16_t* res, const float* w, const float* b, uint16_t* sum_out,
                   uint8_t* yq, uint8_t* yqt, float* mean, float* rstd, int64_t N, int D, float eps,
                   const float* scale, float* amax, int striped, hipStream_t s);
int pdt_ln_fwd_drop(const void* x, const void* res, int dtype, const float* w, const float* b, void* y, void* sum_out,
                    float* mean, float* rstd, int64_t N, int D, float eps, const int64_t* ticket, int dstream,
                    int thr, hipStream_t s);
int pdt_ln_bwd(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* mean,
               const float* rstd, void* dx, float* dw, float* db, int64_t N, int D, float* ws, hipStream_t s);
int pdt_ln_bwd_drop(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* mean,
                    const float* rstd, void* dx, void* dh, float* dw, float* db, int64_t N, int D, float* ws,
                    const int64_t* ticket, int dstream, int thr, hipStream_t s);

// kernels/layerwise.hip
int64_t pdt_layerwise_chunks(int n, const int64_t* numel);
int pdt_lars(int n, void* const* p, void* const* g, void* const* buf, void* const* copy, const int64_t* numel,
             int p_dtype, int g_dtype, float lr, const float* lr_ptr, float momentum, float dampening, float wd,
             int nesterov, int first, float tc, float eps, int maximize, const float* inv_scale,
             const float* found_inf, float* partials, double* sums, float* ratio, int norms_only, hipStream_t s);
int pdt_lamb(int n, void* const* p, void* const* g, void* const* m, void* const* v, void* const* copy,
             const int64_t* numel, int p_dtype, int g_dtype, float lr, const float* lr_ptr, float beta1, float beta2,
             float eps, float wd, const float* step_ptr, float step_host, int maximize, const float* inv_scale,
             const float* found_inf, float* partials, double* sums, float* ratio, int norms_only, hipStream_t s);

// kernels/lenet.hip
int pdt_mean_small(const float* v, int64_t n, float scale, float* out, hipStream_t s);
int pdt_lenet_stem_fwd(const float* x, const float* w, const float* b, int64_t N, float slope, float* y,
                       uint8_t* code, hipStream_t s);
int64_t pdt_lenet_stem_slab_floats(int64_t N, int ipb);
int pdt_lenet_stem_bwd(const float* dy, const uint8_t* code, const float* x, int64_t N, int ipb, float slope,
                       float* slab, float* dw, float* db, hipStream_t s);
int pdt_leaky_pool_fwd(const float* x, int64_t planes, int H, int W, float slope, float* y, uint8_t* code,
                       hipStream_t s);
int pdt_leaky_pool_bwd(const float* dy, const uint8_t* code, int64_t planes, int H, int W, float slope, float* dx,
                       hipStream_t s);
int pdt_softmax_nll_small(const void* logits, int dtype, const int64_t* target, int64_t N, int V, int mode,
                          float smoothing, float* loss, void* dlogits, float dscale, double* acc, hipStream_t s);

// kernels/lenet_tail.hip
int pdt_lenet_tail_fwd(const float* p1, const float* w2, const float* b2, const float* w3, const float* b3,
                       const float* fw1, const float* fb1, const float* fw2, const float* fb2, float slope, int N,
                       float* logits, uint8_t* code2, float* p2, float* h3, float* h4, hipStream_t s);
int64_t pdt_lenet_tail_ws_floats(int N);
int pdt_lenet_tail_bwd(const float* dl, const float* p1, const float* w2, const float* b2, const float* w3,
                       const float* b3, const float* fw1, const float* fb1, const float* fw2, const float* fb2,
                       float slope, int N, const uint8_t* code2, const float* p2, const float* h3, const float* h4,
                       float* ws, float* dp1, float* dw2, float* db2, float* dw3, float* db3, float* dfw1,
                       float* dfb1, float* dfw2, float* dfb2, hipStream_t s);

// kernels/optim.hip
int pdt_sgd(int n, void* const* p, void* const* g, void* const* buf, void* const* copy, const int64_t* numel,
            int p_dtype, int g_dtype, float lr, const float* lr_ptr, float momentum, float dampening, float wd,
            int nesterov, int first, int maximize, const float* inv_scale, const float* found_inf, hipStream_t s);
int pdt_adam(int n, void* const* p, void* const* g, void* const* m, void* const* v, void* const* copy,
             const int64_t* numel, int p_dtype, int g_dtype, float lr, const float* lr_ptr, float beta1, float beta2,
             float eps, float wd, int decoupled, const float* step_ptr, float step_host, int maximize,
             const float* inv_scale, const float* found_inf, hipStream_t s);
int pdt_adadelta(int n, void* const* p, void* const* g, void* const* sa, void* const* ad, void* const* copy,
                 const int64_t* numel, int p_dtype, int g_dtype, float lr, const float* lr_ptr, float rho, float eps,
                 float wd, int maximize, const float* inv_scale, const float* found_inf, hipStream_t s);

// kernels/p2p.hip
int64_t pdt_p2p_flags_bytes();
int64_t pdt_p2p_data_bytes(int64_t cap);
int pdt_p2p_allreduce(const void* in, void* out, int64_t n, int dtype, char* const* data_ptrs,
                      uint32_t* const* flag_ptrs, int rank, int world, int64_t cap, float post_scale, uint32_t* st,
                      int algo, int max_blocks, double timeout_s, hipStream_t s);

// kernels/rmsnorm.hip
int64_t pdt_rms_workspace_floats(int64_t N, int D);
int pdt_rms_fwd(const void* x, const void* res, int dtype, const float* w, void* y, void* sum_out, float* rstd,
                int64_t N, int D, float eps, hipStream_t s);
int pdt_rms_fwd_fp8(const uint16_t* x, const uint16_t* res, const float* w, uint16_t* sum_out, uint8_t* yq,
                    uint8_t* yqt, float* rstd, int64_t N, int D, float eps, const float* scale, float* amax,
                    int striped, hipStream_t s);
int pdt_rms_bwd(const void* dy, const void* x, const void* dres, int dtype, const float* w, const float* rstd,
                void* dx, float* dw, int64_t N, int D, float* ws, hipStream_t s);

// kernels/rope.hip
int pdt_rope_qkv(uint16_t* qkv, const float* cos, const float* sin, int B, int T, int H, int conj, hipStream_t s);
int pdt_rope_qkv_gqa(uint16_t* qkv, const float* cos, const float* sin, int B, int T, int H, int Hkv, int conj,
                     hipStream_t s);

// kernels/slice_sum.hip
int pdt_slice_sum_bf16(const uint16_t* x, uint16_t* out, int S, int64_t n, hipStream_t s);

// kernels/softmax_ce.hip
int pdt_ce_fwd(const void* logits, int dtype, const int64_t* target, int64_t N, int64_t V, float smoothing,
               int64_t ignore_index, float* loss, float* lse, hipStream_t s);
int pdt_ce_bwd(const void* logits, int dtype, const int64_t* target, const float* lse, const float* dloss,
               float dloss_scale, int64_t N, int64_t V, float smoothing, int64_t ignore_index, void* dlogits,
               hipStream_t s);

// kernels/subsample.hip
int pdt_subsample_gather(const uint16_t* x, uint16_t* xs, int N, int H, int W, int C, int s, hipStream_t st);
int pdt_subsample_scatter_add(const uint16_t* t, uint16_t* full, int N, int H, int W, int C, int s, hipStream_t st);

// kernels/swiglu.hip
int pdt_swiglu_fwd(const void* gu, int dtype, void* y, int64_t N, int F, hipStream_t s);
int pdt_swiglu_bwd(const void* dy, const void* gu, int dtype, void* dgu, int64_t N, int F, hipStream_t s);

// kernels/weight_prep.hip
int pdt_weight_prep_max_items();
int pdt_weight_prep(const uint16_t* const* src, uint16_t* const* dst, const int* R, const int* C, const int* taps,
                    int n, hipStream_t s);

}  // extern "C"
