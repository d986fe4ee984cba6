// Python binding for the gfx950 kernels (pybind11 over at::Tensor).
//
// Thin by design: validates devices / dtypes / layouts, collects raw pointers, and calls the
// C-ABI launchers in kernels/*.hip on the current HIP stream (so the calls are ordered with
// PyTorch's own kernels and can be captured into a hipGraph). Every kernel lives in its own
// .hip translation unit; this file is the only one that includes the PyTorch headers.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstring>
#include <map>
#include <vector>

#include "fp8_pack.h"
#include "launchers.h"

namespace {

using at::Tensor;

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

int dcode(const Tensor& t) {
  if (t.scalar_type() == at::kFloat) return 0;
  if (t.scalar_type() == at::kBFloat16) return 1;
  TORCH_CHECK(false, "pdt: unsupported dtype ", t.scalar_type(), " (fp32 / bf16 only)");
}

void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "pdt: ", name, " must be a GPU tensor");
}

bool dense(const Tensor& t) { return t.is_contiguous() || t.is_non_overlapping_and_dense(); }

// ----------------------------------------------------------------------------- checks and pointer accessors
// The vocabulary every binding below is written in. A binding reads: checks, allocate, pdt_x(...), check rc.
bool has(const c10::optional<Tensor>& t) { return t.has_value() && t->defined(); }

// The only casts of a tensor's storage to the launchers' element types: bf16 travels as uint16_t, fp8 and
// bool as uint8_t. bf16_ptr for operands, bf16_out for results.
uint16_t* bf16_out(const Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); }
const uint16_t* bf16_ptr(const Tensor& t) { return bf16_out(t); }
uint8_t* byte_ptr(const Tensor& t) { return static_cast<uint8_t*>(t.data_ptr()); }

// An optional output (allocated or left undefined by the binding): its pointer, or nullptr.
template <class T>
T* ptr_or_null(const Tensor& t) {
  return t.defined() ? t.data_ptr<T>() : nullptr;
}
template <>
uint16_t* ptr_or_null<uint16_t>(const Tensor& t) {
  return t.defined() ? bf16_out(t) : nullptr;
}

// An op's name, for the error text, and the device of its first tensor: every tensor whose raw pointer
// goes to the launcher has to live there (the launch runs on that device's current stream).
struct Op {
  const char* name;
  c10::Device dev;
  Op(const char* name, const Tensor& first) : name(name), dev(first.device()) {
    TORCH_CHECK(first.is_cuda(), name, ": the first tensor must be a GPU tensor");
  }
};

void check_flat(const Op& op, const char* name, const Tensor& t, at::ScalarType dtype, int64_t numel) {
  TORCH_CHECK(t.defined() && t.scalar_type() == dtype && t.is_contiguous() && t.numel() == numel &&
                  t.device() == op.dev,
              op.name, ": ", name, " must be a contiguous ", dtype, " tensor of ", numel, " elements on ", op.dev);
}

float* f32_ptr(const Op& op, const char* name, const Tensor& t, int64_t numel) {
  check_flat(op, name, t, at::kFloat, numel);
  return t.data_ptr<float>();
}
uint8_t* u8_ptr(const Op& op, const char* name, const Tensor& t, int64_t numel) {
  check_flat(op, name, t, at::kByte, numel);
  return t.data_ptr<uint8_t>();
}
float* opt_f32_ptr(const Op& op, const char* name, const c10::optional<Tensor>& t, int64_t numel) {
  return has(t) ? f32_ptr(op, name, *t, numel) : nullptr;
}
uint8_t* opt_u8_ptr(const Op& op, const char* name, const c10::optional<Tensor>& t, int64_t numel) {
  return has(t) ? u8_ptr(op, name, *t, numel) : nullptr;
}
// fp8 state rows (ops/fp8.py Fp8State) of at least pdt::kAmaxRowMin floats carry the 16 amax stripes.
int fp8_striped(const Tensor& row) { return row.numel() >= pdt::kAmaxRowMin ? 1 : 0; }
// A producer's fp8 state row (amax, scale, scale_inv, ...): its pointer; the scale is element 1.
float* fp8_row_ptr(const Op& op, const Tensor& row) {
  TORCH_CHECK(row.defined() && row.scalar_type() == at::kFloat && row.numel() >= 3 && row.is_contiguous() &&
                  row.device() == op.dev,
              op.name, ": state_row must be a contiguous fp32 row (amax, scale, scale_inv, ...) on ", op.dev);
  return row.data_ptr<float>();
}

// A device-side scalar (learning rate, loss scale, step count): the kernel reads element 0.
const float* opt_scalar_ptr(const Op& op, const char* name, const c10::optional<Tensor>& t) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() >= 1 && t->device() == op.dev, op.name, ": ", name,
              " must be an fp32 tensor on ", op.dev);
  return t->data_ptr<float>();
}

struct Lists {
  std::vector<void*> ptrs;
  static Lists from(const Op& op, const std::vector<Tensor>& ts, const char* name, int expect_dtype, size_t n) {
    Lists l;
    if (ts.empty()) {
      l.ptrs.assign(n, nullptr);
      return l;
    }
    TORCH_CHECK(ts.size() == n, "pdt: list ", name, " has ", ts.size(), " tensors, expected ", n);
    for (const auto& t : ts) {
      TORCH_CHECK(t.device() == op.dev, op.name, ": ", name, " tensors must be on ", op.dev);
      TORCH_CHECK(dense(t), "pdt: ", name, " tensors must be dense");
      if (expect_dtype >= 0) TORCH_CHECK(dcode(t) == expect_dtype, "pdt: ", name, " dtype mismatch");
      l.ptrs.push_back(t.data_ptr());
    }
    return l;
  }
};

std::vector<int64_t> numels(const std::vector<Tensor>& ts) {
  std::vector<int64_t> n;
  n.reserve(ts.size());
  for (const auto& t : ts) n.push_back(t.numel());
  return n;
}

void check_same_numel(const std::vector<Tensor>& a, const std::vector<Tensor>& b, const char* name) {
  if (b.empty()) return;
  for (size_t i = 0; i < a.size(); ++i)
    TORCH_CHECK(a[i].numel() == b[i].numel() && (a[i].strides() == b[i].strides() || a[i].is_contiguous() ==
                b[i].is_contiguous()), "pdt: ", name, "[", i, "] shape/layout mismatch");
}

int uniform_dtype(const std::vector<Tensor>& ts) {
  TORCH_CHECK(!ts.empty(), "pdt: empty tensor list");
  const int d = dcode(ts[0]);
  for (const auto& t : ts) TORCH_CHECK(dcode(t) == d, "pdt: mixed dtypes in one tensor list");
  return d;
}

// ----------------------------------------------------------------------------- optimizers
void sgd(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> bufs,
         std::vector<Tensor> copies, double lr, c10::optional<Tensor> lr_t, double momentum, double dampening,
         double wd, bool nesterov, bool first, bool maximize, c10::optional<Tensor> inv_scale,
         c10::optional<Tensor> found_inf) {
  if (params.empty()) return;
  const Op op("sgd", params[0]);
  const size_t n = params.size();
  const int pd = uniform_dtype(params), gd = uniform_dtype(grads);
  check_same_numel(params, grads, "grads");
  check_same_numel(params, bufs, "momentum_buffer");
  check_same_numel(params, copies, "model_copy");
  auto P = Lists::from(op, params, "params", pd, n), G = Lists::from(op, grads, "grads", gd, n),
       B = Lists::from(op, bufs, "momentum_buffer", 0, n), C = Lists::from(op, copies, "model_copy", 1, n);
  auto ne = numels(params);
  int rc = pdt_sgd((int)n, P.ptrs.data(), G.ptrs.data(), B.ptrs.data(), C.ptrs.data(), ne.data(), pd, gd, (float)lr,
                   opt_scalar_ptr(op, "lr_t", lr_t), (float)momentum, (float)dampening, (float)wd, nesterov, first,
                   maximize, opt_scalar_ptr(op, "inv_scale", inv_scale), opt_scalar_ptr(op, "found_inf", found_inf),
                   stream());
  TORCH_CHECK(rc == 0, "pdt_sgd failed");
}

void adam(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> exp_avg,
          std::vector<Tensor> exp_avg_sq, std::vector<Tensor> copies, double lr, c10::optional<Tensor> lr_t,
          double beta1, double beta2, double eps, double wd, bool decoupled, c10::optional<Tensor> step_t,
          double step, bool maximize, c10::optional<Tensor> inv_scale, c10::optional<Tensor> found_inf) {
  if (params.empty()) return;
  const Op op("adam", params[0]);
  const size_t n = params.size();
  const int pd = uniform_dtype(params), gd = uniform_dtype(grads);
  check_same_numel(params, grads, "grads");
  check_same_numel(params, exp_avg, "exp_avg");
  check_same_numel(params, exp_avg_sq, "exp_avg_sq");
  check_same_numel(params, copies, "model_copy");
  TORCH_CHECK(!exp_avg.empty() && !exp_avg_sq.empty(), "pdt_adam: states required");
  auto P = Lists::from(op, params, "params", pd, n), G = Lists::from(op, grads, "grads", gd, n),
       M = Lists::from(op, exp_avg, "exp_avg", 0, n), V = Lists::from(op, exp_avg_sq, "exp_avg_sq", 0, n),
       C = Lists::from(op, copies, "model_copy", 1, n);
  auto ne = numels(params);
  int rc = pdt_adam((int)n, P.ptrs.data(), G.ptrs.data(), M.ptrs.data(), V.ptrs.data(), C.ptrs.data(), ne.data(), pd,
                    gd, (float)lr, opt_scalar_ptr(op, "lr_t", lr_t), (float)beta1, (float)beta2, (float)eps, (float)wd,
                    decoupled, opt_scalar_ptr(op, "step_t", step_t), (float)step, maximize,
                    opt_scalar_ptr(op, "inv_scale", inv_scale), opt_scalar_ptr(op, "found_inf", found_inf), stream());
  TORCH_CHECK(rc == 0, "pdt_adam failed");
}

void adadelta(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> square_avg,
              std::vector<Tensor> acc_delta, std::vector<Tensor> copies, double lr, c10::optional<Tensor> lr_t,
              double rho, double eps, double wd, bool maximize, c10::optional<Tensor> inv_scale,
              c10::optional<Tensor> found_inf) {
  if (params.empty()) return;
  const Op op("adadelta", params[0]);
  const size_t n = params.size();
  const int pd = uniform_dtype(params), gd = uniform_dtype(grads);
  check_same_numel(params, grads, "grads");
  check_same_numel(params, square_avg, "square_avg");
  check_same_numel(params, acc_delta, "acc_delta");
  check_same_numel(params, copies, "model_copy");
  auto P = Lists::from(op, params, "params", pd, n), G = Lists::from(op, grads, "grads", gd, n),
       S = Lists::from(op, square_avg, "square_avg", 0, n), A = Lists::from(op, acc_delta, "acc_delta", 0, n),
       C = Lists::from(op, copies, "model_copy", 1, n);
  auto ne = numels(params);
  int rc = pdt_adadelta((int)n, P.ptrs.data(), G.ptrs.data(), S.ptrs.data(), A.ptrs.data(), C.ptrs.data(), ne.data(),
                        pd, gd, (float)lr, opt_scalar_ptr(op, "lr_t", lr_t), (float)rho, (float)eps, (float)wd,
                        maximize, opt_scalar_ptr(op, "inv_scale", inv_scale),
                        opt_scalar_ptr(op, "found_inf", found_inf), stream());
  TORCH_CHECK(rc == 0, "pdt_adadelta failed");
}

// Layer-wise optimizers (kernels/layerwise.hip). The scratch belongs to the caller and is allocated once:
// partials fp32 [>= 2 * layerwise_chunks(params)], sums fp64 [>= 2 n], ratio fp32 [>= n]; slot t belongs to
// params[t]. All three undefined: no trust ratio (r = 1), update pass only.
int64_t layerwise_chunks(std::vector<Tensor> params) {
  auto ne = numels(params);
  return pdt_layerwise_chunks((int)ne.size(), ne.data());
}

struct LayerwiseScratch {
  float* partials = nullptr;
  double* sums = nullptr;
  float* ratio = nullptr;
  LayerwiseScratch(const std::vector<Tensor>& params, const c10::optional<Tensor>& partials_t,
                   const c10::optional<Tensor>& sums_t, const c10::optional<Tensor>& ratio_t, bool norms_only) {
    for (const auto& p : params)
      TORCH_CHECK(p.numel() > 0, "pdt layerwise: zero-element parameters have no trust-ratio slot; leave them out");
    const bool given = has(ratio_t);
    TORCH_CHECK(given || !norms_only, "pdt layerwise: norms_only needs the scratch tensors");
    if (!given) return;
    TORCH_CHECK(has(partials_t) && has(sums_t), "pdt layerwise: partials, sums and ratio come together");
    const int64_t n = (int64_t)params.size();
    const auto dev = params[0].device();
    TORCH_CHECK(partials_t->is_cuda() && partials_t->device() == dev && partials_t->scalar_type() == at::kFloat &&
                    partials_t->is_contiguous() && partials_t->numel() >= 2 * layerwise_chunks(params),
                "pdt layerwise: partials must be fp32 [2 * chunks] on the parameters' device");
    TORCH_CHECK(sums_t->is_cuda() && sums_t->device() == dev && sums_t->scalar_type() == at::kDouble &&
                    sums_t->is_contiguous() && sums_t->numel() >= 2 * n,
                "pdt layerwise: sums must be fp64 [n, 2] on the parameters' device");
    TORCH_CHECK(ratio_t->is_cuda() && ratio_t->device() == dev && ratio_t->scalar_type() == at::kFloat &&
                    ratio_t->is_contiguous() && ratio_t->numel() >= n,
                "pdt layerwise: ratio must be fp32 [n] on the parameters' device");
    partials = partials_t->data_ptr<float>();
    sums = sums_t->data_ptr<double>();
    ratio = ratio_t->data_ptr<float>();
  }
};

void lars(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> bufs,
          std::vector<Tensor> copies, double lr, c10::optional<Tensor> lr_t, double momentum, double dampening,
          double wd, bool nesterov, bool first, double trust_coefficient, double eps, bool maximize,
          c10::optional<Tensor> inv_scale, c10::optional<Tensor> found_inf, c10::optional<Tensor> partials,
          c10::optional<Tensor> sums, c10::optional<Tensor> ratio, bool norms_only) {
  if (params.empty()) return;
  const Op op("lars", params[0]);
  const size_t n = params.size();
  const int pd = uniform_dtype(params), gd = uniform_dtype(grads);
  TORCH_CHECK(grads.size() == n, "pdt_lars: one gradient per parameter");
  check_same_numel(params, grads, "grads");
  check_same_numel(params, bufs, "momentum_buffer");
  check_same_numel(params, copies, "model_copy");
  auto P = Lists::from(op, params, "params", pd, n), G = Lists::from(op, grads, "grads", gd, n),
       B = Lists::from(op, bufs, "momentum_buffer", 0, n), C = Lists::from(op, copies, "model_copy", 1, n);
  LayerwiseScratch sc(params, partials, sums, ratio, norms_only);
  auto ne = numels(params);
  int rc = pdt_lars((int)n, P.ptrs.data(), G.ptrs.data(), B.ptrs.data(), C.ptrs.data(), ne.data(), pd, gd, (float)lr,
                    opt_scalar_ptr(op, "lr_t", lr_t), (float)momentum, (float)dampening, (float)wd, nesterov, first,
                    (float)trust_coefficient, (float)eps, maximize, opt_scalar_ptr(op, "inv_scale", inv_scale),
                    opt_scalar_ptr(op, "found_inf", found_inf), sc.partials, sc.sums, sc.ratio, norms_only, stream());
  TORCH_CHECK(rc == 0, "pdt_lars failed: ", rc);
}

void lamb(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> exp_avg,
          std::vector<Tensor> exp_avg_sq, std::vector<Tensor> copies, double lr, c10::optional<Tensor> lr_t,
          double beta1, double beta2, double eps, double wd, c10::optional<Tensor> step_t, double step,
          bool maximize, c10::optional<Tensor> inv_scale, c10::optional<Tensor> found_inf,
          c10::optional<Tensor> partials, c10::optional<Tensor> sums, c10::optional<Tensor> ratio, bool norms_only) {
  if (params.empty()) return;
  const Op op("lamb", params[0]);
  const size_t n = params.size();
  const int pd = uniform_dtype(params), gd = uniform_dtype(grads);
  TORCH_CHECK(grads.size() == n, "pdt_lamb: one gradient per parameter");
  TORCH_CHECK(exp_avg.size() == n && exp_avg_sq.size() == n, "pdt_lamb: states required");
  check_same_numel(params, grads, "grads");
  check_same_numel(params, exp_avg, "exp_avg");
  check_same_numel(params, exp_avg_sq, "exp_avg_sq");
  check_same_numel(params, copies, "model_copy");
  auto P = Lists::from(op, params, "params", pd, n), G = Lists::from(op, grads, "grads", gd, n),
       M = Lists::from(op, exp_avg, "exp_avg", 0, n), V = Lists::from(op, exp_avg_sq, "exp_avg_sq", 0, n),
       C = Lists::from(op, copies, "model_copy", 1, n);
  LayerwiseScratch sc(params, partials, sums, ratio, norms_only);
  auto ne = numels(params);
  int rc = pdt_lamb((int)n, P.ptrs.data(), G.ptrs.data(), M.ptrs.data(), V.ptrs.data(), C.ptrs.data(), ne.data(), pd,
                    gd, (float)lr, opt_scalar_ptr(op, "lr_t", lr_t), (float)beta1, (float)beta2, (float)eps, (float)wd,
                    opt_scalar_ptr(op, "step_t", step_t), (float)step, maximize,
                    opt_scalar_ptr(op, "inv_scale", inv_scale), opt_scalar_ptr(op, "found_inf", found_inf), sc.partials,
                    sc.sums, sc.ratio, norms_only, stream());
  TORCH_CHECK(rc == 0, "pdt_lamb failed: ", rc);
}

// ----------------------------------------------------------------------------- amp / buffers
void amp_unscale(std::vector<Tensor> grads, Tensor inv_scale, Tensor found_inf) {
  if (grads.empty()) return;
  const Op op("amp_unscale", grads[0]);
  const int d = uniform_dtype(grads);
  auto G = Lists::from(op, grads, "grads", d, grads.size());
  auto ne = numels(grads);
  TORCH_CHECK(pdt_amp_unscale((int)grads.size(), G.ptrs.data(), ne.data(), d, f32_ptr(op, "inv_scale", inv_scale, 1),
                              f32_ptr(op, "found_inf", found_inf, 1), stream()) == 0, "pdt_amp_unscale failed");
}

void amp_update(Tensor scale, Tensor growth_tracker, Tensor found_inf, double growth, double backoff, int64_t interval) {
  const Op op("amp_update", scale);
  TORCH_CHECK(growth_tracker.scalar_type() == at::kInt && growth_tracker.numel() == 1 &&
                  growth_tracker.device() == op.dev, "amp_update: growth_tracker must be int32 [1] on ", op.dev);
  pdt_amp_update(f32_ptr(op, "scale", scale, 1), growth_tracker.data_ptr<int>(), f32_ptr(op, "found_inf", found_inf, 1),
                 (float)growth, (float)backoff, (int)interval, stream());
}

void mt_scale(std::vector<Tensor> xs, c10::optional<Tensor> scale_t, double scale) {
  if (xs.empty()) return;
  const Op op("mt_scale", xs[0]);
  const int d = uniform_dtype(xs);
  auto X = Lists::from(op, xs, "x", d, xs.size());
  auto ne = numels(xs);
  TORCH_CHECK(pdt_mt_scale((int)xs.size(), X.ptrs.data(), ne.data(), d, opt_scalar_ptr(op, "scale_t", scale_t),
                           (float)scale, stream()) == 0, "pdt_mt_scale failed");
}

void mt_copy(std::vector<Tensor> src, std::vector<Tensor> dst, c10::optional<Tensor> scale_t, double scale) {
  if (src.empty()) return;
  const Op op("mt_copy", src[0]);
  TORCH_CHECK(src.size() == dst.size(), "mt_copy: list size mismatch");
  check_same_numel(src, dst, "dst");
  const int sd = uniform_dtype(src), dd = uniform_dtype(dst);
  auto S = Lists::from(op, src, "src", sd, src.size()), D = Lists::from(op, dst, "dst", dd, dst.size());
  auto ne = numels(src);
  TORCH_CHECK(pdt_mt_copy((int)src.size(), S.ptrs.data(), D.ptrs.data(), ne.data(), sd, dd,
                          opt_scalar_ptr(op, "scale_t", scale_t), (float)scale, stream()) == 0, "pdt_mt_copy failed");
}

void l2norm_sq(std::vector<Tensor> xs, Tensor out) {
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() >= 1, "l2norm_sq: out must be fp32");
  if (xs.empty()) {
    out.zero_();
    return;
  }
  const Op op("l2norm_sq", xs[0]);
  TORCH_CHECK(out.device() == op.dev, "l2norm_sq: out must be on ", op.dev);
  const int d = uniform_dtype(xs);
  auto X = Lists::from(op, xs, "x", d, xs.size());
  auto ne = numels(xs);
  pdt_l2norm_sq((int)xs.size(), X.ptrs.data(), ne.data(), d, out.data_ptr<float>(), stream());
}

void clip_coef(Tensor sumsq, double max_norm, Tensor coef, c10::optional<Tensor> norm) {
  const Op op("clip_coef", sumsq);
  pdt_clip_coef(f32_ptr(op, "sumsq", sumsq, 1), (float)max_norm, f32_ptr(op, "coef", coef, 1),
                opt_f32_ptr(op, "norm", norm, 1), stream());
}

// ----------------------------------------------------------------------------- batchnorm (NHWC bf16)
// A BatchNorm / conv activation: bf16 on the op's device, channels_last when 4-D, [M, C] contiguous when 2-D.
void check_nhwc_bf16(const Op& op, const char* name, const Tensor& t) {
  TORCH_CHECK(t.defined() && t.device() == op.dev && t.scalar_type() == at::kBFloat16, op.name, ": ", name,
              " must be a bf16 tensor on ", op.dev);
  if (t.dim() == 4) {
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), op.name, ": ", name, " must be channels_last");
  } else {
    TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), op.name, ": ", name, " must be [M, C] contiguous or NHWC");
  }
}

// The residual added by a BatchNorm over x (or nullptr): x's sizes and strides, so bf16 channels_last as x.
const uint16_t* residual_ptr(const Op& op, const Tensor& x, const c10::optional<Tensor>& res) {
  if (!has(res)) return nullptr;
  check_nhwc_bf16(op, "residual", *res);
  TORCH_CHECK(res->sizes() == x.sizes() && res->strides() == x.strides(), op.name, ": residual layout mismatch");
  return bf16_ptr(*res);
}

// The ReLU bit-mask [M C / 8] a BatchNorm backward with relu reads (nullptr without relu).
const uint8_t* relu_mask_ptr(const Op& op, const c10::optional<Tensor>& mask, bool relu, int64_t bytes) {
  if (!relu) return nullptr;
  TORCH_CHECK(has(mask), op.name, ": relu needs the mask");
  return u8_ptr(op, "mask", *mask, bytes);
}

// dgamma / dbeta fp32 [C] of a BatchNorm backward: allocated with need_dgamma, else undefined (null pointers).
struct GammaGrads {
  Tensor dg, db;
  GammaGrads(bool need_dgamma, int64_t C, const at::TensorOptions& fopt) {
    if (need_dgamma) {
      dg = at::empty({C}, fopt);
      db = at::empty({C}, fopt);
    }
  }
  float* dg_ptr() const { return ptr_or_null<float>(dg); }
  float* db_ptr() const { return ptr_or_null<float>(db); }
};

// bn_x / bn_mask / bn_mean of a producer op: its output [M, C] is the gradient at the output of a BatchNorm
// with input bn_x (bf16 [M, C] as check_nhwc_bf16), ReLU bit-mask bn_mask (uint8 [M C / 8], or none) and batch
// mean bn_mean (fp32 [C]), whose backward partials the producer accumulates. sum_only: bn_x is not read.
struct BnSide {
  const uint16_t* x = nullptr;
  const uint8_t* mask = nullptr;
  const float* mean = nullptr;
};
BnSide bn_side(const Op& op, const c10::optional<Tensor>& bn_x, const c10::optional<Tensor>& bn_mask,
               const c10::optional<Tensor>& bn_mean, int64_t M, int64_t C, bool sum_only) {
  BnSide s;
  if (!sum_only) {
    TORCH_CHECK(has(bn_x), op.name, ": bn_x is required");
    check_nhwc_bf16(op, "bn_x", *bn_x);
    TORCH_CHECK(bn_x->numel() == M * C, op.name, ": bn_x must be [M, C] = [", M, ", ", C, "]");
    s.x = bf16_ptr(*bn_x);
  }
  TORCH_CHECK(has(bn_mean), op.name, ": bn_mean is required with bn_x");
  s.mean = f32_ptr(op, "bn_mean", *bn_mean, C);
  s.mask = opt_u8_ptr(op, "bn_mask", bn_mask, M * C / 8);
  return s;
}

int64_t bn_ws_floats(int64_t M, int64_t C) { return pdt_bn_workspace_floats(M, (int)C); }

// Self-resetting arrival counters of the BN reduce kernels (one per 64-channel chunk), one
// buffer per device, zeroed once at creation (first call happens before any graph capture).
unsigned* bn_counters(const Tensor& like) {
  static std::map<int, Tensor> bufs;
  const int dev = like.get_device();
  auto it = bufs.find(dev);
  if (it == bufs.end()) {
    it = bufs.emplace(dev, at::zeros({4096}, like.options().dtype(at::kInt))).first;
  }
  return reinterpret_cast<unsigned*>(it->second.data_ptr<int>());
}

// res_ab [2, C] (optional): the residual is a deferred BatchNorm's input, added as ab[0]*res + ab[1].
// apply = false: statistics only -> {undefined, undefined, mean, invstd, ab [2, C]} (the y = a x + b
// coefficients, for a consumer that applies them itself).
std::vector<Tensor> bn_fwd_train(Tensor x, c10::optional<Tensor> res, c10::optional<Tensor> weight,
                                 c10::optional<Tensor> bias, c10::optional<Tensor> running_mean,
                                 c10::optional<Tensor> running_var, double momentum, double eps, bool relu,
                                 c10::optional<Tensor> res_ab, bool apply) {
  const Op op("bn_fwd_train", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  TORCH_CHECK(C % 64 == 0 && C <= 64 * 4096, "pdt bn: C must be a multiple of 64");
  const float* rab = opt_f32_ptr(op, "res_ab", res_ab, 2 * C);
  Tensor y;
  if (apply) y = at::empty_like(x);
  Tensor mask;
  if (relu && apply) mask = at::empty({M * C / 8}, x.options().dtype(at::kByte));
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt);
  auto ws = at::empty({bn_ws_floats(M, C)}, fopt);
  int rc = pdt_bn_fwd_train(bf16_ptr(x), residual_ptr(op, x, res), rab, rab ? rab + C : nullptr,
                            opt_f32_ptr(op, "weight", weight, C), opt_f32_ptr(op, "bias", bias, C),
                            opt_f32_ptr(op, "running_mean", running_mean, C),
                            opt_f32_ptr(op, "running_var", running_var, C), (float)momentum, (float)eps, M, (int)C,
                            relu, ptr_or_null<uint16_t>(y), ptr_or_null<uint8_t>(mask), mean.data_ptr<float>(),
                            invstd.data_ptr<float>(), ws.data_ptr<float>(), bn_counters(x), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_fwd_train failed: ", rc);
  if (!apply) return {Tensor(), Tensor(), mean, invstd, ws.narrow(0, bn_ws_floats(M, C) - 4 * C, 2 * C).view({2, C})};
  return {y, mask, mean, invstd};
}

// ResNet stem tail (train): BN + ReLU + MaxPool2d(3, 2, 1) -> {y_pooled, code, mean, invstd}
std::vector<Tensor> bn_relu_maxpool_fwd(Tensor x, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                                        c10::optional<Tensor> running_mean, c10::optional<Tensor> running_var,
                                        double momentum, double eps) {
  const Op op("bn_relu_maxpool_fwd", x);
  check_nhwc_bf16(op, "x", x);
  TORCH_CHECK(x.dim() == 4, "bn_relu_maxpool: 4-D NHWC input");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C % 64 == 0, "pdt bn: C must be a multiple of 64");
  const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  auto y = at::empty({N, C, Ho, Wo}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto code = at::empty({N * Ho * Wo * C}, x.options().dtype(at::kByte));
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt);
  auto ws = at::empty({bn_ws_floats(N * H * W, C)}, fopt);
  int rc = pdt_bn_relu_maxpool_fwd_train(bf16_ptr(x), opt_f32_ptr(op, "weight", weight, C),
                                         opt_f32_ptr(op, "bias", bias, C),
                                         opt_f32_ptr(op, "running_mean", running_mean, C),
                                         opt_f32_ptr(op, "running_var", running_var, C), (float)momentum, (float)eps,
                                         (int)N, (int)H, (int)W, (int)C, bf16_out(y), code.data_ptr<uint8_t>(),
                                         mean.data_ptr<float>(), invstd.data_ptr<float>(), ws.data_ptr<float>(),
                                         bn_counters(x), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_relu_maxpool_fwd_train failed");
  return {y, code, mean, invstd};
}

// The same with the statistics from stem_conv_fwd_stats's partials (no reduce pass over x).
std::vector<Tensor> bn_relu_maxpool_fwd_parts(Tensor x, Tensor part, c10::optional<Tensor> weight,
                                              c10::optional<Tensor> bias, c10::optional<Tensor> running_mean,
                                              c10::optional<Tensor> running_var, double momentum, double eps) {
  const Op op("bn_relu_maxpool_fwd_parts", x);
  check_nhwc_bf16(op, "x", x);
  TORCH_CHECK(x.dim() == 4, "bn_relu_maxpool: 4-D NHWC input");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C == 64, "bn_relu_maxpool_fwd_parts: C == 64 (the stem)");
  TORCH_CHECK(part.dim() == 1 && part.numel() % (2 * C + 1) == 0, "bn_relu_maxpool_fwd_parts: part [P * (2 C + 1)] f32");
  const int64_t P = part.numel() / (2 * C + 1);
  const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  auto y = at::empty({N, C, Ho, Wo}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto code = at::empty({N * Ho * Wo * C}, x.options().dtype(at::kByte));
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt);
  auto ws = at::empty({pdt_bn_parts_ws_floats((int)P, (int)C)}, fopt);
  int rc = pdt_bn_relu_maxpool_fwd_train_parts(f32_ptr(op, "part", part, P * (2 * C + 1)), (int)P, bf16_ptr(x),
                                               opt_f32_ptr(op, "weight", weight, C), opt_f32_ptr(op, "bias", bias, C),
                                               opt_f32_ptr(op, "running_mean", running_mean, C),
                                               opt_f32_ptr(op, "running_var", running_var, C), (float)momentum,
                                               (float)eps, (int)N, (int)H, (int)W, (int)C, bf16_out(y),
                                               code.data_ptr<uint8_t>(), mean.data_ptr<float>(),
                                               invstd.data_ptr<float>(), ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_relu_maxpool_fwd_train_parts failed: ", rc);
  return {y, code, mean, invstd};
}

// Global-average-pool gradient: g [N, C] bf16 -> dy [N, C, H, W] channels_last = g / (H W). With bn_x / bn_mask /
// bn_mean (the pooled tensor is a BatchNorm(+ReLU) output): also that BatchNorm's backward partials [2, T, C]
// (the input of bn_bwd_train_tiles); {dy} alone when the reduction does not apply to C.
std::vector<Tensor> gap_bwd(Tensor g, int64_t H, int64_t W, c10::optional<Tensor> bn_x, c10::optional<Tensor> bn_mask,
                            c10::optional<Tensor> bn_mean, bool bn_sum_only) {
  const Op op("gap_bwd", g);
  TORCH_CHECK(g.dim() == 2 && g.scalar_type() == at::kBFloat16 && g.is_contiguous() && g.size(1) % 8 == 0,
              "gap_bwd: g [N, C] contiguous bf16, C % 8 == 0");
  const int64_t N = g.size(0), C = g.size(1), M = N * H * W;
  auto dy = at::empty({N, C, H, W}, g.options().memory_format(at::MemoryFormat::ChannelsLast));
  const bool red = (has(bn_x) || bn_sum_only) && pdt_gap_bwd_parts(M, (int)C) > 0;
  Tensor part;
  BnSide bn;
  if (red) {
    bn = bn_side(op, bn_x, bn_mask, bn_mean, M, C, bn_sum_only);
    TORCH_CHECK(bn_sum_only || bn_x->sizes() == dy.sizes(), "gap_bwd: bn_x must be [N, C, H, W]");
    part = at::empty({2, pdt_gap_bwd_parts(M, (int)C), C}, g.options().dtype(at::kFloat));
  }
  const int rc = pdt_gap_bwd(bf16_ptr(g), (int)N, (int)(H * W), (int)C, bf16_out(dy), bn.x, bn.mask, bn.mean,
                             ptr_or_null<float>(part), stream());
  TORCH_CHECK(rc == 0, "pdt_gap_bwd failed: ", rc);
  if (red) return {dy, part};
  return {dy};
}

Tensor maxpool3s2_bwd(Tensor dy, Tensor code, int64_t H, int64_t W) {
  const Op op("maxpool3s2_bwd", dy);
  dy = dy.contiguous(at::MemoryFormat::ChannelsLast);
  check_nhwc_bf16(op, "dy", dy);
  const int64_t N = dy.size(0), C = dy.size(1);
  TORCH_CHECK(dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == (W - 1) / 2 + 1, "maxpool3s2_bwd: shape mismatch");
  auto dz = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  int rc = pdt_maxpool3s2_bwd(bf16_ptr(dy), u8_ptr(op, "code", code, dy.numel()), bf16_out(dz), (int)N, (int)H, (int)W,
                              (int)C, stream());
  TORCH_CHECK(rc == 0, "pdt_maxpool3s2_bwd failed");
  return dz;
}

Tensor bn_fwd_eval(Tensor x, c10::optional<Tensor> res, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                   Tensor running_mean, Tensor running_var, double eps, bool relu) {
  const Op op("bn_fwd_eval", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  auto y = at::empty_like(x);
  auto ws = at::empty({2 * C}, x.options().dtype(at::kFloat));
  int rc = pdt_bn_fwd_eval(bf16_ptr(x), residual_ptr(op, x, res), opt_f32_ptr(op, "weight", weight, C),
                           opt_f32_ptr(op, "bias", bias, C), f32_ptr(op, "running_mean", running_mean, C),
                           f32_ptr(op, "running_var", running_var, C), (float)eps, M, (int)C, relu, bf16_out(y),
                           ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_fwd_eval failed");
  return y;
}

std::vector<Tensor> bn_bwd_train(Tensor dy, Tensor x, c10::optional<Tensor> mask, c10::optional<Tensor> weight,
                                 Tensor mean, Tensor invstd, bool relu, bool has_res, bool need_dgamma) {
  const Op op("bn_bwd_train", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), "pdt bn bwd: dy layout mismatch");
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  TORCH_CHECK(C % 64 == 0, "pdt bn bwd: C must be a multiple of 64");
  auto dx = at::empty_like(x);
  Tensor dres;
  if (has_res) dres = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const GammaGrads gg(need_dgamma, C, fopt);
  auto ws = at::empty({bn_ws_floats(M, C)}, fopt);
  int rc = pdt_bn_bwd_train(bf16_ptr(dy), bf16_ptr(x), relu_mask_ptr(op, mask, relu, M * C / 8),
                            opt_f32_ptr(op, "weight", weight, C), f32_ptr(op, "mean", mean, C),
                            f32_ptr(op, "invstd", invstd, C), M, (int)C, relu, has_res, bf16_out(dx),
                            ptr_or_null<uint16_t>(dres), gg.dg_ptr(), gg.db_ptr(), ws.data_ptr<float>(), bn_counters(x),
                            stream());
  TORCH_CHECK(rc == 0, "pdt_bn_bwd_train failed");
  return {dx, dres, gg.dg, gg.db};
}

// ---- SyncBatchNorm (ops/sync_batchnorm.py): the train forward / backward split around the exchange.
// This rank's raw statistics [2, C] = (mean_r, M2_r = sum (x - mean_r)^2). row (optional, fp32 [2C + 1]): written
// in place as (mean_r, M2_r, M) — this rank's row of the exchange buffer — and returned.
Tensor bn_sync_fwd_stats(Tensor x, c10::optional<Tensor> row) {
  const Op op("bn_sync_fwd_stats", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 64 == 0 && C <= 64 * 4096 && x.numel() > 0, "pdt sync bn: C must be a multiple of 64, M >= 1");
  const int64_t M = x.numel() / C;
  auto fopt = x.options().dtype(at::kFloat);
  const bool in_row = has(row);
  if (in_row) TORCH_CHECK(M < (1 << 24), "pdt sync bn: the row count travels as fp32 (M < 2^24)");
  auto stats = in_row ? *row : at::empty({2, C}, fopt);
  float* sp = f32_ptr(op, "row", stats, in_row ? 2 * C + 1 : 2 * C);
  auto ws = at::empty({bn_ws_floats(M, C)}, fopt);
  const int rc = pdt_bn_sync_fwd_stats(bf16_ptr(x), M, (int)C, sp, in_row ? sp + 2 * C : nullptr, ws.data_ptr<float>(),
                                       bn_counters(x), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_sync_fwd_stats failed: ", rc);
  return stats;
}

// gathered [W, 2C + 1] (rank r: mean_r, M2_r, n_r) -> {mean, invstd, ab [2, C], ntot int64 [1]}; updates the
// running statistics.
std::vector<Tensor> bn_sync_fwd_merge(Tensor gathered, c10::optional<Tensor> weight, c10::optional<Tensor> bias,
                                      c10::optional<Tensor> running_mean, c10::optional<Tensor> running_var,
                                      double momentum, double eps) {
  const Op op("bn_sync_fwd_merge", gathered);
  TORCH_CHECK(gathered.dim() == 2 && gathered.size(0) >= 1 && gathered.size(1) % 2 == 1,
              "pdt sync bn: gathered must be [W, 2C + 1]");
  const int64_t W = gathered.size(0), C = (gathered.size(1) - 1) / 2;
  TORCH_CHECK(C >= 64 && C % 64 == 0, "pdt sync bn: C must be a multiple of 64");
  auto mean = at::empty({C}, gathered.options()), invstd = at::empty({C}, gathered.options());
  auto ab = at::empty({2, C}, gathered.options());
  auto ntot = at::empty({1}, gathered.options().dtype(at::kLong));
  const int rc = pdt_bn_sync_fwd_merge(f32_ptr(op, "gathered", gathered, W * (2 * C + 1)), (int)W, (int)C,
                                       opt_f32_ptr(op, "weight", weight, C), opt_f32_ptr(op, "bias", bias, C),
                                       opt_f32_ptr(op, "running_mean", running_mean, C),
                                       opt_f32_ptr(op, "running_var", running_var, C), (float)momentum, (float)eps,
                                       mean.data_ptr<float>(), invstd.data_ptr<float>(), ab.data_ptr<float>(),
                                       ntot.data_ptr<int64_t>(), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_sync_fwd_merge failed: ", rc);
  return {mean, invstd, ab, ntot};
}

// y = relu?(ab[0] x + ab[1] + res?) -> {y, mask (with relu)}.
std::vector<Tensor> bn_apply_coef(Tensor x, c10::optional<Tensor> res, Tensor ab, bool relu) {
  const Op op("bn_apply_coef", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 64 == 0 && x.numel() > 0, "pdt sync bn: C must be a multiple of 64, M >= 1");
  const int64_t M = x.numel() / C;
  auto y = at::empty_like(x);
  Tensor mask;
  if (relu) mask = at::empty({M * C / 8}, x.options().dtype(at::kByte));
  const int rc = pdt_bn_apply_coef(bf16_ptr(x), residual_ptr(op, x, res), f32_ptr(op, "ab", ab, 2 * C), M, (int)C, relu,
                                   bf16_out(y), ptr_or_null<uint8_t>(mask), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_apply_coef failed: ", rc);
  return {y, mask};
}

// This rank's raw backward sums [2, C] = (sum dz, sum dz (x - mean)), dz = dy * mask with relu.
// row (optional, fp32 [2C]): written in place (this rank's row of the exchange buffer) and returned.
Tensor bn_sync_bwd_sums(Tensor dy, Tensor x, c10::optional<Tensor> mask, Tensor mean, bool relu,
                        c10::optional<Tensor> row) {
  const Op op("bn_sync_bwd_sums", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), "pdt sync bn: dy layout mismatch");
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 64 == 0 && x.numel() > 0, "pdt sync bn: C must be a multiple of 64, M >= 1");
  const int64_t M = x.numel() / C;
  auto fopt = x.options().dtype(at::kFloat);
  auto sums = has(row) ? *row : at::empty({2, C}, fopt);
  auto ws = at::empty({bn_ws_floats(M, C)}, fopt);
  const int rc = pdt_bn_sync_bwd_sums(bf16_ptr(dy), bf16_ptr(x), relu_mask_ptr(op, mask, relu, M * C / 8),
                                      f32_ptr(op, "mean", mean, C), M, (int)C, relu, f32_ptr(op, "row", sums, 2 * C),
                                      ws.data_ptr<float>(), bn_counters(x), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_sync_bwd_sums failed: ", rc);
  return sums;
}

// gathered [W, 2C] (rank r: sum dz, sum dz (x - mean)) -> {coef [3, C] = A, B, D from all rows over ntot,
// dgamma, dbeta from row `rank` only (undefined without need_dgamma)}.
std::vector<Tensor> bn_sync_bwd_merge(Tensor gathered, int64_t rank, c10::optional<Tensor> weight, Tensor invstd,
                                      Tensor ntot, bool need_dgamma) {
  const Op op("bn_sync_bwd_merge", gathered);
  TORCH_CHECK(gathered.dim() == 2 && gathered.size(0) >= 1 && gathered.size(1) % 2 == 0,
              "pdt sync bn: gathered must be [W, 2C]");
  const int64_t W = gathered.size(0), C = gathered.size(1) / 2;
  TORCH_CHECK(C >= 64 && C % 64 == 0, "pdt sync bn: C must be a multiple of 64");
  TORCH_CHECK(rank >= 0 && rank < W, "pdt sync bn: rank ", rank, " outside [0, ", W, ")");
  TORCH_CHECK(ntot.device() == op.dev && ntot.scalar_type() == at::kLong && ntot.numel() == 1,
              "pdt sync bn: ntot int64 [1]");
  auto coef = at::empty({3, C}, gathered.options());
  const GammaGrads gg(need_dgamma, C, gathered.options());
  const int rc = pdt_bn_sync_bwd_merge(f32_ptr(op, "gathered", gathered, W * 2 * C), (int)W, (int)rank, (int)C,
                                       opt_f32_ptr(op, "weight", weight, C), f32_ptr(op, "invstd", invstd, C),
                                       ntot.data_ptr<int64_t>(), coef.data_ptr<float>(), gg.dg_ptr(), gg.db_ptr(),
                                       stream());
  TORCH_CHECK(rc == 0, "pdt_bn_sync_bwd_merge failed: ", rc);
  return {coef, gg.dg, gg.db};
}

// dx = A dz + B (x - mean) + D from coef [3, C] -> {dx, dres = dz (with has_res)}.
std::vector<Tensor> bn_bwd_apply_coef(Tensor dy, Tensor x, c10::optional<Tensor> mask, Tensor mean, Tensor coef,
                                      bool relu, bool has_res) {
  const Op op("bn_bwd_apply_coef", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), "pdt sync bn: dy layout mismatch");
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 64 == 0 && x.numel() > 0, "pdt sync bn: C must be a multiple of 64, M >= 1");
  const int64_t M = x.numel() / C;
  auto dx = at::empty_like(x);
  Tensor dres;
  if (has_res) dres = at::empty_like(x);
  const int rc = pdt_bn_bwd_apply_coef(bf16_ptr(dy), bf16_ptr(x), relu_mask_ptr(op, mask, relu, M * C / 8),
                                       f32_ptr(op, "mean", mean, C), f32_ptr(op, "coef", coef, 3 * C), M, (int)C, relu,
                                       has_res, bf16_out(dx), ptr_or_null<uint16_t>(dres), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_bwd_apply_coef failed: ", rc);
  return {dx, dres};
}

// ResNet stem backward: max-pool gradient (the BN's dz, never returned) with the stem BatchNorm's
// backward reduction fused in, then BN finalize + apply. x: the BN input [N,64,H,W] channels_last.
// Returns {dx, dgamma, dbeta}.
std::vector<Tensor> maxpool3s2_bwd_bn(Tensor dy, Tensor code, Tensor x, c10::optional<Tensor> weight, Tensor mean,
                                      Tensor invstd, bool need_dgamma) {
  const Op op("maxpool3s2_bwd_bn", dy);
  check_nhwc_bf16(op, "dy", dy);
  check_nhwc_bf16(op, "x", x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C == 64, "maxpool3s2_bwd_bn: C == 64");
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == C && dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == (W - 1) / 2 + 1,
              "maxpool3s2_bwd_bn: dy shape");
  auto dz = at::empty_like(x);
  auto dx = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const GammaGrads gg(need_dgamma, C, fopt);
  const int T = pdt_maxpool_bn_parts((int)N, (int)H);
  auto part = at::empty({2 * (int64_t)T * C}, fopt);
  auto ws = at::empty({pdt_bn_tiles_ws_floats(T, (int)C) + 2 * C}, fopt);
  const int rc = pdt_maxpool3s2_bwd_bn(bf16_ptr(dy), u8_ptr(op, "code", code, dy.numel()), bf16_out(dz), (int)N, (int)H,
                                       (int)W, (int)C, bf16_ptr(x), opt_f32_ptr(op, "weight", weight, C),
                                       f32_ptr(op, "mean", mean, C), f32_ptr(op, "invstd", invstd, C), bf16_out(dx),
                                       gg.dg_ptr(), gg.db_ptr(), part.data_ptr<float>(), ws.data_ptr<float>(),
                                       stream());
  TORCH_CHECK(rc == 0, "pdt_maxpool3s2_bwd_bn failed: ", rc);
  return {dx, gg.dg, gg.db};
}

// Same without the BN apply: returns {dz (the max-pool gradient = dy at the BN output), coef [3, 64]
// (A, B, D: dx = A dz + B (x - mean) + D), dgamma, dbeta} for stem_conv_wgrad_bn.
std::vector<Tensor> maxpool3s2_bwd_bn_coef(Tensor dy, Tensor code, Tensor x, c10::optional<Tensor> weight,
                                           Tensor mean, Tensor invstd, bool need_dgamma, bool write_dz) {
  const Op op("maxpool3s2_bwd_bn_coef", dy);
  check_nhwc_bf16(op, "dy", dy);
  check_nhwc_bf16(op, "x", x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C == 64, "maxpool3s2_bwd_bn_coef: C == 64");
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == C && dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == (W - 1) / 2 + 1,
              "maxpool3s2_bwd_bn_coef: dy shape");
  Tensor dz;
  if (write_dz) dz = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto coef = at::empty({3, C}, fopt);
  const GammaGrads gg(need_dgamma, C, fopt);
  const int T = pdt_maxpool_bn_parts((int)N, (int)H);
  auto part = at::empty({2 * (int64_t)T * C}, fopt);
  auto ws = at::empty({pdt_bn_tiles_ws_floats(T, (int)C) + 2 * C}, fopt);
  const int rc = pdt_maxpool3s2_bwd_bn_coef(bf16_ptr(dy), u8_ptr(op, "code", code, dy.numel()),
                                            ptr_or_null<uint16_t>(dz), (int)N, (int)H, (int)W, (int)C, bf16_ptr(x),
                                            opt_f32_ptr(op, "weight", weight, C), f32_ptr(op, "mean", mean, C),
                                            f32_ptr(op, "invstd", invstd, C), coef.data_ptr<float>(), gg.dg_ptr(),
                                            gg.db_ptr(), part.data_ptr<float>(), ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_maxpool3s2_bwd_bn_coef failed: ", rc);
  return {dz, coef, gg.dg, gg.db};
}

// The per-tile partials [2, T, C] fp32 a producer op left for a BatchNorm over C channels; returns T.
int64_t check_tile_parts(const Op& op, const Tensor& part, int64_t C) {
  TORCH_CHECK(part.dim() == 3 && part.size(0) == 2 && part.size(1) >= 1 && part.size(2) == C, op.name,
              ": partials [2, T, C] fp32 expected");
  f32_ptr(op, "part", part, part.numel());
  return part.size(1);
}

// BN training backward with the reduction taken from the dy producer's per-tile partials
// (conv1x1_gemm with bn_x): finalize + apply only.
std::vector<Tensor> bn_bwd_train_tiles(Tensor dy, Tensor x, Tensor part, c10::optional<Tensor> mask,
                                       c10::optional<Tensor> weight, Tensor mean, Tensor invstd, bool relu,
                                       bool has_res, bool need_dgamma) {
  const Op op("bn_bwd_train_tiles", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), "pdt bn bwd: dy layout mismatch");
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  const int BMt = pdt_conv1x1_tile_rows();
  TORCH_CHECK(C % 64 == 0, "pdt bn bwd: C must be a multiple of 64");
  // any tile count: backward partials are plain sums (stride-2 data gradient: 4 phases of tiles)
  const int64_t T = check_tile_parts(op, part, C);
  auto dx = at::empty_like(x);
  Tensor dres;
  if (has_res) dres = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const GammaGrads gg(need_dgamma, C, fopt);
  auto ws = at::empty({pdt_bn_tiles_ws_floats((int)T, (int)C) + 2 * C}, fopt);
  const int rc = pdt_bn_bwd_train_tiles(part.data_ptr<float>(), (int)T, BMt, bf16_ptr(dy), bf16_ptr(x),
                                        relu_mask_ptr(op, mask, relu, M * C / 8), opt_f32_ptr(op, "weight", weight, C),
                                        f32_ptr(op, "mean", mean, C), f32_ptr(op, "invstd", invstd, C), M, (int)C, relu,
                                        has_res, bf16_out(dx), ptr_or_null<uint16_t>(dres), gg.dg_ptr(), gg.db_ptr(),
                                        ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_bn_bwd_train_tiles failed: ", rc);
  return {dx, dres, gg.dg, gg.db};
}

// BN training backward WITHOUT the apply: {coef [3, C] (A, B, D: dx = A dy m + B (x - mean) + D),
// dgamma, dbeta} for a consumer that forms dx while loading its operand (conv1x1_bwd_fused). The
// reduction comes from the dy producer's partials [2, T, C] when given, else from a pass over (dy, x).
std::vector<Tensor> bn_bwd_coef(Tensor dy, Tensor x, c10::optional<Tensor> part, c10::optional<Tensor> mask,
                                c10::optional<Tensor> weight, Tensor mean, Tensor invstd, bool relu, bool need_dgamma) {
  const Op op("bn_bwd_coef", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  TORCH_CHECK(C % 64 == 0, "pdt bn coef: C must be a multiple of 64");
  auto fopt = x.options().dtype(at::kFloat);
  auto coef = at::empty({3, C}, fopt);
  const GammaGrads gg(need_dgamma, C, fopt);
  const float* gp = opt_f32_ptr(op, "weight", weight, C);
  const float* ip = f32_ptr(op, "invstd", invstd, C);
  int rc;
  if (has(part)) {
    const int T = (int)check_tile_parts(op, *part, C);
    auto ws = at::empty({pdt_bn_tiles_ws_floats(T, (int)C)}, fopt);
    rc = pdt_bn_bwd_coef_tiles(part->data_ptr<float>(), T, gp, ip, M, (int)C, coef.data_ptr<float>(), gg.dg_ptr(),
                               gg.db_ptr(), ws.data_ptr<float>(), stream());
  } else {
    check_nhwc_bf16(op, "dy", dy);
    TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), "pdt bn coef: dy layout mismatch");
    auto ws = at::empty({bn_ws_floats(M, C)}, fopt);
    rc = pdt_bn_bwd_coef(bf16_ptr(dy), bf16_ptr(x), relu_mask_ptr(op, mask, relu, M * C / 8), gp,
                         f32_ptr(op, "mean", mean, C), ip, M, (int)C, relu, coef.data_ptr<float>(), gg.dg_ptr(),
                         gg.db_ptr(), ws.data_ptr<float>(), bn_counters(x), stream());
  }
  TORCH_CHECK(rc == 0, "pdt bn_bwd_coef failed: ", rc);
  return {coef, gg.dg, gg.db};
}

// Fused backward of a bottleneck's last 1x1 conv (w [C4, CW, 1, 1]: CW -> C4) and the BatchNorm that
// follows it (csrc/kernels/conv1x1_bwd_fused.hip): from dy (gradient at that BN's output), z (its
// input), mz (its ReLU bits), mean and coef [3, C4] (A, B, D of bn_bwd_coef) and the conv input xa,
// returns {dxa, dw, part}: the conv's data and weight gradients and, when bn_x / bn_mean are given
// (xa is the output of a BatchNorm with input bn_x, ReLU bits bn_mask, batch mean bn_mean), that
// BatchNorm's backward partials [2, G, CW] (else undefined). Empty list: shape not taken.
// xcoef [2, CW] (with bn_x / bn_mean): that BatchNorm's apply was deferred to the conv's forward — xa
// (only its shape is used) is recomputed as relu(xcoef[0] bn_x + xcoef[1]), and its ReLU bits are
// computed and written into bn_mask (an output then, M*CW/8 bytes).
std::vector<Tensor> conv1x1_bwd_fused(Tensor dy, Tensor z, Tensor mz, Tensor mean, Tensor coef, Tensor w, Tensor xa,
                                      c10::optional<Tensor> bn_x, c10::optional<Tensor> bn_mask,
                                      c10::optional<Tensor> bn_mean, c10::optional<Tensor> xcoef,
                                      c10::optional<Tensor> wt_pre) {
  const Op op("conv1x1_bwd_fused", dy);
  check_nhwc_bf16(op, "dy", dy);
  check_nhwc_bf16(op, "z", z);
  TORCH_CHECK(xa.dim() == 4 && xa.device() == op.dev && xa.scalar_type() == at::kBFloat16, "conv1x1_bwd_fused: xa");
  const bool recomp = has(xcoef);
  if (!recomp) check_nhwc_bf16(op, "xa", xa);
  const int64_t C4 = z.size(1), CW = xa.size(1);
  const int64_t M = z.numel() / C4;
  if (!pdt_conv1x1_bwd_fused_ok((int)C4, (int)CW) || M * C4 >= ((int64_t)1 << 31)) return {};
  TORCH_CHECK(dy.sizes() == z.sizes() && dy.strides() == z.strides(), "conv1x1_bwd_fused: dy / z layout mismatch");
  TORCH_CHECK(xa.numel() == M * CW, "conv1x1_bwd_fused: xa pixels");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.numel() == C4 * CW && w.size(0) == C4 && w.device() == op.dev,
              "conv1x1_bwd_fused: weight [C4, CW, 1, 1] bf16");
  Tensor wt;
  if (has(wt_pre)) {  // W^T from the step's batched weight prep
    TORCH_CHECK(wt_pre->scalar_type() == at::kBFloat16 && wt_pre->is_contiguous() && wt_pre->dim() == 2 &&
                    wt_pre->size(0) == CW && wt_pre->size(1) == C4 && wt_pre->device() == op.dev,
                "conv1x1_bwd_fused: wt [CW, C4] bf16");
    wt = *wt_pre;
  } else {
    wt = w.reshape({C4, CW}).t().contiguous();
  }
  auto dxa = at::empty({xa.size(0), CW, xa.size(2), xa.size(3)}, xa.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto dw = at::empty({C4, CW}, w.options());
  const int G = pdt_conv1x1_bwd_fused_grid((int)M, (int)C4, (int)CW);
  auto fopt = z.options().dtype(at::kFloat);
  auto ws = at::empty({(int64_t)G * C4 * CW}, fopt);
  Tensor part;
  BnSide bn;
  if (has(bn_x)) {
    bn = bn_side(op, bn_x, bn_mask, bn_mean, M, CW, false);
    part = at::empty({2, G, CW}, fopt);
  }
  const float* xcp = nullptr;
  uint8_t* mout = nullptr;
  if (recomp) {
    TORCH_CHECK(bn.x && bn.mask, "conv1x1_bwd_fused: xcoef needs bn_x, bn_mean and the bn_mask output");
    xcp = f32_ptr(op, "xcoef", *xcoef, 2 * CW);
    mout = bn_mask->data_ptr<uint8_t>();
    bn.mask = nullptr;
  }
  const float* cp = f32_ptr(op, "coef", coef, 3 * C4);
  const int rc = pdt_conv1x1_bwd_fused(bf16_ptr(dy), bf16_ptr(z), u8_ptr(op, "mz", mz, M * C4 / 8),
                                       f32_ptr(op, "mean", mean, C4), cp, cp + C4, cp + 2 * C4, bf16_ptr(wt),
                                       recomp ? nullptr : bf16_ptr(xa), bn.x, bn.mask, bn.mean,
                                       ptr_or_null<float>(part), xcp, mout, bf16_out(dxa), bf16_out(dw),
                                       ws.data_ptr<float>(), (int)M, (int)C4, (int)CW, stream());
  TORCH_CHECK(rc == 0, "pdt_conv1x1_bwd_fused failed: ", rc);
  return {dxa, dw.view(w.sizes()), part};
}

// ----------------------------------------------------------------------------- LeNet tail (fp32)
// The reference LeNet after the stem (cnn.py:13-22) in one forward kernel / two backward kernels
// (csrc/kernels/lenet_tail.hip). ws: the 8 tail parameters in module order (w2, b2, w3, b3, fw1, fb1,
// fw2, fb2), contiguous fp32.
void check_tail_params(const std::vector<Tensor>& w) {
  TORCH_CHECK(w.size() == 8, "lenet_tail: 8 parameters (conv2 w/b, conv3 w/b, fc1 w/b, fc2 w/b)");
  const int64_t numel[8] = {2400, 16, 48000, 120, 10080, 84, 840, 10};
  for (int i = 0; i < 8; ++i) {
    check_cuda(w[i], "lenet_tail param");
    TORCH_CHECK(w[i].scalar_type() == at::kFloat && w[i].is_contiguous() && w[i].numel() == numel[i],
                "lenet_tail: parameter ", i, " must be contiguous fp32 with ", numel[i], " elements");
  }
}

std::vector<Tensor> lenet_tail_fwd(Tensor p1, std::vector<Tensor> w, double slope) {
  check_tail_params(w);
  check_cuda(p1, "p1");
  TORCH_CHECK(p1.scalar_type() == at::kFloat && p1.is_contiguous() && p1.dim() == 4 && p1.size(1) == 6 &&
              p1.size(2) == 14 && p1.size(3) == 14, "lenet_tail_fwd: p1 [N,6,14,14] contiguous fp32");
  const int64_t N = p1.size(0);
  auto o = p1.options();
  auto logits = at::empty({N, 10}, o);
  auto code2 = at::empty({N, 400}, o.dtype(at::kByte));
  auto p2 = at::empty({N, 400}, o), h3 = at::empty({N, 120}, o), h4 = at::empty({N, 84}, o);
  const int rc = pdt_lenet_tail_fwd(p1.data_ptr<float>(), w[0].data_ptr<float>(), w[1].data_ptr<float>(),
                                    w[2].data_ptr<float>(), w[3].data_ptr<float>(), w[4].data_ptr<float>(),
                                    w[5].data_ptr<float>(), w[6].data_ptr<float>(), w[7].data_ptr<float>(),
                                    (float)slope, (int)N, logits.data_ptr<float>(), code2.data_ptr<uint8_t>(),
                                    p2.data_ptr<float>(), h3.data_ptr<float>(), h4.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_lenet_tail_fwd failed: ", rc);
  return {logits, code2, p2, h3, h4};
}

// -> {dp1, dw2, db2, dw3, db3, dfw1, dfb1, dfw2, dfb2} (parameter gradients in the parameters' shapes)
std::vector<Tensor> lenet_tail_bwd(Tensor dl, Tensor p1, std::vector<Tensor> w, double slope, Tensor code2, Tensor p2,
                                   Tensor h3, Tensor h4) {
  check_tail_params(w);
  const int64_t N = p1.size(0);
  dl = dl.contiguous().to(at::kFloat);
  TORCH_CHECK(dl.numel() == N * 10 && code2.numel() == N * 400 && p2.numel() == N * 400 && h3.numel() == N * 120 &&
              h4.numel() == N * 84, "lenet_tail_bwd: saved tensor sizes");
  auto o = p1.options();
  auto ws = at::empty({pdt_lenet_tail_ws_floats((int)N)}, o);
  auto dp1 = at::empty_like(p1);
  std::vector<Tensor> g;
  for (const auto& t : w) g.push_back(at::empty_like(t));
  const int rc = pdt_lenet_tail_bwd(dl.data_ptr<float>(), p1.data_ptr<float>(), w[0].data_ptr<float>(),
                                    w[1].data_ptr<float>(), w[2].data_ptr<float>(), w[3].data_ptr<float>(),
                                    w[4].data_ptr<float>(), w[5].data_ptr<float>(), w[6].data_ptr<float>(),
                                    w[7].data_ptr<float>(), (float)slope, (int)N, code2.data_ptr<uint8_t>(),
                                    p2.data_ptr<float>(), h3.data_ptr<float>(), h4.data_ptr<float>(),
                                    ws.data_ptr<float>(), dp1.data_ptr<float>(), g[0].data_ptr<float>(),
                                    g[1].data_ptr<float>(), g[2].data_ptr<float>(), g[3].data_ptr<float>(),
                                    g[4].data_ptr<float>(), g[5].data_ptr<float>(), g[6].data_ptr<float>(),
                                    g[7].data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_lenet_tail_bwd failed: ", rc);
  return {dp1, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7]};
}

// ----------------------------------------------------------------------------- 1x1 conv GEMM (+ BN stats)
// A row-major GEMM operand: 2-D contiguous bf16 on the op's device.
void check_mat_bf16(const Op& op, const char* name, const Tensor& t) {
  TORCH_CHECK(t.defined() && t.device() == op.dev && t.scalar_type() == at::kBFloat16 && t.dim() == 2 &&
                  t.is_contiguous(), op.name, ": ", name, " must be 2-D contiguous bf16 on ", op.dev);
}

// out[M,N] = a[M,K] @ b[N,K]^T (+ out, when acc: in-place accumulate). a, b, out: row-major bf16
// (a 1x1 conv's channels_last activations viewed as [N*H*W, C]). stats: also return the per-tile
// partials [2, T, N] fp32 (tile sums, centred tile sums of squares; T = ceil(M / 256)).
// bn_x / bn_mask / bn_mean: out is the gradient at the output of a BatchNorm with this input
// (channels_last [M, N] bf16), ReLU bit-mask (or none) and batch mean: return that BatchNorm's
// backward per-tile partials [2, T, N] fp32 (sum dz, sum dz (x - mean)) instead (not with stats).
// a_coef [2, K] fp32 (optional): a is the INPUT of a BatchNorm + ReLU whose apply is deferred to here —
// the GEMM uses relu(a_coef[0] * a + a_coef[1]) per channel (forward only; not with acc / bn_x).
c10::optional<Tensor> conv1x1_gemm(Tensor a, Tensor b, Tensor out, bool acc, bool stats,
                                   c10::optional<Tensor> c_in, c10::optional<Tensor> c_mask,
                                   c10::optional<Tensor> bn_x, c10::optional<Tensor> bn_mask,
                                   c10::optional<Tensor> bn_mean, int64_t c_stride, int64_t c_H, int64_t c_W,
                                   c10::optional<Tensor> a_coef, bool bn_sum_only, bool no_store) {
  const Op op("conv1x1_gemm", a);
  check_mat_bf16(op, "a", a);
  check_mat_bf16(op, "b", b);
  check_mat_bf16(op, "out", out);
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K && out.size(0) == M && out.size(1) == N, "conv1x1_gemm: shape mismatch");
  TORCH_CHECK(K % 32 == 0 && N % 64 == 0, "conv1x1_gemm: K % 32 == 0 and N % 64 == 0 required");
  TORCH_CHECK(!(acc && stats), "conv1x1_gemm: acc and stats are exclusive");
  // acc source: out itself (in place), or c_in [M, N] (then optionally masked by c_mask, M*N/8 bytes)
  const uint16_t* cp = acc ? bf16_ptr(out) : nullptr;
  if (has(c_in)) {
    TORCH_CHECK(acc, "conv1x1_gemm: c_in needs acc");
    // c_stride > 0: c_in is the compact [M / (c_H c_W) * Hs * Ws, N] gradient of a stride subsampling
    TORCH_CHECK(c_stride <= 0 || (c_H > 0 && c_W > 0 && M % (c_H * c_W) == 0), "conv1x1_gemm: c_H * c_W must divide M");
    TORCH_CHECK(c_stride <= 0 || !has(c_mask), "conv1x1_gemm: c_stride excludes c_mask");
    const int64_t cm_rows = c_stride > 0 ? M / (c_H * c_W) * ((c_H - 1) / c_stride + 1) * ((c_W - 1) / c_stride + 1) : M;
    TORCH_CHECK(c_in->device() == op.dev && c_in->scalar_type() == at::kBFloat16 && c_in->numel() == cm_rows * N &&
                    c_in->is_contiguous(c_in->dim() == 4 ? at::MemoryFormat::ChannelsLast
                                                         : at::MemoryFormat::Contiguous),
                "conv1x1_gemm: c_in must be [M, N] bf16 (channels_last when 4-D)");
    cp = bf16_ptr(*c_in);
  }
  TORCH_CHECK(acc || !has(c_mask), "conv1x1_gemm: c_mask must be uint8 [M * N / 8] with acc");
  const uint8_t* mp = opt_u8_ptr(op, "c_mask", c_mask, M * N / 8);
  TORCH_CHECK(c_stride <= 0 || has(c_in), "conv1x1_gemm: c_stride needs c_in");
  c10::optional<Tensor> part;
  const int64_t T = (M + pdt_conv1x1_tile_rows() - 1) / pdt_conv1x1_tile_rows();
  if (stats) part = at::empty({2, T, N}, a.options().dtype(at::kFloat));
  // bn_sum_only: the BatchNorm input is not read; only the partials' sum(dz) row is meaningful (ALG backward)
  const bool bstats = has(bn_x) || bn_sum_only;
  BnSide bn;
  if (bstats) {
    TORCH_CHECK(!stats, "conv1x1_gemm: stats and bn_x are exclusive");
    bn = bn_side(op, bn_x, bn_mask, bn_mean, M, N, bn_sum_only);
    part = at::empty({2, T, N}, a.options().dtype(at::kFloat));
  }
  TORCH_CHECK(!has(a_coef) || (!acc && !bstats), "conv1x1_gemm: a_coef is forward-only (no acc / bn_x)");
  const int rc = pdt_conv1x1_gemm(bf16_ptr(a), bf16_ptr(b), bf16_out(out), cp, mp,
                                  stats ? part->data_ptr<float>() : nullptr, (int)M, (int)K, (int)N, bn.x, bn.mask,
                                  bn.mean, bstats ? part->data_ptr<float>() : nullptr, (int)c_stride, (int)c_H,
                                  (int)c_W, opt_f32_ptr(op, "a_coef", a_coef, 2 * K), stream(), no_store ? 1 : 0);
  TORCH_CHECK(rc == 0, "pdt_conv1x1_gemm failed: ", rc);
  return part;
}

// A BatchNorm (+ residual) + ReLU applied in the epilogue of the 1x1-conv GEMM that produced its input
// (csrc/kernels/conv1x1.hip APPLY): y = relu(ab[0] * (a b^T) + ab[1] + r), r = res or rab[0] res + rab[1].
// a [M, K], b [N, K] bf16 row-major; res: the residual (bf16, M * N elements, channels_last when 4-D; y gets
// its shape / layout); ab, rab: fp32 [2, N]; a_coef: fp32 [2, K] (A is a deferred BatchNorm input, ATR).
// Returns {y, mask uint8 [M * N / 8]}.
std::vector<Tensor> conv1x1_gemm_apply(Tensor a, Tensor b, Tensor res, Tensor ab, c10::optional<Tensor> rab,
                                       c10::optional<Tensor> a_coef) {
  const Op op("conv1x1_gemm_apply", a);
  check_mat_bf16(op, "a", a);
  check_mat_bf16(op, "b", b);
  TORCH_CHECK(a.size(1) == b.size(1), "conv1x1_gemm_apply: a [M, K], b [N, K] contiguous bf16");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  const auto fmt = res.dim() == 4 ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous;
  TORCH_CHECK(res.device() == op.dev && res.scalar_type() == at::kBFloat16 && res.numel() == M * N &&
                  res.is_contiguous(fmt) && (res.dim() != 4 || res.size(1) == N),
              "conv1x1_gemm_apply: res must be [M, N] bf16 (channels_last when 4-D)");
  auto y = at::empty_like(res, res.options(), fmt);
  auto mask = at::empty({M * N / 8}, res.options().dtype(at::kByte));
  const int rc = pdt_conv1x1_gemm_apply(bf16_ptr(a), bf16_ptr(b), bf16_out(y), bf16_ptr(res),
                                        f32_ptr(op, "ab", ab, 2 * N), opt_f32_ptr(op, "rab", rab, 2 * N),
                                        mask.data_ptr<uint8_t>(), (int)M, (int)K, (int)N,
                                        opt_f32_ptr(op, "a_coef", a_coef, 2 * K), stream());
  TORCH_CHECK(rc == 0, "pdt_conv1x1_gemm_apply failed: ", rc);
  return {y, mask};
}

// Batched per-step weight transforms (csrc/kernels/weight_prep.hip): for each i, src[i] = a conv weight
// [Co, Ci, k, k] bf16 (k = 1: any layout; k = 3: channels_last, storage [Co][3][3][Ci]) -> dst[i]: k = 1:
// W^T [Ci, Co] contiguous; k = 3: the flipped transposed weights [Ci, Co, 3, 3] channels_last (= conv3x3_flip).
void weight_prep(std::vector<Tensor> src, std::vector<Tensor> dst) {
  TORCH_CHECK(src.size() == dst.size(), "weight_prep: src / dst lists differ");
  if (src.empty()) return;
  const Op op("weight_prep", src[0]);
  const int cap = pdt_weight_prep_max_items();
  std::vector<const uint16_t*> sp;
  std::vector<uint16_t*> dp;
  std::vector<int> R, C, T;
  auto flush = [&]() {
    if (sp.empty()) return;
    TORCH_CHECK(pdt_weight_prep(sp.data(), dp.data(), R.data(), C.data(), T.data(), (int)sp.size(), stream()) == 0,
                "pdt_weight_prep failed");
    sp.clear(); dp.clear(); R.clear(); C.clear(); T.clear();
  };
  for (size_t i = 0; i < src.size(); ++i) {
    const Tensor& w = src[i];
    const Tensor& d = dst[i];
    TORCH_CHECK(w.device() == op.dev && d.device() == op.dev, "weight_prep: src / dst must be on ", op.dev);
    TORCH_CHECK(w.dim() == 4 && w.scalar_type() == at::kBFloat16 && d.scalar_type() == at::kBFloat16 &&
                    w.size(2) == w.size(3) && (w.size(2) == 1 || w.size(2) == 3),
                "weight_prep: bf16 [Co, Ci, k, k] weights, k = 1 or 3");
    const int64_t Co = w.size(0), Ci = w.size(1), k = w.size(2);
    if (k == 1) {
      TORCH_CHECK(w.is_contiguous() || w.is_contiguous(at::MemoryFormat::ChannelsLast), "weight_prep: 1x1 weight layout");
      TORCH_CHECK(d.dim() == 2 && d.size(0) == Ci && d.size(1) == Co && d.is_contiguous(), "weight_prep: dst [Ci, Co]");
    } else {
      TORCH_CHECK(w.is_contiguous(at::MemoryFormat::ChannelsLast), "weight_prep: 3x3 weight must be channels_last");
      TORCH_CHECK(d.dim() == 4 && d.size(0) == Ci && d.size(1) == Co && d.size(2) == 3 && d.size(3) == 3 &&
                      d.is_contiguous(at::MemoryFormat::ChannelsLast),
                  "weight_prep: dst [Ci, Co, 3, 3] channels_last");
    }
    sp.push_back(bf16_ptr(w));
    dp.push_back(bf16_out(d));
    R.push_back((int)Co);
    C.push_back((int)Ci);
    T.push_back((int)(k * k));
    if ((int)sp.size() == cap) flush();
  }
  flush();
}

// Weight gradient of a stride-1 1x1 conv (csrc/kernels/conv1x1_wgrad.hip): dw [Co, Ci] bf16 =
// dy[M, Co]^T x[M, Ci] from the row-major bf16 NHWC views (split-K over pixels, fixed-order fp32
// reduction). Returns an undefined tensor for a shape the kernel does not take (caller falls back).
Tensor conv1x1_wgrad(Tensor x, Tensor dy) {
  const Op op("conv1x1_wgrad", x);
  check_mat_bf16(op, "x", x);
  check_mat_bf16(op, "dy", dy);
  TORCH_CHECK(x.size(0) == dy.size(0), "conv1x1_wgrad: x [M, Ci], dy [M, Co]");
  const int64_t M = x.size(0), Ci = x.size(1), Co = dy.size(1);
  if (M * std::max(Ci, Co) >= ((int64_t)1 << 31)) return Tensor();
  int ns = 0;
  const int64_t wsf = pdt_conv1x1_wgrad_ws_floats((int)M, (int)Ci, (int)Co, &ns);
  if (wsf == 0) return Tensor();
  auto ws = at::empty({wsf}, x.options().dtype(at::kFloat));
  auto dw = at::empty({Co, Ci}, x.options());
  const int rc = pdt_conv1x1_wgrad(bf16_ptr(x), bf16_ptr(dy), bf16_out(dw), ws.data_ptr<float>(), (int)M, (int)Ci,
                                   (int)Co, stream());
  if (rc == -1 || rc == -2) return Tensor();
  TORCH_CHECK(rc == 0, "pdt_conv1x1_wgrad failed: ", rc);
  return dw;
}

// ALG backward of conv3 + bn3 (csrc/kernels/bn_alg.hip, ops/conv.py _bwd_alg): [dy1 | dy2 | 1]^T x in fp32,
// rows co1 + co2 (+ the ones block: column sums of x). x [M, Ci], dy1 [M, co1], dy2 [M, co2] contiguous bf16.
// Returns an empty tensor for an unsupported shape.
Tensor conv1x1_wgrad_seg(Tensor x, Tensor dy1, Tensor dy2) {
  const Op op("conv1x1_wgrad_seg", x);
  check_mat_bf16(op, "x", x);
  check_mat_bf16(op, "dy1", dy1);
  check_mat_bf16(op, "dy2", dy2);
  TORCH_CHECK(dy1.size(0) == x.size(0) && dy2.size(0) == x.size(0), "conv1x1_wgrad_seg: contiguous bf16 [M, *] operands");
  const int64_t M = x.size(0), Ci = x.size(1), co1 = dy1.size(1), co2 = dy2.size(1);
  if (M * std::max(std::max(Ci, co1), co2) >= ((int64_t)1 << 31)) return Tensor();
  int rows = 0;
  const int64_t wsf = pdt_conv1x1_wgrad_seg_ws_floats((int)M, (int)Ci, (int)co1, (int)co2, &rows);
  if (wsf == 0) return Tensor();
  auto ws = at::empty({wsf}, x.options().dtype(at::kFloat));
  auto out = at::empty({rows, Ci}, x.options().dtype(at::kFloat));
  const int rc = pdt_conv1x1_wgrad_seg(bf16_ptr(x), bf16_ptr(dy1), (int)co1, bf16_ptr(dy2), (int)co2,
                                       out.data_ptr<float>(), ws.data_ptr<float>(), (int)M, (int)Ci, stream());
  if (rc == -1 || rc == -2) return Tensor();
  TORCH_CHECK(rc == 0, "pdt_conv1x1_wgrad_seg failed: ", rc);
  return out;
}

// out[M, N] = [a1 | a2 x rep2 | 1] b^T (b [N, k1 + rep2 k2 + 32]) with the BSTATS epilogue when bn_x is given
// (then returns the backward partials [2, T, N], as conv1x1_gemm).
c10::optional<Tensor> conv1x1_gemm_seg(Tensor a1, Tensor a2, int64_t rep2, Tensor b, Tensor out,
                                       c10::optional<Tensor> bn_x, c10::optional<Tensor> bn_mask,
                                       c10::optional<Tensor> bn_mean) {
  const Op op("conv1x1_gemm_seg", a1);
  check_mat_bf16(op, "a1", a1);
  check_mat_bf16(op, "a2", a2);
  check_mat_bf16(op, "b", b);
  check_mat_bf16(op, "out", out);
  const int64_t M = a1.size(0), k1 = a1.size(1), k2 = a2.size(1), N = b.size(0);
  TORCH_CHECK(a2.size(0) == M && out.size(0) == M && out.size(1) == N && b.size(1) == k1 + rep2 * k2 + 32 && rep2 >= 1,
              "conv1x1_gemm_seg: shape mismatch");
  TORCH_CHECK(k1 % 32 == 0 && k2 % 32 == 0 && N % 64 == 0, "conv1x1_gemm_seg: k1, k2 % 32 and N % 64 required");
  c10::optional<Tensor> part;
  BnSide bn;
  if (has(bn_x)) {
    bn = bn_side(op, bn_x, bn_mask, bn_mean, M, N, false);
    const int64_t T = (M + pdt_conv1x1_tile_rows() - 1) / pdt_conv1x1_tile_rows();
    part = at::empty({2, T, N}, a1.options().dtype(at::kFloat));
  }
  const int rc = pdt_conv1x1_gemm_seg(bf16_ptr(a1), (int)k1, bf16_ptr(a2), (int)k2, (int)rep2, bf16_ptr(b),
                                      bf16_out(out), (int)M, (int)N, bn.x, bn.mask, bn.mean,
                                      part.has_value() ? part->data_ptr<float>() : nullptr, stream());
  TORCH_CHECK(rc == 0, "pdt_conv1x1_gemm_seg failed: ", rc);
  return part;
}

// The ALG backward's fp32 Gram workspace wg [rows, CW] (csrc/kernels/bn_alg.hip): at least min_rows rows.
const float* alg_wg_ptr(const Op& op, const Tensor& wg, int64_t CW, int64_t min_rows) {
  TORCH_CHECK(wg.dim() == 2 && wg.size(1) == CW && wg.size(0) >= min_rows, op.name, ": wg [>= ", min_rows, ", ", CW,
              "] fp32");
  return f32_ptr(op, "wg", wg, wg.numel());
}

// (bcat [CW, C4 + 2 CW + 32] bf16, dW [C4, CW] bf16) of the ALG backward (csrc/kernels/bn_alg.hip).
std::vector<Tensor> bn_alg_assemble(Tensor w, Tensor coef, Tensor mean, Tensor G, Tensor wg, Tensor BWG, int64_t rep) {
  const Op op("bn_alg_assemble", w);
  check_mat_bf16(op, "w", w);
  const int64_t C4 = w.size(0), CW = w.size(1);
  TORCH_CHECK(rep == 1 || rep == 2, "bn_alg_assemble: rep 1 or 2");
  auto bcat = at::empty({CW, C4 + rep * CW + 32}, w.options());
  auto dW = at::empty({C4, CW}, w.options());
  const int rc = pdt_bn_alg_assemble(bf16_ptr(w), f32_ptr(op, "coef", coef, 3 * C4), f32_ptr(op, "mean", mean, C4),
                                     f32_ptr(op, "G", G, (C4 / 128) * CW * CW), alg_wg_ptr(op, wg, CW, C4 + CW + 1),
                                     f32_ptr(op, "BWG", BWG, std::max<int64_t>(1, CW / 128) * C4 * CW), bf16_out(bcat),
                                     bf16_out(dW), (int)C4, (int)CW, (int)rep, stream());
  TORCH_CHECK(rc == 0, "pdt_bn_alg_assemble failed: ", rc);
  return {bcat, dW};
}

// (G [CW, CW], BWG [C4, CW]) fp32 of the ALG backward: W^T diag(B) W and diag(B) W Gram (csrc/kernels/bn_alg.hip).
std::vector<Tensor> bn_alg_small_gemm(Tensor w, Tensor coef, Tensor wg, c10::optional<Tensor> wt) {
  const Op op("bn_alg_small_gemm", w);
  check_mat_bf16(op, "w", w);
  const int64_t C4 = w.size(0), CW = w.size(1);
  TORCH_CHECK(C4 % 64 == 0 && CW % 64 == 0, "bn_alg_small_gemm: coef [3, C4], wg [>= C4 + CW, CW] fp32, C4 / CW % 64");
  TORCH_CHECK(C4 % 128 == 0 && (CW == 64 || CW % 128 == 0), "bn_alg_small_gemm: C4 % 128, CW 64 or % 128");
  // split-K slices (summed by bn_alg_assemble): G [C4 / 128, CW, CW], BWG [max(1, CW / 128), C4, CW]
  auto G = at::empty({C4 / 128, CW, CW}, wg.options());
  auto BWG = at::empty({std::max<int64_t>(1, CW / 128), C4, CW}, wg.options());
  const uint16_t* wtp = nullptr;
  if (has(wt)) {  // W^T [CW, C4]: the matrix-core form
    check_mat_bf16(op, "wt", *wt);
    TORCH_CHECK(wt->size(0) == CW && wt->size(1) == C4, "bn_alg_small_gemm: wt [CW, C4] bf16 contiguous");
    wtp = bf16_ptr(*wt);
  }
  TORCH_CHECK(pdt_bn_alg_small_gemm(bf16_ptr(w), wtp, f32_ptr(op, "coef", coef, 3 * C4),
                                    alg_wg_ptr(op, wg, CW, C4 + CW), G.data_ptr<float>(), BWG.data_ptr<float>(),
                                    (int)C4, (int)CW, stream()) == 0,
              "pdt_bn_alg_small_gemm failed");
  return {G, BWG};
}

// Completes a sum-only producer's BatchNorm backward partials in place (csrc/kernels/bn_alg.hip).
void bn_alg_fix_s2(Tensor part, Tensor wg, Tensor w) {
  const Op op("bn_alg_fix_s2", part);
  check_mat_bf16(op, "w", w);
  const int64_t C4 = w.size(0), CW = w.size(1);
  TORCH_CHECK(part.dim() == 3 && part.size(0) == 2 && part.size(2) == C4, "bn_alg_fix_s2: part [2, T, C4] fp32");
  TORCH_CHECK(pdt_bn_alg_fix_s2(f32_ptr(op, "part", part, part.numel()), (int)part.size(1),
                                alg_wg_ptr(op, wg, CW, C4), bf16_ptr(w), (int)C4, (int)CW, stream()) == 0,
              "pdt_bn_alg_fix_s2 failed");
}

// A downsample BatchNorm's backward partials [2, 1, C4] from s1 = sum(g), its mean and the ALG pass (bn_alg.hip).
Tensor bn_alg_ds_part(Tensor s1, Tensor mean, Tensor wg, Tensor w) {
  const Op op("bn_alg_ds_part", s1);
  check_mat_bf16(op, "w", w);
  const int64_t C4 = w.size(0), CW = w.size(1);
  auto part = at::empty({2, 1, C4}, s1.options());
  TORCH_CHECK(pdt_bn_alg_ds_part(part.data_ptr<float>(), f32_ptr(op, "s1", s1, C4), f32_ptr(op, "mean", mean, C4),
                                 alg_wg_ptr(op, wg, CW, C4), bf16_ptr(w), (int)C4, (int)CW, stream()) == 0,
              "pdt_bn_alg_ds_part failed");
  return part;
}

// BN training forward with the statistics taken from conv1x1_gemm's per-tile partials.
std::vector<Tensor> bn_fwd_train_tiles(Tensor x, Tensor part, c10::optional<Tensor> res, c10::optional<Tensor> weight,
                                       c10::optional<Tensor> bias, c10::optional<Tensor> running_mean,
                                       c10::optional<Tensor> running_var, double momentum, double eps, bool relu,
                                       c10::optional<Tensor> res_ab, bool apply, int64_t sub) {
  const Op op("bn_fwd_train_tiles", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t C = x.size(1);
  const int64_t M = x.numel() / C;
  TORCH_CHECK(C % 64 == 0, "pdt bn: C must be a multiple of 64");
  TORCH_CHECK(part.dim() == 3 && part.size(0) == 2 && part.size(2) == C,
              "bn_fwd_train_tiles: partials [2, T, C] fp32 expected");
  // tile height from the partials' row count: 256 (every producer) or 224 (the layer-1 row-tile 3x3,
  // used only where M / 224 >= 256, so the two never give the same T)
  const int64_t T = part.size(1);
  const int BMt = T == (M + 255) / 256 ? 256 : (M % 224 == 0 && T == M / 224 ? 224 : 0);
  TORCH_CHECK(BMt > 0, "bn_fwd_train_tiles: partials row count ", T, " matches no tile height for M = ", M);
  const float* rab = opt_f32_ptr(op, "res_ab", res_ab, 2 * C);
  Tensor y;
  if (apply) y = at::empty_like(x);
  Tensor mask;
  if (relu && apply) mask = at::empty({M * C / 8}, x.options().dtype(at::kByte));
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({C}, fopt), invstd = at::empty({C}, fopt);
  auto ws = at::empty({pdt_bn_tiles_ws_floats((int)T, (int)C)}, fopt);
  // sub >= 2: also the stride-sub subsample of y (x must be 4-D [N, C, H, W])
  Tensor ys;
  if (sub >= 2) {
    TORCH_CHECK(apply && x.dim() == 4, "bn_fwd_train_tiles: the subsample output needs the apply and a 4-D x");
    ys = at::empty({x.size(0), C, (x.size(2) - 1) / sub + 1, (x.size(3) - 1) / sub + 1},
                   x.options().memory_format(at::MemoryFormat::ChannelsLast));
  }
  const int rc = pdt_bn_fwd_train_tiles(f32_ptr(op, "part", part, 2 * T * C), (int)T, BMt, bf16_ptr(x),
                                        residual_ptr(op, x, res), rab, rab ? rab + C : nullptr,
                                        opt_f32_ptr(op, "weight", weight, C), opt_f32_ptr(op, "bias", bias, C),
                                        opt_f32_ptr(op, "running_mean", running_mean, C),
                                        opt_f32_ptr(op, "running_var", running_var, C), (float)momentum, (float)eps, M,
                                        (int)C, relu, ptr_or_null<uint16_t>(y), ptr_or_null<uint8_t>(mask),
                                        mean.data_ptr<float>(), invstd.data_ptr<float>(), ws.data_ptr<float>(),
                                        stream(), ptr_or_null<uint16_t>(ys), sub >= 2 ? (int)x.size(2) : 0,
                                        sub >= 2 ? (int)x.size(3) : 0, (int)sub);
  if (rc == -4) return {};  // (subsample not taken: the caller gathers)
  TORCH_CHECK(rc == 0, "pdt_bn_fwd_train_tiles failed: ", rc);
  if (!apply)  // the apply coefficients (a, b) are the workspace's last 2C floats (past the level-1 sums)
    return {Tensor(), Tensor(), mean, invstd, ws.narrow(0, ws.numel() - 2 * C, 2 * C).view({2, C})};
  if (sub >= 2) return {y, mask, mean, invstd, ys};
  return {y, mask, mean, invstd};
}

// ----------------------------------------------------------------------------- 3x3 conv (stride 1, pad 1)
// A 3x3 conv weight [*, Ci, 3, 3] bf16 on the op's device, returned channels_last (storage [*][3][3][Ci], the
// kernels' layout).
Tensor check_w3x3(const Op& op, const Tensor& w, int64_t Ci) {
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3 && w.size(1) == Ci &&
                  w.scalar_type() == at::kBFloat16 && w.device() == op.dev,
              op.name, ": weight [Co, ", Ci, ", 3, 3] bf16 on ", op.dev);
  return w.contiguous(at::MemoryFormat::ChannelsLast);
}

// Which kernel conv3x3s1_fwd (and _fwd_stats / _fwd_bnbwd, where they have the epilogue) runs at this shape
// under the current conv3x3_opt bits: the launchers' own decision (conv3x3.hip variant_of). Host only.
const char* conv3x3s1_variant(int64_t N, int64_t H, int64_t W, int64_t Ci, int64_t Co) {
  static const char* const names[] = {"tap_wide", "tap_narrow", "halo_wide", "halo_narrow", "wst", "wsr"};
  static_assert(PDT_C3_TAP_WIDE == 0 && PDT_C3_TAP_NARROW == 1 && PDT_C3_HALO_WIDE == 2 && PDT_C3_HALO_NARROW == 3 &&
                    PDT_C3_WST == 4 && PDT_C3_WSR == 5, "names follow launchers.h");
  const int v = pdt_conv3x3s1_variant((int)N, (int)H, (int)W, (int)Ci, (int)Co);
  TORCH_CHECK(v >= 0 && v <= PDT_C3_WSR, "conv3x3s1_variant: shape not taken by conv3x3s1_fwd: ", v);
  return names[v];
}

// (R, ntiles, tiles_per_split, nsplit, co_tile) of conv3x3s1_wgrad / conv3x3s2_wgrad at this INPUT shape under
// the current conv3x3_wgrad_tune setting (conv3x3_wgrad.hip geo_of), or None where the kernel declines. Host only.
py::object conv3x3_wgrad_geo(int64_t N, int64_t H, int64_t W, int64_t Ci, int64_t Co, int64_t stride) {
  int g[5];
  if (!pdt_conv3x3_wgrad_geo((int)N, (int)H, (int)W, (int)Ci, (int)Co, (int)stride, g)) return py::none();
  return py::make_tuple(g[0], g[1], g[2], g[3], g[4]);
}

// y = conv2d(x, w, stride=1, padding=1) for channels_last bf16 x [N,Ci,H,W] and w [Co,Ci,3,3].
Tensor conv3x3s1_fwd(Tensor x, Tensor w) {
  const Op op("conv3x3s1_fwd", x);
  check_nhwc_bf16(op, "x", x);
  w = check_w3x3(op, w, x.size(1));
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = w.size(0);
  auto y = at::empty({N, Co, H, W}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_conv3x3s1_fwd(bf16_ptr(x), bf16_ptr(w), bf16_out(y), (int)N, (int)H, (int)W, (int)Ci, (int)Co,
                                   stream());
  TORCH_CHECK(rc == 0, "pdt_conv3x3s1_fwd failed: ", rc);
  return y;
}

// conv3x3s1_fwd + the per-tile BatchNorm statistics of y (tile_stats.h): {y, part [2, T, Co]}, or
// {y} alone when the shape runs on a kernel without the statistics epilogue.
std::vector<Tensor> conv3x3s1_fwd_stats(Tensor x, Tensor w) {
  const Op op("conv3x3s1_fwd_stats", x);
  check_nhwc_bf16(op, "x", x);
  w = check_w3x3(op, w, x.size(1));
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = w.size(0);
  auto y = at::empty({N, Co, H, W}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t rows = pdt_conv3x3s1_stats_tile_rows((int)N, (int)H, (int)W, (int)Ci, (int)Co);
  const int64_t T = (N * H * W + rows - 1) / rows;
  auto part = at::empty({2, T, Co}, x.options().dtype(at::kFloat));
  const int rc = pdt_conv3x3s1_fwd_stats(bf16_ptr(x), bf16_ptr(w), bf16_out(y), part.data_ptr<float>(), (int)N, (int)H,
                                         (int)W, (int)Ci, (int)Co, stream());
  if (rc == -5) return {conv3x3s1_fwd(x, w)};
  TORCH_CHECK(rc == 0, "pdt_conv3x3s1_fwd_stats failed: ", rc);
  return {y, part};
}

// y = conv3x3s1(x, w) where y is the gradient at a BatchNorm's output (bn_x: that BN's input, same
// shape as y; bn_mask: its ReLU bit-mask or none; bn_mean: its batch mean): returns {y, partials
// [2, T, Co]} of the BN's backward reduction, or {y} where only a kernel without the epilogue applies.
std::vector<Tensor> conv3x3s1_fwd_bnbwd(Tensor x, Tensor w, Tensor bn_x, c10::optional<Tensor> bn_mask,
                                        Tensor bn_mean) {
  const Op op("conv3x3s1_fwd_bnbwd", x);
  check_nhwc_bf16(op, "x", x);
  w = check_w3x3(op, w, x.size(1));
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = w.size(0);
  const BnSide bn = bn_side(op, bn_x, bn_mask, bn_mean, N * H * W, Co, false);
  TORCH_CHECK(bn_x.dim() == 4 && bn_x.size(0) == N && bn_x.size(1) == Co && bn_x.size(2) == H && bn_x.size(3) == W,
              "conv3x3s1_fwd_bnbwd: bn_x must have the output's shape");
  auto y = at::empty({N, Co, H, W}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t rows = pdt_conv3x3s1_bnbwd_tile_rows((int)N, (int)H, (int)W, (int)Ci, (int)Co);
  const int64_t T = (N * H * W + rows - 1) / rows;
  auto part = at::empty({2, T, Co}, x.options().dtype(at::kFloat));
  const int rc = pdt_conv3x3s1_fwd_bnbwd(bf16_ptr(x), bf16_ptr(w), bf16_out(y), bn.x, bn.mask, bn.mean,
                                         part.data_ptr<float>(), (int)N, (int)H, (int)W, (int)Ci, (int)Co, stream());
  if (rc == -5) return {conv3x3s1_fwd(x, w)};
  TORCH_CHECK(rc == 0, "pdt_conv3x3s1_fwd_bnbwd failed: ", rc);
  return {y, part};
}

// ----------------------------------------------------------------------------- 3x3 conv (stride 2, pad 1)
// y = conv2d(x, w, stride=2, padding=1), channels_last bf16 (csrc/kernels/conv3x3_s2.hip); stats: also
// the per-tile BatchNorm statistics of y -> {y, part [2, T, Co]}. Ci % 64, Co % 128 == 0 (returns {} for
// a shape the kernel does not take).
std::vector<Tensor> conv3x3s2_fwd(Tensor x, Tensor w, bool stats) {
  const Op op("conv3x3s2_fwd", x);
  check_nhwc_bf16(op, "x", x);
  w = check_w3x3(op, w, x.size(1));
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = w.size(0);
  const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  auto y = at::empty({N, Co, Ho, Wo}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  Tensor part;
  if (stats) part = at::empty({2, (N * Ho * Wo + 255) / 256, Co}, x.options().dtype(at::kFloat));
  const int rc = pdt_conv3x3s2_fwd(bf16_ptr(x), bf16_ptr(w), bf16_out(y), ptr_or_null<float>(part), (int)N, (int)H,
                                   (int)W, (int)Ci, (int)Co, stream());
  if (rc == -1 || rc == -2) return {};
  TORCH_CHECK(rc == 0, "pdt_conv3x3s2_fwd failed: ", rc);
  if (stats) return {y, part};
  return {y};
}

// dx [N, Ci, H, W] of that conv from dy [N, Co, Ho, Wo] and wf = conv3x3_flip(w). With bn_x / bn_mean
// (bn_mask optional): dx is the gradient at a BatchNorm's output -> {dx, partials [2, T, Ci]} of its
// backward reduction (T = 4 phases of tiles). Returns {} for a shape the kernel does not take.
std::vector<Tensor> conv3x3s2_dgrad(Tensor dy, Tensor wf, int64_t H, int64_t W, c10::optional<Tensor> bn_x,
                                    c10::optional<Tensor> bn_mask, c10::optional<Tensor> bn_mean) {
  const Op op("conv3x3s2_dgrad", dy);
  check_nhwc_bf16(op, "dy", dy);
  wf = check_w3x3(op, wf, dy.size(1));  // the flipped weight [Ci, Co, 3, 3]
  const int64_t N = dy.size(0), Co = dy.size(1), Ci = wf.size(0);
  TORCH_CHECK(dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == (W - 1) / 2 + 1, "conv3x3s2_dgrad: dy spatial size");
  auto dx = at::empty({N, Ci, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  BnSide bn;
  Tensor part;
  if (has(bn_x)) {
    bn = bn_side(op, bn_x, bn_mask, bn_mean, N * H * W, Ci, false);
    TORCH_CHECK(bn_x->sizes() == dx.sizes(), "conv3x3s2_dgrad: bn_x must have dx's shape");
    part = at::empty({2, (int64_t)pdt_conv3x3s2_dgrad_tiles((int)N, (int)H, (int)W), Ci},
                     dy.options().dtype(at::kFloat));
  }
  const int rc = pdt_conv3x3s2_dgrad(bf16_ptr(dy), bf16_ptr(wf), bf16_out(dx), bn.x, bn.mask, bn.mean,
                                     ptr_or_null<float>(part), (int)N, (int)H, (int)W, (int)Ci, (int)Co, stream());
  if (rc == -1 || rc == -2) return {};
  TORCH_CHECK(rc == 0, "pdt_conv3x3s2_dgrad failed: ", rc);
  if (has(bn_x)) return {dx, part};
  return {dx};
}

// Weight gradient of the stride-2 pad-1 3x3 conv (conv3x3_wgrad.hip, S = 2): dw [Co, Ci, 3, 3]
// channels_last bf16 from x [N, Ci, H, W] and dy [N, Co, Ho, Wo]; undefined for an unsupported shape.
Tensor conv3x3s2_wgrad(Tensor x, Tensor dy) {
  const Op op("conv3x3s2_wgrad", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = dy.size(1);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == (W - 1) / 2 + 1,
              "conv3x3s2_wgrad: dy [N, Co, Ho, Wo]");
  int ns = 0;
  const int64_t wsf = pdt_conv3x3s2_wgrad_ws_floats((int)N, (int)H, (int)W, (int)Ci, (int)Co, &ns);
  if (wsf == 0 || N * H * W * std::max(Ci, Co) >= ((int64_t)1 << 31)) return Tensor();
  auto ws = at::empty({wsf}, x.options().dtype(at::kFloat));
  auto dw = at::empty({Co, Ci, 3, 3}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_conv3x3s2_wgrad(bf16_ptr(x), bf16_ptr(dy), bf16_out(dw), ws.data_ptr<float>(), (int)N, (int)H,
                                     (int)W, (int)Ci, (int)Co, stream());
  if (rc == -4 || rc == -1 || rc == -2) return Tensor();
  TORCH_CHECK(rc == 0, "pdt_conv3x3s2_wgrad failed: ", rc);
  return dw;
}

// Weight gradient of the stride-1 pad-1 3x3 conv (csrc/kernels/conv3x3_wgrad.hip): dw [Co, Ci, 3, 3]
// channels_last bf16 from channels_last bf16 x [N, Ci, H, W] and dy [N, Co, H, W]. Returns an
// undefined tensor for a shape the kernel does not take (caller falls back).
Tensor conv3x3s1_wgrad(Tensor x, Tensor dy) {
  const Op op("conv3x3s1_wgrad", x);
  check_nhwc_bf16(op, "x", x);
  check_nhwc_bf16(op, "dy", dy);
  const int64_t N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3), Co = dy.size(1);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == H && dy.size(3) == W, "conv3x3s1_wgrad: dy [N, Co, H, W]");
  int ns = 0;
  const int64_t wsf = pdt_conv3x3_wgrad_ws_floats((int)N, (int)H, (int)W, (int)Ci, (int)Co, &ns);
  if (wsf == 0 || N * H * W * std::max(Ci, Co) >= ((int64_t)1 << 31)) return Tensor();
  auto ws = at::empty({wsf}, x.options().dtype(at::kFloat));
  auto dw = at::empty({Co, Ci, 3, 3}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_conv3x3s1_wgrad(bf16_ptr(x), bf16_ptr(dy), bf16_out(dw), ws.data_ptr<float>(), (int)N, (int)H,
                                     (int)W, (int)Ci, (int)Co, stream());
  if (rc == -4) return Tensor();
  TORCH_CHECK(rc == 0, "pdt_conv3x3s1_wgrad failed: ", rc);
  return dw;
}

// Data-gradient weights: wf [Ci, Co, 3, 3] (channels_last storage [Ci][3][3][Co]) with
// wf[ci, co, kh, kw] = w[co, ci, 2 - kh, 2 - kw], so dx = conv3x3s1_fwd(dy, wf).
Tensor conv3x3_flip(Tensor w) {
  const Op op("conv3x3_flip", w);
  w = check_w3x3(op, w, w.dim() == 4 ? w.size(1) : 0);
  const int64_t Co = w.size(0), Ci = w.size(1);
  auto wf = at::empty({Ci, Co, 3, 3}, w.options().memory_format(at::MemoryFormat::ChannelsLast));
  TORCH_CHECK(pdt_conv3x3_flip_weights(bf16_ptr(w), bf16_out(wf), (int)Co, (int)Ci, stream()) == 0,
              "pdt_conv3x3_flip_weights failed");
  return wf;
}

// ----------------------------------------------------------------------------- 7x7/s2 stem conv (3 -> 64)
// The stem's input x [N, 3, H, W] (W % 32 == 0; the weight gradients also need W <= 224) and weight [64, 3, 7, 7].
void check_stem_x(const Op& op, const Tensor& x) {
  check_nhwc_bf16(op, "x", x);
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 && x.size(3) % 32 == 0, op.name, ": x [N, 3, H, W] with W % 32 == 0");
}
Tensor check_stem_w(const Op& op, const Tensor& w) {
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 64 && w.size(1) == 3 && w.size(2) == 7 && w.size(3) == 7 &&
                  w.scalar_type() == at::kBFloat16 && w.device() == op.dev, op.name, ": weight [64, 3, 7, 7] bf16");
  return w.contiguous(at::MemoryFormat::ChannelsLast);
}

// y = conv2d(x, w, stride=2, padding=3) for channels_last bf16 x [N,3,H,W] (W % 32 == 0) and w [64,3,7,7].
Tensor stem_conv_fwd(Tensor x, Tensor w) {
  const Op op("stem_conv_fwd", x);
  check_stem_x(op, x);
  w = check_stem_w(op, w);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3), OH = (H - 1) / 2 + 1, OW = W / 2;
  auto wp = at::empty({pdt_stem_conv_wprep_elems()}, w.options());
  auto y = at::empty({N, 64, OH, OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_stem_conv_fwd(bf16_ptr(x), bf16_ptr(w), bf16_out(wp), bf16_out(y), (int)N, (int)H, (int)W,
                                   stream());
  TORCH_CHECK(rc == 0, "pdt_stem_conv_fwd failed: ", rc);
  return y;
}

// stem_conv_fwd plus the output's BatchNorm statistics -> {y, part} (part: P (2 * 64 + 1) floats, the
// input of bn_relu_maxpool_fwd_parts); {} when it does not apply (W != 224).
std::vector<Tensor> stem_conv_fwd_stats(Tensor x, Tensor w) {
  const Op op("stem_conv_fwd_stats", x);
  check_stem_x(op, x);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3), OH = (H - 1) / 2 + 1, OW = W / 2;
  const int64_t P = pdt_stem_stats_parts((int)N, (int)H, (int)W);
  w = check_stem_w(op, w);
  if (P == 0) return {};
  auto wp = at::empty({pdt_stem_conv_wprep_elems()}, w.options());
  auto y = at::empty({N, 64, OH, OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto part = at::empty({P * (2 * 64 + 1)}, x.options().dtype(at::kFloat));
  const int rc = pdt_stem_conv_fwd_stats(bf16_ptr(x), bf16_ptr(w), bf16_out(wp), bf16_out(y), part.data_ptr<float>(),
                                         (int)N, (int)H, (int)W, stream());
  TORCH_CHECK(rc == 0, "pdt_stem_conv_fwd_stats failed: ", rc);
  return {y, part};
}

// Weight gradient of stem_conv_fwd: dw [64, 3, 7, 7] (channels_last) from x and dy [N, 64, OH, OW]
// (channels_last); W % 32 == 0 and W <= 224.
Tensor stem_conv_wgrad(Tensor x, Tensor dy) {
  const Op op("stem_conv_wgrad", x);
  check_stem_x(op, x);
  TORCH_CHECK(x.size(3) <= 224, op.name, ": W <= 224");
  check_nhwc_bf16(op, "dy", dy);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == 64 && dy.size(2) == (H - 1) / 2 + 1 && dy.size(3) == W / 2,
              "stem_conv_wgrad: dy [N, 64, OH, OW]");
  auto ws = at::empty({pdt_stem_wgrad_ws_floats()}, x.options().dtype(at::kFloat));
  auto dw = at::empty({64, 3, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_stem_conv_wgrad(bf16_ptr(x), bf16_ptr(dy), bf16_out(dw), ws.data_ptr<float>(), (int)N, (int)H,
                                     (int)W, stream());
  TORCH_CHECK(rc == 0, "pdt_stem_conv_wgrad failed: ", rc);
  return dw;
}

// stem_conv_wgrad with the stem BatchNorm's backward apply fused into the gradient load: the conv's
// output gradient is A dz + B (xb - mean) + D (coef [3, 64] = A, B, D from maxpool3s2_bwd_bn_coef;
// xb: the BN input = the stem conv output, dz: the gradient at the BN output, both [N, 64, OH, OW]).
Tensor stem_conv_wgrad_bn(Tensor x, Tensor dz, Tensor xb, Tensor coef, Tensor mean) {
  const Op op("stem_conv_wgrad_bn", x);
  check_stem_x(op, x);
  TORCH_CHECK(x.size(3) <= 224, op.name, ": W <= 224");
  check_nhwc_bf16(op, "dz", dz);
  check_nhwc_bf16(op, "xb", xb);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(dz.size(0) == N && dz.size(1) == 64 && dz.size(2) == (H - 1) / 2 + 1 && dz.size(3) == W / 2,
              "stem_conv_wgrad_bn: dz [N, 64, OH, OW]");
  TORCH_CHECK(xb.sizes() == dz.sizes(), "stem_conv_wgrad_bn: xb shape");
  auto ws = at::empty({pdt_stem_wgrad_ws_floats()}, x.options().dtype(at::kFloat));
  auto dw = at::empty({64, 3, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_stem_conv_wgrad_bn(bf16_ptr(x), bf16_ptr(dz), bf16_ptr(xb), f32_ptr(op, "coef", coef, 3 * 64),
                                        f32_ptr(op, "mean", mean, 64), bf16_out(dw), ws.data_ptr<float>(), (int)N,
                                        (int)H, (int)W, stream());
  TORCH_CHECK(rc == 0, "pdt_stem_conv_wgrad_bn failed: ", rc);
  return dw;
}

// The same weight gradient from the gradient at the max-pool OUTPUT (dyp [N, 64, PH, PW]) and the pool's
// winner codes: the pool's input gradient dz is formed per tile inside the kernel, never in HBM.
Tensor stem_conv_wgrad_bn_pool(Tensor x, Tensor dyp, Tensor code, Tensor xb, Tensor coef, Tensor mean) {
  const Op op("stem_conv_wgrad_bn_pool", x);
  check_stem_x(op, x);
  TORCH_CHECK(x.size(3) <= 224, op.name, ": W <= 224");
  check_nhwc_bf16(op, "dyp", dyp);
  check_nhwc_bf16(op, "xb", xb);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3);
  const int64_t OH = (H - 1) / 2 + 1, OW = W / 2;
  TORCH_CHECK(xb.size(0) == N && xb.size(1) == 64 && xb.size(2) == OH && xb.size(3) == OW,
              "stem_conv_wgrad_bn_pool: xb [N, 64, OH, OW]");
  TORCH_CHECK(dyp.size(0) == N && dyp.size(1) == 64 && dyp.size(2) == (OH - 1) / 2 + 1 && dyp.size(3) == (OW - 1) / 2 + 1,
              "stem_conv_wgrad_bn_pool: dyp [N, 64, PH, PW]");
  auto ws = at::empty({pdt_stem_wgrad_ws_floats()}, x.options().dtype(at::kFloat));
  auto dw = at::empty({64, 3, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_stem_conv_wgrad_bn_pool(bf16_ptr(x), bf16_ptr(dyp), u8_ptr(op, "code", code, dyp.numel()),
                                             bf16_ptr(xb), f32_ptr(op, "coef", coef, 3 * 64),
                                             f32_ptr(op, "mean", mean, 64), bf16_out(dw), ws.data_ptr<float>(), (int)N,
                                             (int)H, (int)W, stream());
  TORCH_CHECK(rc == 0, "pdt_stem_conv_wgrad_bn_pool failed: ", rc);
  return dw;
}

// ----------------------------------------------------------------------------- cross entropy
std::vector<Tensor> ce_fwd(Tensor logits, Tensor target, double smoothing, int64_t ignore_index) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "ce: logits must be contiguous [N, V]");
  const int64_t N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(target.scalar_type() == at::kLong && target.is_contiguous() && target.numel() == N &&
                  target.device() == logits.device(), "ce: target must be int64 [N] on the logits' device");
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({N}, fopt), lse = at::empty({N}, fopt);
  pdt_ce_fwd(logits.data_ptr(), dcode(logits), target.data_ptr<int64_t>(), N, V, (float)smoothing, ignore_index,
             loss.data_ptr<float>(), lse.data_ptr<float>(), stream());
  return {loss, lse};
}

Tensor ce_bwd(Tensor logits, Tensor target, Tensor lse, c10::optional<Tensor> dloss, double dloss_scale,
              double smoothing, int64_t ignore_index) {
  const Op op("ce_bwd", logits);
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "ce: logits must be contiguous [N, V]");
  const int64_t N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(target.scalar_type() == at::kLong && target.is_contiguous() && target.numel() == N &&
                  target.device() == op.dev, "ce: target must be int64 [N] on the logits' device");
  auto dl = at::empty_like(logits);
  const float* dp = nullptr;
  Tensor dloss_c;
  if (has(dloss)) {
    dloss_c = dloss->to(at::kFloat).contiguous();
    if (dloss_c.numel() == 1) dloss_c = dloss_c.expand({N}).contiguous();
    dp = f32_ptr(op, "dloss", dloss_c, N);
  }
  pdt_ce_bwd(logits.data_ptr(), dcode(logits), target.data_ptr<int64_t>(), f32_ptr(op, "lse", lse, N), dp,
             (float)dloss_scale, N, V, (float)smoothing, ignore_index, dl.data_ptr(), stream());
  return dl;
}

// ----------------------------------------------------------------------------- layernorm
// res: optional residual branch; then the sum s = x + res is returned as a 4th output and normalised.
std::vector<Tensor> ln_fwd(Tensor x, Tensor w, Tensor b, double eps, c10::optional<Tensor> res) {
  const Op op("ln_fwd", x);
  TORCH_CHECK(x.is_contiguous(), "ln: x must be contiguous");
  const int64_t D = x.size(-1), N = x.numel() / D;
  const bool hr = has(res);
  if (hr)
    TORCH_CHECK(res->is_contiguous() && res->sizes() == x.sizes() && res->scalar_type() == x.scalar_type(),
                "ln: residual must match x (contiguous, same shape/dtype)");
  auto y = at::empty_like(x);
  Tensor sum;
  if (hr) sum = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({N}, fopt), rstd = at::empty({N}, fopt);
  int rc = pdt_ln_fwd(x.data_ptr(), hr ? res->data_ptr() : nullptr, dcode(x), f32_ptr(op, "w", w, D),
                      f32_ptr(op, "b", b, D), y.data_ptr(), hr ? sum.data_ptr() : nullptr, mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), N, (int)D, (float)eps, stream());
  TORCH_CHECK(rc == 0, "pdt_ln_fwd: unsupported D=", D);
  return {y, mean, rstd, sum};
}

// LayerNorm straight to fp8 for an fp8 GEMM (layernorm.hip ln_fwd_fp8_kernel): x bf16 [N, D]
// (+ res: s = x + res stored). Returns {yq [N, D], yq^T [D, N], mean, rstd, s}; state_row is the
// consuming GEMM's input-operand row (amax, scale, ...).
std::vector<Tensor> ln_fwd_fp8(Tensor x, Tensor w, Tensor b, double eps, c10::optional<Tensor> res, Tensor state_row) {
  const Op op("ln_fwd_fp8", x);
  TORCH_CHECK(x.is_contiguous() && x.scalar_type() == at::kBFloat16, "ln_fp8: x must be contiguous bf16");
  const int64_t D = x.size(-1), N = x.numel() / D;
  TORCH_CHECK(state_row.scalar_type() == at::kFloat && state_row.numel() >= 3 && state_row.is_contiguous(),
              "ln_fp8: fp32 state row");
  const bool hr = has(res);
  if (hr)
    TORCH_CHECK(res->is_contiguous() && res->sizes() == x.sizes() && res->scalar_type() == x.scalar_type(),
                "ln_fp8: residual must match x (contiguous, same shape/dtype)");
  auto o8 = x.options().dtype(at::kFloat8_e4m3fn);
  auto yq = at::empty({N, D}, o8), yqt = at::empty({D, N}, o8);
  Tensor sum;
  if (hr) sum = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({N}, fopt), rstd = at::empty({N}, fopt);
  float* st = state_row.data_ptr<float>();
  int rc = pdt_ln_fwd_fp8(bf16_ptr(x), hr ? bf16_ptr(*res) : nullptr, f32_ptr(op, "w", w, D), f32_ptr(op, "b", b, D),
                          ptr_or_null<uint16_t>(sum), byte_ptr(yq), byte_ptr(yqt), mean.data_ptr<float>(),
                          rstd.data_ptr<float>(), N, (int)D, (float)eps, st + 1, st, fp8_striped(state_row), stream());
  TORCH_CHECK(rc == 0, "pdt_ln_fwd_fp8: unsupported N=", N, " D=", D);
  return {yq, yqt, mean, rstd, sum};
}

// dres: optional gradient added into dx (the residual stream's own gradient).
std::vector<Tensor> ln_bwd(Tensor dy, Tensor x, Tensor w, Tensor mean, Tensor rstd, c10::optional<Tensor> dres) {
  const Op op("ln_bwd", x);
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(), "ln bwd: contiguous inputs required");
  const int64_t D = x.size(-1), N = x.numel() / D;
  const bool hr = has(dres);
  if (hr)
    TORCH_CHECK(dres->is_contiguous() && dres->sizes() == x.sizes() && dres->scalar_type() == x.scalar_type(),
                "ln bwd: dres must match x (contiguous, same shape/dtype)");
  auto dx = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto dw = at::empty({D}, fopt), db = at::empty({D}, fopt);
  auto ws = at::empty({std::max<int64_t>(pdt_ln_workspace_floats(N, (int)D), 1)}, fopt);
  int rc = pdt_ln_bwd(dy.data_ptr(), x.data_ptr(), hr ? dres->data_ptr() : nullptr, dcode(x), f32_ptr(op, "w", w, D),
                      f32_ptr(op, "mean", mean, N), f32_ptr(op, "rstd", rstd, N), dx.data_ptr(), dw.data_ptr<float>(),
                      db.data_ptr<float>(), N, (int)D, ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_ln_bwd: unsupported D=", D);
  return {dx, dw, db};
}

// ----------------------------------------------------------------------------- rmsnorm / rope / swiglu
bool aligned16(const Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

// A result: the caller's own tensor (`out`: checked against the shape / dtype / device the kernel writes), or a
// new one.
Tensor out_or_new(const Op& op, const char* name, const c10::optional<Tensor>& out, at::IntArrayRef shape,
                  const at::TensorOptions& opt) {
  if (!has(out)) return at::empty(shape, opt);
  TORCH_CHECK(out->is_contiguous() && out->sizes() == shape && out->scalar_type() == opt.dtype().toScalarType() &&
                  out->device() == op.dev && aligned16(*out),
              op.name, ": ", name, " must be a contiguous, 16-byte aligned ", opt.dtype(), " tensor of shape ", shape,
              " on ", op.dev);
  return *out;
}

// res: optional residual branch; then the sum s = x + res is returned as a 3rd output and normalised.
// {y, rstd, s}; y_out / rstd_out / sum_out: write into these instead of new tensors.
std::vector<Tensor> rms_fwd(Tensor x, Tensor w, double eps, c10::optional<Tensor> res, c10::optional<Tensor> y_out,
                            c10::optional<Tensor> rstd_out, c10::optional<Tensor> sum_out) {
  const Op op("rms_fwd", x);
  TORCH_CHECK(x.is_contiguous() && x.dim() >= 1 && aligned16(x), "rms_fwd: x must be contiguous and 16-byte aligned");
  const int64_t D = x.size(-1), N = D > 0 ? x.numel() / D : 0;
  const bool hr = has(res);
  if (hr)
    TORCH_CHECK(res->is_contiguous() && res->sizes() == x.sizes() && res->scalar_type() == x.scalar_type() &&
                    res->device() == op.dev && aligned16(*res),
                "rms_fwd: residual must match x (contiguous, same shape/dtype/device)");
  const int dt = dcode(x);
  const float* wp = f32_ptr(op, "w", w, D);
  TORCH_CHECK(hr || !has(sum_out), "rms_fwd: sum_out without a residual");
  auto y = out_or_new(op, "y_out", y_out, x.sizes(), x.options());
  Tensor sum;
  if (hr) sum = out_or_new(op, "sum_out", sum_out, x.sizes(), x.options());
  auto rstd = out_or_new(op, "rstd_out", rstd_out, {N}, x.options().dtype(at::kFloat));
  int rc = pdt_rms_fwd(x.data_ptr(), hr ? res->data_ptr() : nullptr, dt, wp, y.data_ptr(),
                       hr ? sum.data_ptr() : nullptr, rstd.data_ptr<float>(), N, (int)D, (float)eps, stream());
  TORCH_CHECK(rc == 0, "pdt_rms_fwd: unsupported D=", D);
  return {y, rstd, sum};
}

// RMSNorm straight to fp8 for an fp8 GEMM (rmsnorm.hip rms_fwd_fp8_kernel): x bf16 [..., D] (+ res: s = x + res
// stored). Returns {yq [N, D], yq^T [D, N], rstd, s}; state_row is the consuming GEMM's input-operand row.
// D = 256 K with K <= 6 and N % 16 == 0; anything else is refused.
std::vector<Tensor> rms_fwd_fp8(Tensor x, Tensor w, double eps, c10::optional<Tensor> res, Tensor state_row) {
  const Op op("rms_fwd_fp8", x);
  TORCH_CHECK(x.is_contiguous() && x.dim() >= 1 && x.scalar_type() == at::kBFloat16 && aligned16(x),
              "rms_fwd_fp8: x must be contiguous, 16-byte aligned bf16");
  const int64_t D = x.size(-1), N = D > 0 ? x.numel() / D : 0;
  TORCH_CHECK(D > 0 && D % 256 == 0 && D / 256 <= 6 && N % 16 == 0,
              "rms_fwd_fp8: unsupported N=", N, " D=", D, " (D = 256 K with K <= 6, N % 16 == 0)");
  const bool hr = has(res);
  if (hr)
    TORCH_CHECK(res->is_contiguous() && res->sizes() == x.sizes() && res->scalar_type() == x.scalar_type() &&
                    res->device() == op.dev && aligned16(*res),
                "rms_fwd_fp8: residual must match x (contiguous, same shape/dtype/device)");
  const float* wp = f32_ptr(op, "w", w, D);
  float* st = fp8_row_ptr(op, state_row);
  auto o8 = x.options().dtype(at::kFloat8_e4m3fn);
  auto yq = at::empty({N, D}, o8), yqt = at::empty({D, N}, o8);
  Tensor sum;
  if (hr) sum = at::empty_like(x);
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  int rc = pdt_rms_fwd_fp8(bf16_ptr(x), hr ? bf16_ptr(*res) : nullptr, wp, ptr_or_null<uint16_t>(sum), byte_ptr(yq),
                           byte_ptr(yqt), rstd.data_ptr<float>(), N, (int)D, (float)eps, st + 1, st,
                           fp8_striped(state_row), stream());
  TORCH_CHECK(rc == 0, "pdt_rms_fwd_fp8: unsupported N=", N, " D=", D);
  return {yq, yqt, rstd, sum};
}

// dres: optional gradient added into dx (the residual stream's own gradient). {dx, dw}
std::vector<Tensor> rms_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd, c10::optional<Tensor> dres,
                            c10::optional<Tensor> dx_out, c10::optional<Tensor> dw_out) {
  const Op op("rms_bwd", x);
  TORCH_CHECK(x.is_contiguous() && x.dim() >= 1 && aligned16(x), "rms_bwd: x must be contiguous and 16-byte aligned");
  const auto like_x = [&](const Tensor& t) {
    return t.is_contiguous() && t.sizes() == x.sizes() && t.scalar_type() == x.scalar_type() && t.device() == op.dev &&
           aligned16(t);
  };
  TORCH_CHECK(like_x(dy), "rms_bwd: dy must match x (contiguous, same shape/dtype/device)");
  const int64_t D = x.size(-1), N = D > 0 ? x.numel() / D : 0;
  const bool hr = has(dres);
  if (hr) TORCH_CHECK(like_x(*dres), "rms_bwd: dres must match x (contiguous, same shape/dtype/device)");
  const int dt = dcode(x);
  const float* wp = f32_ptr(op, "w", w, D);
  const float* rp = f32_ptr(op, "rstd", rstd, N);
  TORCH_CHECK(D > 0 && D % 256 == 0 && D <= 2048, "pdt_rms_bwd: unsupported D=", D);
  auto fopt = x.options().dtype(at::kFloat);
  auto dx = out_or_new(op, "dx_out", dx_out, x.sizes(), x.options());
  auto dw = out_or_new(op, "dw_out", dw_out, {D}, fopt);
  auto ws = at::empty({std::max<int64_t>(pdt_rms_workspace_floats(N, (int)D), 1)}, fopt);
  int rc = pdt_rms_bwd(dy.data_ptr(), x.data_ptr(), hr ? dres->data_ptr() : nullptr, dt, wp, rp, dx.data_ptr(),
                       dw.data_ptr<float>(), N, (int)D, ws.data_ptr<float>(), stream());
  TORCH_CHECK(rc == 0, "pdt_rms_bwd: unsupported D=", D);
  return {dx, dw};
}

// Rotary embedding in place on the Q and K thirds of qkv [B, T, 3 * heads * 64] bf16 (rope.hip); cos, sin
// fp32 [T_max, 32]. conj: rotate by -theta (the inverse, and the backward).
void rope_qkv(Tensor qkv, Tensor cos, Tensor sin, int64_t heads, bool conj) {
  const Op op("rope_qkv", qkv);
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "rope_qkv: qkv must be bf16, got ", qkv.scalar_type());
  TORCH_CHECK(qkv.dim() == 3 && qkv.stride(-1) == 1 && qkv.is_contiguous() && aligned16(qkv),
              "rope_qkv: qkv must be a contiguous [B, T, 3 * heads * 64] tensor (unit stride on the last dim)");
  const int64_t B = qkv.size(0), T = qkv.size(1);
  TORCH_CHECK(heads > 0 && qkv.size(2) == 3 * heads * 64, "rope_qkv: head dim must be 64: last dim ", qkv.size(2),
              " is not 3 * heads * 64 with heads = ", heads);
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 32 && sin.sizes() == cos.sizes(),
              "rope_qkv: cos and sin must be [T_max, 32] tables");
  const int64_t Tmax = cos.size(0);
  TORCH_CHECK(T <= Tmax, "rope_qkv: sequence length T = ", T, " exceeds the table's T_max = ", Tmax);
  const float* cp = f32_ptr(op, "cos", cos, Tmax * 32);
  const float* sp = f32_ptr(op, "sin", sin, Tmax * 32);
  TORCH_CHECK(aligned16(cos) && aligned16(sin), "rope_qkv: cos / sin must be 16-byte aligned");
  int rc = pdt_rope_qkv(bf16_out(qkv), cp, sp, (int)B, (int)T, (int)heads, conj ? 1 : 0, stream());
  TORCH_CHECK(rc == 0, "pdt_rope_qkv failed: ", rc);
}

// The grouped-query form: qkv [B, T, (heads + 2 * kv_heads) * 64], heads Q heads, then kv_heads K heads (both
// rotated), then kv_heads V heads (untouched).
void rope_qkv_gqa(Tensor qkv, Tensor cos, Tensor sin, int64_t heads, int64_t kv_heads, bool conj) {
  const Op op("rope_qkv_gqa", qkv);
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, "rope_qkv_gqa: qkv must be bf16, got ", qkv.scalar_type());
  TORCH_CHECK(qkv.dim() == 3 && qkv.stride(-1) == 1 && qkv.is_contiguous() && aligned16(qkv),
              "rope_qkv_gqa: qkv must be a contiguous [B, T, (heads + 2 * kv_heads) * 64] tensor");
  const int64_t B = qkv.size(0), T = qkv.size(1);
  TORCH_CHECK(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, "rope_qkv_gqa: heads = ", heads,
              " is not a positive multiple of kv_heads = ", kv_heads);
  TORCH_CHECK(qkv.size(2) == (heads + 2 * kv_heads) * 64, "rope_qkv_gqa: head dim must be 64: last dim ", qkv.size(2),
              " is not (heads + 2 * kv_heads) * 64 with heads = ", heads, ", kv_heads = ", kv_heads);
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 32 && sin.sizes() == cos.sizes(),
              "rope_qkv_gqa: cos and sin must be [T_max, 32] tables");
  const int64_t Tmax = cos.size(0);
  TORCH_CHECK(T <= Tmax, "rope_qkv_gqa: sequence length T = ", T, " exceeds the table's T_max = ", Tmax);
  const float* cp = f32_ptr(op, "cos", cos, Tmax * 32);
  const float* sp = f32_ptr(op, "sin", sin, Tmax * 32);
  TORCH_CHECK(aligned16(cos) && aligned16(sin), "rope_qkv_gqa: cos / sin must be 16-byte aligned");
  int rc = pdt_rope_qkv_gqa(bf16_out(qkv), cp, sp, (int)B, (int)T, (int)heads, (int)kv_heads, conj ? 1 : 0, stream());
  TORCH_CHECK(rc == 0, "pdt_rope_qkv_gqa failed: ", rc);
}

// ----------------------------------------------------------------------------- KV-cache decoding (attn_decode.hip)
// The checks the cache append and the decode attention share: qkv [B, Tn, (heads + 2 kv_heads) * 64] bf16,
// caches [B, kv_heads, capacity, 64] bf16 contiguous, lens int32 [B], all on the op's device.
struct DecodeDims {
  int B, Tn, H, Hkv, cap;
};
DecodeDims decode_dims(const Op& op, const Tensor& qkv, const Tensor& k_cache, const Tensor& v_cache,
                       const Tensor& lens, int64_t heads, int64_t kv_heads) {
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, op.name, ": qkv must be bf16, got ", qkv.scalar_type());
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous() && aligned16(qkv), op.name,
              ": qkv must be a contiguous, 16-byte aligned [B, Tn, (heads + 2 * kv_heads) * 64] tensor");
  TORCH_CHECK(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, op.name, ": heads = ", heads,
              " is not a positive multiple of kv_heads = ", kv_heads);
  TORCH_CHECK(qkv.size(2) == (heads + 2 * kv_heads) * 64, op.name, ": head dim must be 64: last dim ", qkv.size(2),
              " is not (heads + 2 * kv_heads) * 64 with heads = ", heads, ", kv_heads = ", kv_heads);
  for (const Tensor* c : {&k_cache, &v_cache}) {
    TORCH_CHECK(c->defined() && c->device() == op.dev && c->scalar_type() == at::kBFloat16, op.name,
                ": the caches must be bf16 tensors on ", op.dev);
    TORCH_CHECK(c->dim() == 4 && c->size(3) == 64, op.name, ": the caches must be [B, kv_heads, capacity, 64] ",
                "(head dim 64), got ", c->sizes());
    TORCH_CHECK(c->is_contiguous() && aligned16(*c), op.name, ": the caches must be contiguous and 16-byte aligned");
  }
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), op.name, ": k_cache and v_cache must have equal sizes");
  TORCH_CHECK(k_cache.size(0) == qkv.size(0) && k_cache.size(1) == kv_heads && k_cache.size(2) > 0, op.name,
              ": caches ", k_cache.sizes(), " do not match B = ", qkv.size(0), ", kv_heads = ", kv_heads);
  TORCH_CHECK(k_cache.size(2) * 128 <= 0x7fffffffLL, op.name, ": capacity too large");
  TORCH_CHECK(lens.defined() && lens.device() == op.dev && lens.scalar_type() == at::kInt && lens.is_contiguous() &&
                  lens.dim() == 1 && lens.size(0) == qkv.size(0),
              op.name, ": lens must be a contiguous int32 [B] tensor on ", op.dev);
  return {(int)qkv.size(0), (int)qkv.size(1), (int)heads, (int)kv_heads, (int)k_cache.size(2)};
}

// Rotate the query heads of qkv in place at positions lens[b] + t and write the rotated keys and the values
// of the Tn new tokens to the caches at those positions (a position outside the cache or the table writes nothing).
void rope_kv_append(Tensor qkv, Tensor cos, Tensor sin, int64_t heads, int64_t kv_heads, Tensor k_cache,
                    Tensor v_cache, Tensor lens) {
  const Op op("rope_kv_append", qkv);
  const DecodeDims d = decode_dims(op, qkv, k_cache, v_cache, lens, heads, kv_heads);
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 32 && sin.sizes() == cos.sizes(),
              "rope_kv_append: cos and sin must be [T_max, 32] tables");
  const int64_t Tmax = cos.size(0);
  const float* cp = f32_ptr(op, "cos", cos, Tmax * 32);
  const float* sp = f32_ptr(op, "sin", sin, Tmax * 32);
  TORCH_CHECK(Tmax > 0 && aligned16(cos) && aligned16(sin), "rope_kv_append: cos / sin must be 16-byte aligned");
  int rc = pdt_rope_kv_append(bf16_out(qkv), cp, sp, bf16_out(k_cache), bf16_out(v_cache), lens.data_ptr<int>(), d.B,
                              d.Tn, d.H, d.Hkv, d.cap, (int)Tmax, stream());
  TORCH_CHECK(rc == 0, "pdt_rope_kv_append failed: ", rc);
}

// (S, C) of the decode attention for a cache: S splits of C keys (attn_decode.hip pdt_attn_decode_geo).
// splits = 0: the default rule; group = heads / kv_heads.
std::vector<int64_t> attn_decode_geo(int64_t B, int64_t kv_heads, int64_t capacity, int64_t splits, int64_t group) {
  int g[2] = {0, 0};
  for (int64_t v : {B, kv_heads, capacity, splits, group})
    TORCH_CHECK(v >= 0 && v <= 0x7fffffffLL, "attn_decode_geo: argument ", v, " outside [0, 2^31)");
  int rc = pdt_attn_decode_geo((int)B, (int)kv_heads, (int)capacity, (int)splits, (int)group, g);
  TORCH_CHECK(rc == 0, "attn_decode_geo: bad arguments B = ", B, ", kv_heads = ", kv_heads, ", capacity = ", capacity,
              ", splits = ", splits, ", group = ", group);
  return {g[0], g[1]};
}

// Decode attention of one new token per sequence: qkv [B, 1, (heads + 2 kv_heads) * 64] with Q rotated, the
// caches already holding the token at position lens[b]. out [B, 1, heads * 64] bf16; lse (optional) fp32
// [B, heads]; o_part / ml_part: fp32 scratch of at least B * heads * S * 64 and B * heads * S * 2 elements (needed
// when S > 1). Returns (S, C), the geometry that ran.
std::vector<int64_t> attn_decode(Tensor qkv, Tensor k_cache, Tensor v_cache, Tensor lens, int64_t heads,
                                 int64_t kv_heads, double scale, int64_t splits, Tensor out,
                                 c10::optional<Tensor> o_part, c10::optional<Tensor> ml_part,
                                 c10::optional<Tensor> lse) {
  const Op op("attn_decode", qkv);
  const DecodeDims d = decode_dims(op, qkv, k_cache, v_cache, lens, heads, kv_heads);
  TORCH_CHECK(d.Tn == 1, "attn_decode: one new token per sequence, got Tn = ", d.Tn);
  TORCH_CHECK(scale > 0 && splits >= 0, "attn_decode: scale must be positive and splits >= 0");
  TORCH_CHECK(out.defined() && out.device() == op.dev && out.scalar_type() == at::kBFloat16 && out.is_contiguous() &&
                  out.numel() == (int64_t)d.B * d.H * 64 && aligned16(out),
              "attn_decode: out must be a contiguous bf16 [B, 1, heads * 64] tensor on ", op.dev);
  const std::vector<int64_t> geo = attn_decode_geo(d.B, d.Hkv, d.cap, splits, d.H / d.Hkv);
  const int64_t S = geo[0], rows = (int64_t)d.B * d.H;
  float* lp = opt_f32_ptr(op, "lse", lse, rows);
  float *op_ptr = nullptr, *ml_ptr = nullptr;
  if (S > 1) {
    TORCH_CHECK(has(o_part) && has(ml_part), "attn_decode: S = ", S, " splits need the o_part / ml_part scratch");
    for (const Tensor* t : {&*o_part, &*ml_part})
      TORCH_CHECK(t->device() == op.dev && t->scalar_type() == at::kFloat && t->is_contiguous() && aligned16(*t),
                  "attn_decode: the scratch must be contiguous, 16-byte aligned fp32 on ", op.dev);
    TORCH_CHECK(o_part->numel() >= rows * S * 64 && ml_part->numel() >= rows * S * 2, "attn_decode: scratch too small for S = ",
                S, ": o_part ", o_part->numel(), " < ", rows * S * 64, " or ml_part ", ml_part->numel(), " < ", rows * S * 2);
    op_ptr = o_part->data_ptr<float>();
    ml_ptr = ml_part->data_ptr<float>();
  }
  int rc = pdt_attn_decode(bf16_ptr(qkv), qkv.stride(0), bf16_ptr(k_cache), bf16_ptr(v_cache), lens.data_ptr<int>(),
                           op_ptr, ml_ptr, bf16_out(out), lp, d.B, d.H, d.Hkv, d.cap, (int)S, (int)geo[1], (float)scale,
                           stream());
  TORCH_CHECK(rc == 0, "pdt_attn_decode failed: ", rc);
  if (S > 1) {
    rc = pdt_attn_decode_combine(op_ptr, ml_ptr, bf16_out(out), lp, d.B, d.H, (int)S, stream());
    TORCH_CHECK(rc == 0, "pdt_attn_decode_combine failed: ", rc);
  }
  return geo;
}

// y = silu(gu[:, :F]) * gu[:, F:] for gu [..., 2F] (swiglu.hip)
Tensor swiglu_fwd(Tensor gu, c10::optional<Tensor> y_out) {
  const Op op("swiglu_fwd", gu);
  TORCH_CHECK(gu.is_contiguous() && gu.dim() >= 1 && aligned16(gu),
              "swiglu_fwd: gu must be contiguous and 16-byte aligned");
  const int64_t F2 = gu.size(-1), F = F2 / 2;
  TORCH_CHECK(F2 % 16 == 0 && F2 > 0, "swiglu_fwd: last dim 2F with F % 8 == 0, got ", F2);
  const int64_t N = gu.numel() / F2;
  auto shape = gu.sizes().vec();
  shape.back() = F;
  auto y = out_or_new(op, "y_out", y_out, shape, gu.options());
  int rc = pdt_swiglu_fwd(gu.data_ptr(), dcode(gu), y.data_ptr(), N, (int)F, stream());
  TORCH_CHECK(rc == 0, "pdt_swiglu_fwd failed: ", rc);
  return y;
}

// dgu = [dg | du] from dy [..., F] and the saved gu [..., 2F]
Tensor swiglu_bwd(Tensor dy, Tensor gu, c10::optional<Tensor> dgu_out) {
  const Op op("swiglu_bwd", gu);
  TORCH_CHECK(gu.is_contiguous() && gu.dim() >= 1 && aligned16(gu),
              "swiglu_bwd: gu must be contiguous and 16-byte aligned");
  const int64_t F2 = gu.size(-1), F = F2 / 2;
  TORCH_CHECK(F2 % 16 == 0 && F2 > 0, "swiglu_bwd: last dim 2F with F % 8 == 0, got ", F2);
  const int64_t N = gu.numel() / F2;
  TORCH_CHECK(dy.is_contiguous() && dy.scalar_type() == gu.scalar_type() && dy.device() == op.dev &&
                  dy.dim() == gu.dim() && dy.size(-1) == F && dy.numel() == N * F && aligned16(dy),
              "swiglu_bwd: dy must be contiguous [..., F] of gu's dtype on gu's device");
  auto dgu = out_or_new(op, "dgu_out", dgu_out, gu.sizes(), gu.options());
  int rc = pdt_swiglu_bwd(dy.data_ptr(), gu.data_ptr(), dcode(gu), dgu.data_ptr(), N, (int)F, stream());
  TORCH_CHECK(rc == 0, "pdt_swiglu_bwd failed: ", rc);
  return dgu;
}

// ----------------------------------------------------------------------------- dropout (philox.h)
const int64_t* ticket_ptr(const Tensor& ticket, const Tensor& like) {
  TORCH_CHECK(ticket.is_cuda() && ticket.scalar_type() == at::kLong && ticket.numel() == 2 && ticket.is_contiguous() &&
              ticket.device() == like.device(), "dropout: ticket must be an int64 [2] tensor on the data's device");
  return ticket.data_ptr<int64_t>();
}
int check_thr(int64_t thr) {
  TORCH_CHECK(thr >= 1 && thr <= 255, "dropout: threshold ", thr, " outside 1..255");
  return (int)thr;
}

// state = (key, step) -> a fresh ticket (key, step); step += 1. One launch, no host read: captured in a
// hipGraph, every replay advances.
Tensor dropout_begin(Tensor state) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.numel() == 2 && state.is_contiguous(),
              "dropout: state must be an int64 [2] GPU tensor (key, step)");
  auto ticket = at::empty({2}, state.options());
  pdt_dropout_begin(state.data_ptr<int64_t>(), ticket.data_ptr<int64_t>(), stream());
  return ticket;
}

// y = round_T(x * m * scale), flat mask layout; the backward is the same call on dy.
Tensor dropout_fwd(Tensor x, Tensor ticket, int64_t dstream, int64_t thr) {
  check_cuda(x, "x");
  TORCH_CHECK(x.is_contiguous() && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "dropout: x must be contiguous and 16-byte aligned");
  auto y = at::empty_like(x);
  int rc = pdt_dropout(x.data_ptr(), y.data_ptr(), dcode(x), x.numel(), ticket_ptr(ticket, x), (int)dstream,
                       check_thr(thr), stream());
  TORCH_CHECK(rc == 0, "pdt_dropout failed: ", rc);
  return y;
}

// The bool keep mask the kernels apply: kind "flat" (any shape, element order) or "attn" ([B, H, T, T]).
Tensor dropout_mask(Tensor ticket, int64_t dstream, std::vector<int64_t> shape, int64_t thr, std::string kind) {
  TORCH_CHECK(thr >= 0 && thr <= 255, "dropout: threshold ", thr, " outside 0..255");
  auto out = at::empty(shape, ticket.options().dtype(at::kBool));
  const int64_t* tp = ticket_ptr(ticket, out);
  int rc;
  if (kind == "flat") {
    rc = pdt_dropout_mask_flat(byte_ptr(out), out.numel(), tp, (int)dstream, (int)thr, stream());
  } else {
    TORCH_CHECK(kind == "attn" && shape.size() == 4 && shape[2] == shape[3], "dropout_mask: attn wants [B, H, T, T]");
    rc = pdt_dropout_mask_attn(byte_ptr(out), shape[0] * shape[1], (int)shape[2], tp, (int)dstream, (int)thr, stream());
  }
  TORCH_CHECK(rc == 0, "pdt_dropout_mask failed: ", rc);
  return out;
}

// s = x + dropout(res), y = LN(s): {y, mean, rstd, s}
std::vector<Tensor> ln_fwd_drop(Tensor x, Tensor w, Tensor b, double eps, Tensor res, Tensor ticket, int64_t dstream,
                                int64_t thr) {
  const Op op("ln_fwd_drop", x);
  TORCH_CHECK(x.is_contiguous(), "ln: x must be contiguous");
  const int64_t D = x.size(-1), N = x.numel() / D;
  TORCH_CHECK(res.is_contiguous() && res.sizes() == x.sizes() && res.scalar_type() == x.scalar_type(),
              "ln: residual must match x (contiguous, same shape/dtype)");
  auto y = at::empty_like(x), sum = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({N}, fopt), rstd = at::empty({N}, fopt);
  int rc = pdt_ln_fwd_drop(x.data_ptr(), res.data_ptr(), dcode(x), f32_ptr(op, "w", w, D), f32_ptr(op, "b", b, D),
                           y.data_ptr(), sum.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(), N, (int)D,
                           (float)eps, ticket_ptr(ticket, x), (int)dstream, check_thr(thr), stream());
  TORCH_CHECK(rc == 0, "pdt_ln_fwd_drop: unsupported D=", D);
  return {y, mean, rstd, sum};
}

// {dx, dh, dw, db}: dx as ln_bwd, dh = the dropout backward of dx (the dropped branch's gradient)
std::vector<Tensor> ln_bwd_drop(Tensor dy, Tensor x, Tensor w, Tensor mean, Tensor rstd, c10::optional<Tensor> dres,
                                Tensor ticket, int64_t dstream, int64_t thr) {
  const Op op("ln_bwd_drop", x);
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(), "ln bwd: contiguous inputs required");
  const int64_t D = x.size(-1), N = x.numel() / D;
  const bool hr = has(dres);
  if (hr)
    TORCH_CHECK(dres->is_contiguous() && dres->sizes() == x.sizes() && dres->scalar_type() == x.scalar_type(),
                "ln bwd: dres must match x (contiguous, same shape/dtype)");
  auto dx = at::empty_like(x), dh = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto dw = at::empty({D}, fopt), db = at::empty({D}, fopt);
  auto ws = at::empty({std::max<int64_t>(pdt_ln_workspace_floats(N, (int)D), 1)}, fopt);
  int rc = pdt_ln_bwd_drop(dy.data_ptr(), x.data_ptr(), hr ? dres->data_ptr() : nullptr, dcode(x),
                           f32_ptr(op, "w", w, D), f32_ptr(op, "mean", mean, N), f32_ptr(op, "rstd", rstd, N),
                           dx.data_ptr(), dh.data_ptr(), dw.data_ptr<float>(), db.data_ptr<float>(), N, (int)D,
                           ws.data_ptr<float>(), ticket_ptr(ticket, x), (int)dstream, check_thr(thr), stream());
  TORCH_CHECK(rc == 0, "pdt_ln_bwd_drop: unsupported D=", D);
  return {dx, dh, dw, db};
}

// ----------------------------------------------------------------------------- bias + gelu
Tensor bias_gelu_fwd(Tensor x, c10::optional<Tensor> bias, bool tanh_form) {
  TORCH_CHECK(x.is_contiguous(), "gelu: x must be contiguous");
  const int64_t D = x.size(-1), N = x.numel() / D;
  auto y = at::empty_like(x);
  const bool hb = has(bias);
  const bool bb = hb && bias->scalar_type() == at::kBFloat16;  // a bf16 model's bias, read as is
  if (hb) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == D && (bb || bias->scalar_type() == at::kFloat),
                "bias_gelu: bias [D] fp32 or bf16");
  }
  int rc = pdt_bias_gelu_fwd(x.data_ptr(), dcode(x), hb ? bias->data_ptr() : nullptr, y.data_ptr(), N, (int)D,
                             tanh_form, stream(), bb ? 1 : 0);
  TORCH_CHECK(rc == 0, "pdt_bias_gelu_fwd failed");
  return y;
}

std::vector<Tensor> bias_gelu_bwd(Tensor dy, Tensor x, c10::optional<Tensor> bias, bool tanh_form) {
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(), "gelu bwd: contiguous inputs required");
  const int64_t D = x.size(-1), N = x.numel() / D;
  auto dx = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  const bool hb = has(bias);
  const bool bb = hb && bias->scalar_type() == at::kBFloat16;
  Tensor db, ws;
  if (hb) {
    db = at::empty({D}, bb ? x.options().dtype(at::kBFloat16) : fopt);  // the bias's own dtype
    ws = at::empty({pdt_gelu_workspace_floats(N, (int)D)}, fopt);
  }
  int rc = pdt_bias_gelu_bwd(dy.data_ptr(), x.data_ptr(), dcode(x), hb ? bias->data_ptr() : nullptr, dx.data_ptr(),
                             hb ? db.data_ptr() : nullptr, N, (int)D, tanh_form,
                             ptr_or_null<float>(ws), stream(), bb ? 1 : 0);
  TORCH_CHECK(rc == 0, "pdt_bias_gelu_bwd failed");
  return {dx, db};
}

// ----------------------------------------------------------------------------- flash attention
// Views are [B, H, T, Dh] bf16 with unit stride on Dh (any b/h/t strides, e.g. slices of a packed qkv).
struct Strides3 {
  int64_t v[3];
};
Strides3 bht_strides(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 4 && t.stride(3) == 1, "attn: ", name,
              " must be a bf16 [B,H,T,Dh] view with unit Dh stride");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && t.stride(2) % 8 == 0 && t.stride(1) % 8 == 0,
              "attn: ", name, " rows must be 16-byte aligned");
  return {{t.stride(0), t.stride(1), t.stride(2)}};
}

void attn_fwd_out(Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, double scale) {
  auto qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"), os = bht_strides(o, "o");
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes() && q.sizes() == o.sizes(), "attn: shape mismatch");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == q.size(0) * q.size(1) * q.size(2),
              "attn: lse must be fp32 [B,H,T]");
  const int B = q.size(0), H = q.size(1), T = q.size(2), Dh = q.size(3);
  int rc = pdt_attn_fwd(bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v, bf16_out(o), os.v,
                        lse.data_ptr<float>(), B, H, T, Dh, causal, (float)scale, stream());
  TORCH_CHECK(rc == 0, "pdt_attn_fwd: unsupported head dim ", Dh);
}

void attn_bwd_out(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor dq, Tensor dk, Tensor dv,
                  bool causal, double scale) {
  auto dos = bht_strides(dout, "dout"), qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"),
       os = bht_strides(o, "o"), gs = bht_strides(dq, "dq"), gk = bht_strides(dk, "dk"), gv = bht_strides(dv, "dv");
  TORCH_CHECK(gs.v[0] == gk.v[0] && gs.v[1] == gk.v[1] && gs.v[2] == gk.v[2] && gs.v[0] == gv.v[0] &&
              gs.v[1] == gv.v[1] && gs.v[2] == gv.v[2], "attn bwd: dq/dk/dv must share strides");
  const int B = q.size(0), H = q.size(1), T = q.size(2), Dh = q.size(3);
  auto delta = at::empty({(int64_t)B * H * T}, q.options().dtype(at::kFloat));
  int rc = pdt_attn_bwd(bf16_ptr(dout), dos.v, bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v, bf16_ptr(o),
                        os.v, lse.data_ptr<float>(), delta.data_ptr<float>(), bf16_out(dq), bf16_out(dk), bf16_out(dv),
                        gs.v, B, H, T, Dh, causal, (float)scale, stream());
  TORCH_CHECK(rc == 0, "pdt_attn_bwd: unsupported head dim ", Dh);
}

// Grouped-query attention (attention.hip GQA): q/o/dout/dq [B, H, T, Dh], k/v/dk/dv [B, Hkv, T, Dh] with
// H % Hkv == 0; query head h reads K/V head h / (H / Hkv). Every check runs before any launch.
struct GqaDims {
  int B, H, Hkv, T, Dh;
};
GqaDims gqa_dims(const char* what, const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& lse) {
  TORCH_CHECK(k.sizes() == v.sizes(), what, ": k and v must have equal sizes, got ", k.sizes(), " and ", v.sizes());
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2) && k.size(3) == q.size(3), what,
              ": k/v must match q in B, T and Dh, got q ", q.sizes(), " and k ", k.sizes());
  TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0, what, ": the ", q.size(1),
              " query heads are not a multiple of the ", k.size(1), " K/V heads");
  TORCH_CHECK(q.size(3) == 64, what, ": unsupported head dim ", q.size(3));
  check_cuda(lse, "lse");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.dim() == 3 && lse.size(0) == q.size(0) &&
              lse.size(1) == q.size(1) && lse.size(2) == q.size(2), what, ": lse must be fp32 [B,H,T]");
  return {(int)q.size(0), (int)q.size(1), (int)k.size(1), (int)q.size(2), (int)q.size(3)};
}

void attn_fwd_gqa_out(Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, double scale) {
  auto qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"), os = bht_strides(o, "o");
  TORCH_CHECK(q.sizes() == o.sizes(), "attn gqa: o must have q's shape");
  const GqaDims d = gqa_dims("attn gqa", q, k, v, lse);
  int rc = pdt_attn_fwd_gqa(bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v, bf16_out(o), os.v,
                            lse.data_ptr<float>(), d.B, d.H, d.Hkv, d.T, d.Dh, causal, (float)scale, stream());
  TORCH_CHECK(rc == 0, "pdt_attn_fwd_gqa failed: ", rc);
}

void attn_bwd_gqa_out(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor dq, Tensor dk, Tensor dv,
                      bool causal, double scale) {
  auto dos = bht_strides(dout, "dout"), qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"),
       os = bht_strides(o, "o"), gs = bht_strides(dq, "dq"), gk = bht_strides(dk, "dk"), gv = bht_strides(dv, "dv");
  TORCH_CHECK(gs.v[0] == gk.v[0] && gs.v[1] == gk.v[1] && gs.v[2] == gk.v[2] && gs.v[0] == gv.v[0] &&
              gs.v[1] == gv.v[1] && gs.v[2] == gv.v[2], "attn gqa bwd: dq/dk/dv must share strides");
  TORCH_CHECK(q.sizes() == o.sizes() && q.sizes() == dout.sizes() && q.sizes() == dq.sizes() &&
              k.sizes() == dk.sizes() && v.sizes() == dv.sizes(), "attn gqa bwd: shape mismatch");
  const GqaDims d = gqa_dims("attn gqa bwd", q, k, v, lse);
  auto delta = at::empty({(int64_t)d.B * d.H * d.T}, q.options().dtype(at::kFloat));
  int rc = pdt_attn_bwd_gqa(bf16_ptr(dout), dos.v, bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v,
                            bf16_ptr(o), os.v, lse.data_ptr<float>(), delta.data_ptr<float>(), bf16_out(dq),
                            bf16_out(dk), bf16_out(dv), gs.v, d.B, d.H, d.Hkv, d.T, d.Dh, causal, (float)scale,
                            stream());
  TORCH_CHECK(rc == 0, "pdt_attn_bwd_gqa failed: ", rc);
}

// Attention dropout: the same calls with the mask of P regenerated from the ticket (attention.hip DROP).
void attn_fwd_drop_out(Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, double scale, Tensor ticket,
                       int64_t dstream, int64_t thr) {
  auto qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"), os = bht_strides(o, "o");
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes() && q.sizes() == o.sizes(), "attn: shape mismatch");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == q.size(0) * q.size(1) * q.size(2),
              "attn: lse must be fp32 [B,H,T]");
  const int B = q.size(0), H = q.size(1), T = q.size(2), Dh = q.size(3);
  int rc = pdt_attn_fwd_drop(bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v, bf16_out(o), os.v,
                             lse.data_ptr<float>(), B, H, T, Dh, causal, (float)scale, ticket_ptr(ticket, q),
                             (int)dstream, check_thr(thr), stream());
  TORCH_CHECK(rc == 0, "pdt_attn_fwd_drop: unsupported head dim ", Dh);
}

void attn_bwd_drop_out(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor dq, Tensor dk, Tensor dv,
                       bool causal, double scale, Tensor ticket, int64_t dstream, int64_t thr) {
  auto dos = bht_strides(dout, "dout"), qs = bht_strides(q, "q"), ks = bht_strides(k, "k"), vs = bht_strides(v, "v"),
       os = bht_strides(o, "o"), gs = bht_strides(dq, "dq"), gk = bht_strides(dk, "dk"), gv = bht_strides(dv, "dv");
  TORCH_CHECK(gs.v[0] == gk.v[0] && gs.v[1] == gk.v[1] && gs.v[2] == gk.v[2] && gs.v[0] == gv.v[0] &&
              gs.v[1] == gv.v[1] && gs.v[2] == gv.v[2], "attn bwd: dq/dk/dv must share strides");
  TORCH_CHECK(q.sizes() == k.sizes() && q.sizes() == v.sizes() && q.sizes() == o.sizes() && q.sizes() == dout.sizes() &&
              q.sizes() == dq.sizes() && q.sizes() == dk.sizes() && q.sizes() == dv.sizes(), "attn bwd: shape mismatch");
  const int B = q.size(0), H = q.size(1), T = q.size(2), Dh = q.size(3);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() && lse.numel() == (int64_t)B * H * T,
              "attn bwd: lse must be fp32 [B,H,T]");
  auto delta = at::empty({(int64_t)B * H * T}, q.options().dtype(at::kFloat));
  int rc = pdt_attn_bwd_drop(bf16_ptr(dout), dos.v, bf16_ptr(q), qs.v, bf16_ptr(k), ks.v, bf16_ptr(v), vs.v,
                             bf16_ptr(o), os.v, lse.data_ptr<float>(), delta.data_ptr<float>(), bf16_out(dq),
                             bf16_out(dk), bf16_out(dv), gs.v, B, H, T, Dh, causal, (float)scale, ticket_ptr(ticket, q),
                             (int)dstream, check_thr(thr), stream());
  TORCH_CHECK(rc == 0, "pdt_attn_bwd_drop: unsupported head dim ", Dh);
}

// bias gradient of a Linear layer: column sum of dy [*, D] -> [D] in out_dtype (fp32 / bf16)
// xs = x[:, :, ::s, ::s] for a channels_last bf16 [N, C, H, W] tensor (C % 8 == 0), channels_last out.
Tensor subsample_gather(Tensor x, int64_t s) {
  const Op op("subsample_gather", x);
  check_nhwc_bf16(op, "x", x);
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C % 8 == 0 && s >= 1, "subsample_gather: C % 8 == 0, s >= 1");
  auto xs = at::empty({N, C, (H - 1) / s + 1, (W - 1) / s + 1}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int rc = pdt_subsample_gather(bf16_ptr(x), bf16_out(xs), (int)N, (int)H, (int)W, (int)C, (int)s, stream());
  TORCH_CHECK(rc == 0, "pdt_subsample_gather failed: ", rc);
  return xs;
}

// full[:, :, ::s, ::s] += t (in place; both channels_last bf16).
void subsample_scatter_add(Tensor t, Tensor full, int64_t s) {
  const Op op("subsample_scatter_add", t);
  check_nhwc_bf16(op, "t", t);
  check_nhwc_bf16(op, "full", full);
  const int64_t N = full.size(0), C = full.size(1), H = full.size(2), W = full.size(3);
  TORCH_CHECK(t.size(0) == N && t.size(1) == C && t.size(2) == (H - 1) / s + 1 && t.size(3) == (W - 1) / s + 1 &&
              C % 8 == 0, "subsample_scatter_add: shape");
  const int rc = pdt_subsample_scatter_add(bf16_ptr(t), bf16_out(full), (int)N, (int)H, (int)W, (int)C, (int)s,
                                           stream());
  TORCH_CHECK(rc == 0, "pdt_subsample_scatter_add failed: ", rc);
}

// out = x.sum(0) for a contiguous bf16 [S, ...] tensor (S = 2..64, a power of two), fp32 accumulation.
Tensor slice_sum(Tensor x) {
  check_cuda(x, "slice_sum");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous() && x.dim() >= 2, "slice_sum: contiguous bf16 [S, ...]");
  const int64_t S = x.size(0), n = x.numel() / S;
  auto out = at::empty(x.sizes().slice(1), x.options());
  const int rc = pdt_slice_sum_bf16(bf16_ptr(x), bf16_out(out), (int)S, n, stream());
  TORCH_CHECK(rc == 0, "pdt_slice_sum_bf16 failed: ", rc);
  return out;
}

Tensor colsum(Tensor dy, at::ScalarType out_dtype) {
  check_cuda(dy, "dy");
  TORCH_CHECK(dy.is_contiguous(), "colsum: contiguous input");
  const int64_t D = dy.size(-1), N = D ? dy.numel() / D : 0;
  auto out = at::empty({D}, dy.options().dtype(out_dtype));
  auto ws = at::empty({std::max<int64_t>(pdt_gelu_workspace_floats(N, (int)D), 1)}, dy.options().dtype(at::kFloat));
  int rc = pdt_colsum(dy.data_ptr(), dcode(dy), N, (int)D, out.data_ptr(), dcode(out), ws.data_ptr<float>(),
                      stream());
  TORCH_CHECK(rc == 0, "pdt_colsum failed (D % 8 != 0?)");
  return out;
}

// ---- fp8 (OCP e4m3fn) casts: csrc/kernels/fp8.hip ----
// x: bf16 [M, K] contiguous; state_row: fp32 view [3 + L] = (amax, scale, scale_inv, history...)
// returns {x_fp8 [M, K], x_fp8_t [K, M] (if transpose)}
std::vector<Tensor> fp8_cast_transpose(Tensor x, Tensor state_row, bool transpose) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.is_contiguous(), "fp8_cast: bf16 [M, K]");
  TORCH_CHECK(state_row.scalar_type() == at::kFloat && state_row.numel() >= 3 && state_row.is_contiguous(),
              "fp8_cast: fp32 state row");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M % 16 == 0 && K % 16 == 0, "fp8_cast: M and K must be multiples of 16");
  auto o8 = x.options().dtype(at::kFloat8_e4m3fn);
  auto out = at::empty({M, K}, o8);
  Tensor out_t;
  if (transpose) out_t = at::empty({K, M}, o8);
  float* st = state_row.data_ptr<float>();
  int rc = pdt_fp8_cast_transpose(bf16_ptr(x), M, K, st + 1, byte_ptr(out), transpose ? byte_ptr(out_t) : nullptr, st,
                                  fp8_striped(state_row), stream());
  TORCH_CHECK(rc == 0, "pdt_fp8_cast_transpose failed");
  return {out, out_t};
}

// The MLP activation straight to fp8 (fp8.hip fp8_gelu_cast_kernel). h: bf16 [M, D] (fc1 output
// without bias), bias: fp32 [D] or none. Forward (dg undefined): {fp8(gelu(h + bias)), its
// transpose}. Backward: {fp8(dg * gelu'(h + bias)), its transpose, bias gradient in db_dtype (or
// undefined without bias)}. state_row as fp8_cast_transpose.
std::vector<Tensor> fp8_gelu_cast(Tensor h, c10::optional<Tensor> dg, c10::optional<Tensor> bias, Tensor state_row,
                                  bool tanh_form, at::ScalarType db_dtype) {
  check_cuda(h, "h");
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && h.dim() == 2 && h.is_contiguous(), "fp8_gelu_cast: bf16 [M, D] h");
  TORCH_CHECK(state_row.scalar_type() == at::kFloat && state_row.numel() >= 3 && state_row.is_contiguous(),
              "fp8_gelu_cast: fp32 state row");
  const int64_t M = h.size(0), D = h.size(1);
  TORCH_CHECK(M % 16 == 0 && D % 64 == 0 && M > 0, "fp8_gelu_cast: M % 16 == 0 and D % 64 == 0");
  const bool bwd = has(dg);
  if (bwd)
    TORCH_CHECK(dg->scalar_type() == at::kBFloat16 && dg->sizes() == h.sizes() && dg->is_contiguous(),
                "fp8_gelu_cast: dg like h");
  const bool hb = has(bias);
  if (hb)
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous() && bias->numel() == D,
                "fp8_gelu_cast: fp32 bias [D]");
  auto o8 = h.options().dtype(at::kFloat8_e4m3fn);
  auto out = at::empty({M, D}, o8), out_t = at::empty({D, M}, o8);
  Tensor part, db;
  if (bwd) part = at::empty({pdt_fp8_gelu_cast_workspace_floats(M, (int)D)}, h.options().dtype(at::kFloat));
  float* st = state_row.data_ptr<float>();
  const int nchunk = pdt_fp8_gelu_cast(bf16_ptr(h), bwd ? bf16_ptr(*dg) : nullptr,
                                       hb ? bias->data_ptr<float>() : nullptr, M, (int)D, tanh_form, st + 1,
                                       byte_ptr(out), byte_ptr(out_t), st, ptr_or_null<float>(part),
                                       fp8_striped(state_row), stream());
  TORCH_CHECK(nchunk > 0, "pdt_fp8_gelu_cast failed: ", nchunk);
  if (bwd && hb) {
    TORCH_CHECK(db_dtype == at::kFloat || db_dtype == at::kBFloat16, "fp8_gelu_cast: db dtype fp32 / bf16");
    db = at::empty({D}, h.options().dtype(db_dtype));
    pdt_colsum_finalize(part.data_ptr<float>(), nchunk, (int)D, db.data_ptr(), db_dtype == at::kFloat ? 0 : 1,
                        stream());
  }
  return {out, out_t, db};
}

// A Linear's output gradient dy (bf16 [M, D], D % 64 == 0): {fp8(dy), its transpose, sum_m dy in
// db_dtype} in one pass (fp8.hip M_CAST_SUM) — the cast and the bias gradient.
std::vector<Tensor> fp8_cast_colsum(Tensor x, Tensor state_row, at::ScalarType db_dtype) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.is_contiguous(), "fp8_cast_colsum: bf16 [M, D]");
  TORCH_CHECK(state_row.scalar_type() == at::kFloat && state_row.numel() >= 3 && state_row.is_contiguous(),
              "fp8_cast_colsum: fp32 state row");
  TORCH_CHECK(db_dtype == at::kFloat || db_dtype == at::kBFloat16, "fp8_cast_colsum: db dtype fp32 / bf16");
  const int64_t M = x.size(0), D = x.size(1);
  TORCH_CHECK(M % 16 == 0 && D % 64 == 0 && M > 0, "fp8_cast_colsum: M % 16 == 0 and D % 64 == 0");
  auto o8 = x.options().dtype(at::kFloat8_e4m3fn);
  auto out = at::empty({M, D}, o8), out_t = at::empty({D, M}, o8);
  auto part = at::empty({pdt_fp8_gelu_cast_workspace_floats(M, (int)D)}, x.options().dtype(at::kFloat));
  auto db = at::empty({D}, x.options().dtype(db_dtype));
  float* st = state_row.data_ptr<float>();
  const int nchunk = pdt_fp8_cast_colsum(bf16_ptr(x), M, (int)D, st + 1, byte_ptr(out), byte_ptr(out_t), st,
                                         part.data_ptr<float>(), fp8_striped(state_row), stream());
  TORCH_CHECK(nchunk > 0, "pdt_fp8_cast_colsum failed: ", nchunk);
  pdt_colsum_finalize(part.data_ptr<float>(), nchunk, (int)D, db.data_ptr(), db_dtype == at::kFloat ? 0 : 1, stream());
  return {out, out_t, db};
}

// The Llama MLP activation straight to fp8 (fp8.hip fp8_swiglu_cast_kernel). gu: bf16 [M, 2F] = [gate | up]
// (c_fc's output). Forward (dy undefined): {fp8(silu(gate) up) [M, F], its transpose [F, M]}. Backward (dy bf16
// [M, F]): {fp8([dgate | dup]) [M, 2F], its transpose [2F, M]}. F % 64 == 0 and M % 16 == 0; anything else is
// refused. state_row as fp8_cast_transpose.
std::vector<Tensor> fp8_swiglu_cast(Tensor gu, c10::optional<Tensor> dy, Tensor state_row) {
  const Op op("fp8_swiglu_cast", gu);
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 && gu.dim() == 2 && gu.is_contiguous() && aligned16(gu) &&
                  gu.size(1) % 2 == 0,
              "fp8_swiglu_cast: gu must be a contiguous, 16-byte aligned bf16 [M, 2F] tensor");
  const int64_t M = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(M > 0 && M % 16 == 0 && F > 0 && F % 64 == 0 && F <= 0x7fffffffLL,
              "fp8_swiglu_cast: unsupported M=", M, " F=", F, " (M % 16 == 0 and F % 64 == 0)");
  const bool bwd = has(dy);
  if (bwd)
    TORCH_CHECK(dy->scalar_type() == at::kBFloat16 && dy->dim() == 2 && dy->size(0) == M && dy->size(1) == F &&
                    dy->is_contiguous() && dy->device() == op.dev && aligned16(*dy),
                "fp8_swiglu_cast: dy must be a contiguous, 16-byte aligned bf16 [M, F] tensor on gu's device");
  float* st = fp8_row_ptr(op, state_row);
  auto o8 = gu.options().dtype(at::kFloat8_e4m3fn);
  const int64_t W = bwd ? 2 * F : F;
  auto out = at::empty({M, W}, o8), out_t = at::empty({W, M}, o8);
  const int nchunk = pdt_fp8_swiglu_cast(bf16_ptr(gu), bwd ? bf16_ptr(*dy) : nullptr, M, (int)F, st + 1, byte_ptr(out),
                                         byte_ptr(out_t), st, fp8_striped(state_row), stream());
  TORCH_CHECK(nchunk > 0, "pdt_fp8_swiglu_cast failed: ", nchunk);
  return {out, out_t};
}

// Every tensor of xs (bf16 [M_i, K_i] contiguous) cast with its state row in one launch (<= 64 per
// launch): returns [q_0, qt_0, q_1, qt_1, ...].
std::vector<Tensor> fp8_cast_multi(std::vector<Tensor> xs, std::vector<Tensor> rows) {
  TORCH_CHECK(xs.size() == rows.size(), "fp8_cast_multi: one state row per tensor");
  std::vector<Tensor> res;
  res.reserve(2 * xs.size());
  for (size_t base = 0; base < xs.size(); base += 64) {
    const int n = (int)std::min<size_t>(64, xs.size() - base);
    std::vector<const uint16_t*> px(n);
    std::vector<int> pm(n), pk(n), pst(n);
    std::vector<float*> ps(n);
    std::vector<uint8_t*> po(n), pt(n);
    for (int i = 0; i < n; ++i) {
      const Tensor& x = xs[base + i];
      const Tensor& r = rows[base + i];
      check_cuda(x, "x");
      TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.is_contiguous(), "fp8_cast_multi: bf16 [M, K]");
      TORCH_CHECK(r.scalar_type() == at::kFloat && r.numel() >= 3 && r.is_contiguous(), "fp8_cast_multi: state row");
      const int64_t M = x.size(0), K = x.size(1);
      TORCH_CHECK(M % 16 == 0 && K % 16 == 0 && M > 0 && M * K < ((int64_t)1 << 31), "fp8_cast_multi: shape");
      auto o8 = x.options().dtype(at::kFloat8_e4m3fn);
      res.push_back(at::empty({M, K}, o8));
      res.push_back(at::empty({K, M}, o8));
      px[i] = bf16_ptr(x);
      pm[i] = (int)M;
      pk[i] = (int)K;
      ps[i] = r.data_ptr<float>();
      pst[i] = fp8_striped(r);
      po[i] = byte_ptr(res[res.size() - 2]);
      pt[i] = byte_ptr(res.back());
    }
    const int rc = pdt_fp8_cast_multi(n, px.data(), pm.data(), pk.data(), ps.data(), pst.data(), po.data(), pt.data(),
                                      stream());
    TORCH_CHECK(rc == 0, "pdt_fp8_cast_multi failed: ", rc);
  }
  return res;
}

void fp8_update_scales(Tensor state, int64_t history, double margin) {
  check_cuda(state, "state");
  const bool striped = state.dim() == 2 && state.size(1) == pdt::kAmaxHist + history;
  TORCH_CHECK(state.scalar_type() == at::kFloat && state.is_contiguous() && state.dim() == 2 &&
                  (state.size(1) == 3 + history || striped),
              "fp8_update_scales: state [n, 3 + L] or striped [n, 260 + L] fp32");
  pdt_fp8_update_scales(state.data_ptr<float>(), (int)state.size(0), (int)history, (float)std::pow(2.0, margin),
                        striped ? 1 : 0, stream());
}

// ---- intra-node P2P all-reduce (csrc/kernels/p2p.hip) ----
#define PDT_HIP_CHECK(expr)                                                            \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    TORCH_CHECK(e_ == hipSuccess, "pdt p2p: ", #expr, " failed: ", hipGetErrorString(e_)); \
  } while (0)

struct DevGuard {  // select `dev` for the scope, restore the caller's device after
  int prev = 0;
  explicit DevGuard(int dev) {
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
  }
  ~DevGuard() { (void)hipSetDevice(prev); }
};

class P2PComm {
 public:
  P2PComm(int rank, int world, int64_t capacity_bytes, int max_blocks, int device)
      : rank_(rank), world_(world), cap_(capacity_bytes), max_blocks_(max_blocks), device_(device) {
    TORCH_CHECK(world >= 1 && world <= 8 && rank >= 0 && rank < world, "p2p: 1 <= world <= 8");
    TORCH_CHECK(capacity_bytes % 16 == 0, "p2p: capacity must be a multiple of 16 bytes");
    DevGuard guard(device_);
    flags_bytes_ = pdt_p2p_flags_bytes();
    // uncached: peers poll/read these over xGMI; no stale L2 lines on either side
    PDT_HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&flags_), flags_bytes_, hipDeviceMallocUncached));
    PDT_HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&data_), pdt_p2p_data_bytes(cap_),
                                        hipDeviceMallocUncached));
    PDT_HIP_CHECK(hipMemset(flags_, 0, flags_bytes_));
    PDT_HIP_CHECK(hipDeviceSynchronize());
    data_ptrs_.assign(world_, nullptr);
    flag_ptrs_.assign(world_, nullptr);
    data_ptrs_[rank_] = data_;
    flag_ptrs_[rank_] = flags_;
  }
  ~P2PComm() {
    for (int r = 0; r < world_; ++r)
      if (r != rank_) {
        if (data_ptrs_[r]) (void)hipIpcCloseMemHandle(data_ptrs_[r]);
        if (flag_ptrs_[r]) (void)hipIpcCloseMemHandle(flag_ptrs_[r]);
      }
    (void)hipFree(flags_);
    (void)hipFree(data_);
  }
  // 2 x hipIpcMemHandle_t (data, flags) as bytes, to be exchanged through the c10d store
  py::bytes handles() const {
    hipIpcMemHandle_t h[2];
    PDT_HIP_CHECK(hipIpcGetMemHandle(&h[0], data_));
    PDT_HIP_CHECK(hipIpcGetMemHandle(&h[1], flags_));
    return py::bytes(reinterpret_cast<const char*>(h), sizeof(h));
  }
  void open(const std::vector<py::bytes>& all) {
    TORCH_CHECK((int)all.size() == world_, "p2p: need one handle blob per rank");
    DevGuard guard(device_);
    for (int r = 0; r < world_; ++r) {
      if (r == rank_) continue;
      std::string b = all[r];
      TORCH_CHECK(b.size() == 2 * sizeof(hipIpcMemHandle_t), "p2p: bad handle blob");
      hipIpcMemHandle_t h[2];
      std::memcpy(h, b.data(), sizeof(h));
      void* d = nullptr;
      void* f = nullptr;
      PDT_HIP_CHECK(hipIpcOpenMemHandle(&d, h[0], hipIpcMemLazyEnablePeerAccess));
      PDT_HIP_CHECK(hipIpcOpenMemHandle(&f, h[1], hipIpcMemLazyEnablePeerAccess));
      data_ptrs_[r] = static_cast<char*>(d);
      flag_ptrs_[r] = static_cast<uint32_t*>(f);
    }
    opened_ = true;
  }
  // out = post_scale * sum over ranks of `in` (out may alias in); enqueued on the current stream.
  // st: int32 [3] device state owned by the caller, zero-initialised ([0] epoch, [1] finished-block
  // counter, [2] sticky error flag) — advanced by the kernel itself (hipGraph-capture safe).
  // algo 0 = one-shot, 1 = two-shot (reduce-scatter + all-gather).
  void allreduce(Tensor in, Tensor out, double post_scale, Tensor st, int64_t algo, double timeout_s) {
    TORCH_CHECK(opened_ || world_ == 1, "p2p: open() the peer handles first");
    check_cuda(in, "in");
    TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && in.numel() == out.numel() &&
                    in.scalar_type() == out.scalar_type(), "p2p: contiguous in/out of equal size and dtype");
    TORCH_CHECK(in.numel() % 8 == 0, "p2p: numel must be a multiple of 8");
    TORCH_CHECK(in.numel() * in.element_size() <= cap_, "p2p: tensor larger than the staging capacity");
    check_cuda(st, "st");
    TORCH_CHECK(st.scalar_type() == at::kInt && st.numel() >= 3 && st.is_contiguous(), "p2p: st int32 [3]");
    TORCH_CHECK(algo == 0 || algo == 1, "p2p: algo 0 (one-shot) or 1 (two-shot)");
    int rc = pdt_p2p_allreduce(in.data_ptr(), out.data_ptr(), in.numel(), dcode(in), data_ptrs_.data(),
                               flag_ptrs_.data(), rank_, world_, cap_, (float)post_scale,
                               reinterpret_cast<uint32_t*>(st.data_ptr<int>()), (int)algo, max_blocks_, timeout_s,
                               stream());
    TORCH_CHECK(rc == 0, "pdt_p2p_allreduce failed (", rc, ")");
  }
  int64_t capacity() const { return cap_; }

 private:
  int rank_, world_;
  int64_t cap_;
  int max_blocks_, device_;
  int64_t flags_bytes_ = 0;
  char* data_ = nullptr;
  uint32_t* flags_ = nullptr;
  bool opened_ = false;
  std::vector<char*> data_ptrs_;
  std::vector<uint32_t*> flag_ptrs_;
};

// ---- GPT-2 token + position embedding (csrc/kernels/embedding.hip) ----
// out [B, T, D] = wte[idx] + wpe[arange(T)] (bf16). idx int64 [B, T]; values must be < V (checked on
// the host only in debug paths: an out-of-range id is a caller bug, as for nn.Embedding).
// Per-device error word of the embedding kernels (an out-of-range token id sets it; never cleared
// by the kernels). Allocated at the first call (before any graph capture of the model).
Tensor embedding_err(const Tensor& like) {
  static std::map<int, Tensor> bufs;
  const int dev = like.get_device();
  auto it = bufs.find(dev);
  if (it == bufs.end()) it = bufs.emplace(dev, at::zeros({1}, like.options().dtype(at::kInt))).first;
  return it->second;
}

Tensor embedding_fwd(Tensor idx, Tensor wte, Tensor wpe) {
  check_cuda(idx, "idx");
  check_cuda(wte, "wte");
  check_cuda(wpe, "wpe");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 2 && idx.is_contiguous(), "embedding: idx int64 [B, T]");
  TORCH_CHECK(wte.scalar_type() == at::kBFloat16 && wpe.scalar_type() == at::kBFloat16 && wte.is_contiguous() &&
                  wpe.is_contiguous() && wte.dim() == 2 && wpe.dim() == 2 && wte.size(1) == wpe.size(1),
              "embedding: wte [V, D], wpe [P, D] contiguous bf16");
  const int64_t B = idx.size(0), T = idx.size(1), D = wte.size(1);
  TORCH_CHECK(T <= wpe.size(0) && D % 8 == 0, "embedding: T <= P, D % 8 == 0");
  auto out = at::empty({B, T, D}, wte.options());
  TORCH_CHECK(pdt_embedding_fwd(idx.data_ptr<int64_t>(), bf16_ptr(wte), bf16_ptr(wpe), bf16_out(out), B * T, (int)T,
                                (int)D, (int)wte.size(0), embedding_err(idx).data_ptr<int>(), stream()) == 0,
              "pdt_embedding_fwd failed");
  return out;
}

// (dwte [V, D], dwpe [P, D]) from dout [B, T, D]: deterministic (counting sort + ordered row sums).
std::vector<Tensor> embedding_bwd(Tensor idx, Tensor dout, int64_t V, int64_t P) {
  check_cuda(idx, "idx");
  check_cuda(dout, "dout");
  dout = dout.contiguous();
  TORCH_CHECK(dout.scalar_type() == at::kBFloat16 && dout.dim() == 3 && dout.size(0) == idx.size(0) &&
                  dout.size(1) == idx.size(1), "embedding_bwd: dout [B, T, D] bf16");
  const int64_t B = idx.size(0), T = idx.size(1), D = dout.size(2), n = B * T;
  auto ws = at::zeros({pdt_embedding_bwd_ws_ints(n, (int)V)}, idx.options().dtype(at::kInt));
  auto dwte = at::empty({V, D}, dout.options());
  auto dwpe = T == P ? at::empty({P, D}, dout.options()) : at::zeros({P, D}, dout.options());
  TORCH_CHECK(pdt_embedding_bwd(idx.data_ptr<int64_t>(), bf16_ptr(dout), bf16_out(dwte), bf16_out(dwpe),
                                ws.data_ptr<int>(), n, (int)B, (int)T, (int)V, (int)D,
                                embedding_err(idx).data_ptr<int>(), stream()) == 0,
              "pdt_embedding_bwd failed");
  return {dwte, dwpe};
}

// ---- Linear GEMM with fused epilogues (csrc/kernels/gemm.hip) ----
// a [M, K], b [N, K] contiguous bf16 -> {C [M, N]} (epi 0: a·bᵀ, 1: a·bᵀ + bias) or {C, G} (epi 2:
// C = a·bᵀ, G = gelu(C + bias)). bias [N] fp32 or bf16. N % 128 == 0, K % 64 == 0 (gemm_nt_ok).
std::vector<Tensor> gemm_nt(Tensor a, Tensor b, c10::optional<Tensor> bias, int64_t epi, bool tanh_form) {
  check_cuda(a, "a");
  check_cuda(b, "b");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16 && a.dim() == 2 && b.dim() == 2 &&
                  a.is_contiguous() && b.is_contiguous() && a.size(1) == b.size(1),
              "gemm_nt: a [M, K], b [N, K] contiguous bf16");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  const void* bp = nullptr;
  int bf32 = 0;
  if (has(bias)) {
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N &&
                    (bias->scalar_type() == at::kFloat || bias->scalar_type() == at::kBFloat16),
                "gemm_nt: bias [N] fp32 or bf16");
    bp = bias->data_ptr();
    bf32 = bias->scalar_type() == at::kFloat;
  }
  auto c = at::empty({M, N}, a.options());
  Tensor g = epi == 2 ? at::empty({M, N}, a.options()) : Tensor();
  const int rc = pdt_gemm_nt(bf16_ptr(a), bf16_ptr(b), bf16_out(c), ptr_or_null<uint16_t>(g), bp, bf32, (int)epi,
                             tanh_form ? 1 : 0, (int)M, (int)N, (int)K, stream());
  TORCH_CHECK(rc == 0, "pdt_gemm_nt failed (", rc, ") for M=", M, " N=", N, " K=", K);
  if (epi == 2) return {c, g};
  return {c};
}

// fp8 e4m3 operands (csrc/kernels/gemm.hip F8): C [M, N] bf16 = (a sa)(b sb)^T (+ bias) from a [M, K], b [N, K]
// contiguous float8_e4m3fn and one-element fp32 dequantisation scales (torch._scaled_mm's scale_a / scale_b).
// N % 128 == 0, K % 128 == 0 (gemm_nt_fp8_ok).
Tensor gemm_nt_fp8(Tensor a, Tensor b, Tensor sa, Tensor sb, c10::optional<Tensor> bias) {
  check_cuda(a, "a");
  check_cuda(b, "b");
  TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn && b.scalar_type() == at::kFloat8_e4m3fn && a.dim() == 2 &&
                  b.dim() == 2 && a.is_contiguous() && b.is_contiguous() && a.size(1) == b.size(1),
              "gemm_nt_fp8: a [M, K], b [N, K] contiguous float8_e4m3fn");
  TORCH_CHECK(sa.scalar_type() == at::kFloat && sb.scalar_type() == at::kFloat && sa.numel() == 1 && sb.numel() == 1 &&
                  sa.is_cuda() && sb.is_cuda(), "gemm_nt_fp8: one-element fp32 device scales");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  const void* bp = nullptr;
  int bf32 = 0;
  if (has(bias)) {
    TORCH_CHECK(bias->is_contiguous() && bias->numel() == N &&
                    (bias->scalar_type() == at::kFloat || bias->scalar_type() == at::kBFloat16),
                "gemm_nt_fp8: bias [N] fp32 or bf16");
    bp = bias->data_ptr();
    bf32 = bias->scalar_type() == at::kFloat;
  }
  auto c = at::empty({M, N}, a.options().dtype(at::kBFloat16));
  // few output tiles and no bias (the weight gradients): split K, fp32 partials + one reduce pass
  const int ks = bp ? 1 : pdt_gemm_nt_fp8_ksplit((int)M, (int)N, (int)K);
  Tensor ws;
  if (ks > 1) ws = at::empty({(int64_t)ks * M * N}, a.options().dtype(at::kFloat));
  const int rc = pdt_gemm_nt_fp8(byte_ptr(a), byte_ptr(b), bf16_out(c), sa.data_ptr<float>(), sb.data_ptr<float>(), bp,
                                 bf32, bp ? 1 : 0, (int)M, (int)N, (int)K, ptr_or_null<float>(ws), ks, stream());
  TORCH_CHECK(rc == 0, "pdt_gemm_nt_fp8 failed (", rc, ") for M=", M, " N=", N, " K=", K);
  return c;
}

// Read-only queries (no launch): the tile width (128 / 256; 0 = shape not served) gemm_nt and gemm_nt_fp8 run
// [M, N] with, and the number of K splits gemm_nt_fp8 takes without a bias.
int64_t gemm_nt_tile_n(int64_t M, int64_t N) { return pdt_gemm_nt_tile_n((int)M, (int)N); }
int64_t gemm_nt_fp8_ksplit(int64_t M, int64_t N, int64_t K) { return pdt_gemm_nt_fp8_ksplit((int)M, (int)N, (int)K); }

// ---- LeNet (reference model) ops: csrc/kernels/lenet.hip ----
constexpr int kStemIpb = 4;  // images per workgroup in the conv1 weight-gradient reduction

std::vector<Tensor> lenet_stem_fwd(Tensor x, Tensor w, Tensor b, double slope) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 4 && x.size(1) == 1 &&
                  x.size(2) == 28 && x.size(3) == 28, "lenet_stem: x must be contiguous fp32 [N,1,28,28]");
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous() && w.numel() == 150 && b.numel() == 6 &&
                  b.is_contiguous(), "lenet_stem: conv1 weight [6,1,5,5] / bias [6] fp32");
  const int64_t N = x.size(0);
  auto y = at::empty({N, 6, 14, 14}, x.options());
  auto code = at::empty({N, 6, 14, 14}, x.options().dtype(at::kByte));
  pdt_lenet_stem_fwd(x.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(), N, (float)slope,
                     y.data_ptr<float>(), code.data_ptr<uint8_t>(), stream());
  return {y, code};
}

std::vector<Tensor> lenet_stem_bwd(Tensor dy, Tensor code, Tensor x, double slope) {
  const int64_t N = x.size(0);
  dy = dy.contiguous();
  TORCH_CHECK(dy.scalar_type() == at::kFloat && dy.numel() == N * 1176 && code.numel() == N * 1176 &&
                  x.numel() == N * 784, "lenet_stem_bwd: shape mismatch");
  auto slab = at::empty({std::max<int64_t>(pdt_lenet_stem_slab_floats(N, kStemIpb), 1)}, x.options());
  auto dw = at::empty({6, 1, 5, 5}, x.options());
  auto db = at::empty({6}, x.options());
  pdt_lenet_stem_bwd(dy.data_ptr<float>(), code.data_ptr<uint8_t>(), x.data_ptr<float>(), N, kStemIpb,
                     (float)slope, slab.data_ptr<float>(), dw.data_ptr<float>(), db.data_ptr<float>(), stream());
  return {dw, db};
}

std::vector<Tensor> leaky_pool_fwd(Tensor x, double slope) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous() && x.dim() == 4, "leaky_pool: contiguous fp32 NCHW");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  auto y = at::empty({N, C, H / 2, W / 2}, x.options());
  auto code = at::empty({N, C, H / 2, W / 2}, x.options().dtype(at::kByte));
  pdt_leaky_pool_fwd(x.data_ptr<float>(), N * C, (int)H, (int)W, (float)slope, y.data_ptr<float>(),
                     code.data_ptr<uint8_t>(), stream());
  return {y, code};
}

Tensor leaky_pool_bwd(Tensor dy, Tensor code, int64_t H, int64_t W, double slope) {
  dy = dy.contiguous();
  const int64_t N = dy.size(0), C = dy.size(1);
  TORCH_CHECK(dy.scalar_type() == at::kFloat && dy.size(2) == H / 2 && dy.size(3) == W / 2 &&
                  code.numel() == dy.numel(), "leaky_pool_bwd: shape mismatch");
  auto dx = at::empty({N, C, H, W}, dy.options());
  pdt_leaky_pool_bwd(dy.data_ptr<float>(), code.data_ptr<uint8_t>(), N * C, (int)H, (int)W, (float)slope,
                     dx.data_ptr<float>(), stream());
  return dx;
}

// returns {loss[N] (if want_loss), dlogits (if want_grad)}; acc (fp64 [3]) accumulates eval metrics
// mean_scale > 0 (with want_loss): also {.., mean_scale * sum(loss)} as a 0-d fp32 tensor (fixed-order
// one-workgroup sum; the training loss without a torch reduction per step).
std::vector<Tensor> softmax_nll_small(Tensor logits, Tensor target, int64_t mode, double smoothing, bool want_loss,
                                      bool want_grad, double dscale, c10::optional<Tensor> acc,
                                      double mean_scale) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "softmax_nll_small: contiguous [N, V] logits");
  TORCH_CHECK(logits.size(1) <= 1024, "softmax_nll_small: V <= 1024");
  TORCH_CHECK(target.scalar_type() == at::kLong && target.is_contiguous(), "softmax_nll_small: int64 target");
  const int64_t N = logits.size(0);
  Tensor loss, dl;
  if (want_loss) loss = at::empty({N}, logits.options().dtype(at::kFloat));
  if (want_grad) dl = at::empty_like(logits);
  double* ap = nullptr;
  if (has(acc)) {
    TORCH_CHECK(acc->scalar_type() == at::kDouble && acc->numel() >= 3, "softmax_nll_small: acc fp64 [3]");
    ap = acc->data_ptr<double>();
  }
  int rc = pdt_softmax_nll_small(logits.data_ptr(), dcode(logits), target.data_ptr<int64_t>(), N,
                                 (int)logits.size(1), (int)mode, (float)smoothing,
                                 ptr_or_null<float>(loss), want_grad ? dl.data_ptr() : nullptr,
                                 (float)dscale, ap, stream());
  TORCH_CHECK(rc == 0, "pdt_softmax_nll_small failed");
  if (mean_scale > 0.0 && want_loss) {
    auto mean = at::empty({}, logits.options().dtype(at::kFloat));
    pdt_mean_small(loss.data_ptr<float>(), N, (float)mean_scale, mean.data_ptr<float>(), stream());
    return {loss, dl, mean};
  }
  return {loss, dl};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 HIP kernels for pytorch_distributed_training_example_amd";
  m.def("sgd", &sgd);
  m.def("adam", &adam);
  m.def("adadelta", &adadelta);
  m.def("lars", &lars);
  m.def("lamb", &lamb);
  m.def("layerwise_chunks", &layerwise_chunks);
  m.def("amp_unscale", &amp_unscale);
  m.def("amp_update", &amp_update);
  m.def("mt_scale", &mt_scale);
  m.def("mt_copy", &mt_copy);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("clip_coef", &clip_coef);
  m.def("bn_tune", [](int variant, int target_blocks, int u_fwd, int u_bwd) {
    if (pdt_bn_tune(variant, target_blocks, u_fwd, u_bwd) != 0)
      throw py::value_error("bn_tune: variant must be 0 (keep), 3 (in-kernel finalize) or 5 (finalize kernel), got " +
                            std::to_string(variant));
  }, py::arg("variant") = 0, py::arg("target_blocks") = 0, py::arg("u_fwd") = 0, py::arg("u_bwd") = 0);
  m.def("bn_fwd_train", &bn_fwd_train, py::arg("x"), py::arg("res"), py::arg("weight"), py::arg("bias"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"), py::arg("relu"),
        py::arg("res_ab") = py::none(), py::arg("apply") = true);
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("bn_relu_maxpool_fwd", &bn_relu_maxpool_fwd);
  m.def("bn_relu_maxpool_fwd_parts", &bn_relu_maxpool_fwd_parts);
  m.def("maxpool3s2_bwd", &maxpool3s2_bwd);
  m.def("conv1x1_gemm", &conv1x1_gemm, py::arg("a"), py::arg("b"), py::arg("out"), py::arg("acc"), py::arg("stats"),
        py::arg("c_in") = py::none(), py::arg("c_mask") = py::none(), py::arg("bn_x") = py::none(),
        py::arg("bn_mask") = py::none(), py::arg("bn_mean") = py::none(), py::arg("c_stride") = 0,
        py::arg("c_H") = 0, py::arg("c_W") = 0, py::arg("a_coef") = py::none(), py::arg("bn_sum_only") = false,
        py::arg("no_store") = false);
  m.def("conv1x1_probe", [](int probe) { pdt_conv1x1_probe(probe); });
  m.def("conv1x1_persist", [](int mode) { return pdt_conv1x1_persist(mode); },
        "1x1 GEMM persistence mode (0 off, 1 measured kinds, 2 all, -1 env default); returns the previous mode");
  m.def("conv1x1_last_persistent", []() { return pdt_conv1x1_last_persistent(); },
        "which kernel the last 1x1 GEMM call launched: 0 one tile per workgroup, else the persistent kernel's waves "
        "per workgroup (+256 statistics-only, +512 APPLY)");
  m.def("conv3x3_opt", [](int v) { return pdt_conv3x3_opt(v); },
        "3x3 conv variant bits (csrc/kernels/conv3x3.hip conv3x3_opt; -1 env default); returns the previous value");
  m.def("weight_prep", &weight_prep);
  m.def("bn_tiles_fused", [](int on) { pdt_bn_tiles_fused(on); });
  m.def("maxpool_bwd_v2", [](int on) { pdt_maxpool_bwd_v2(on); });
  m.def("pool_fwd_contig", [](int on) { pdt_pool_fwd_contig(on); });
  m.def("bn_apply_wgs", [](int n) { pdt_bn_apply_wgs(n); });
  m.def("bn_row_wgs", [](int n) { pdt_bn_row_wgs(n); });
  m.def("gap_bwd", &gap_bwd, py::arg("g"), py::arg("H"), py::arg("W"), py::arg("bn_x") = py::none(),
        py::arg("bn_mask") = py::none(), py::arg("bn_mean") = py::none(), py::arg("bn_sum_only") = false);
  m.def("conv1x1_gemm_apply", &conv1x1_gemm_apply, py::arg("a"), py::arg("b"), py::arg("res"), py::arg("ab"),
        py::arg("rab") = py::none(), py::arg("a_coef") = py::none());
  m.def("bn_bwd_train_tiles", &bn_bwd_train_tiles);
  m.def("maxpool3s2_bwd_bn", &maxpool3s2_bwd_bn);
  m.def("maxpool3s2_bwd_bn_coef", &maxpool3s2_bwd_bn_coef, py::arg("dy"), py::arg("code"), py::arg("x"),
        py::arg("weight"), py::arg("mean"), py::arg("invstd"), py::arg("need_dgamma"), py::arg("write_dz") = true);
  m.def("slice_sum", &slice_sum);
  m.def("subsample_gather", &subsample_gather);
  m.def("subsample_scatter_add", &subsample_scatter_add);
  m.def("bn_fwd_train_tiles", &bn_fwd_train_tiles, py::arg("x"), py::arg("part"), py::arg("res"), py::arg("weight"),
        py::arg("bias"), py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("relu"), py::arg("res_ab") = py::none(), py::arg("apply") = true, py::arg("sub") = 0);
  m.def("conv3x3s1_variant", &conv3x3s1_variant);
  m.def("conv3x3_wgrad_geo", &conv3x3_wgrad_geo);
  m.def("conv3x3s1_fwd", &conv3x3s1_fwd);
  m.def("conv3x3s1_fwd_stats", &conv3x3s1_fwd_stats);
  m.def("conv3x3s1_fwd_bnbwd", &conv3x3s1_fwd_bnbwd);
  m.def("conv3x3_flip", &conv3x3_flip);
  m.def("conv3x3s2_fwd", &conv3x3s2_fwd);
  m.def("conv3x3s2_wgrad", &conv3x3s2_wgrad);
  m.def("conv3x3s2_dgrad", &conv3x3s2_dgrad, py::arg("dy"), py::arg("wf"), py::arg("H"), py::arg("W"),
        py::arg("bn_x") = py::none(), py::arg("bn_mask") = py::none(), py::arg("bn_mean") = py::none());
  m.def("stem_conv_fwd", &stem_conv_fwd);
  m.def("stem_conv_fwd_stats", &stem_conv_fwd_stats);
  m.def("stem_conv_wgrad", &stem_conv_wgrad);
  m.def("stem_conv_wgrad_bn", &stem_conv_wgrad_bn);
  m.def("stem_conv_wgrad_bn_pool", &stem_conv_wgrad_bn_pool);
  m.def("conv3x3s1_wgrad", &conv3x3s1_wgrad);
  m.def("conv1x1_wgrad", &conv1x1_wgrad);
  m.def("conv1x1_wgrad_seg", &conv1x1_wgrad_seg);
  m.def("conv1x1_gemm_seg", &conv1x1_gemm_seg, py::arg("a1"), py::arg("a2"), py::arg("rep2"), py::arg("b"),
        py::arg("out"), py::arg("bn_x") = py::none(), py::arg("bn_mask") = py::none(), py::arg("bn_mean") = py::none());
  m.def("bn_alg_assemble", &bn_alg_assemble, py::arg("w"), py::arg("coef"), py::arg("mean"), py::arg("G"), py::arg("wg"),
        py::arg("BWG"), py::arg("rep") = 2);
  m.def("bn_alg_fix_s2", &bn_alg_fix_s2);
  m.def("bn_alg_ds_part", &bn_alg_ds_part);
  m.def("bn_alg_small_gemm", &bn_alg_small_gemm, py::arg("w"), py::arg("coef"), py::arg("wg"), py::arg("wt") = py::none());
  m.def("conv1x1_wgrad_tune", [](int target_wgs, int variant, int interleave) { pdt_conv1x1_wgrad_tune(target_wgs, variant, interleave); },
        py::arg("target_wgs"), py::arg("variant") = -2, py::arg("interleave") = -2);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("gemm_nt", &gemm_nt);
  m.def("gemm_nt_fp8", &gemm_nt_fp8, py::arg("a"), py::arg("b"), py::arg("sa"), py::arg("sb"), py::arg("bias") = py::none());
  m.def("gemm_nt_tile_n", &gemm_nt_tile_n);
  m.def("gemm_nt_fp8_ksplit", &gemm_nt_fp8_ksplit);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("embedding_err", &embedding_err);
  m.def("conv3x3_wgrad_tune", [](int target_wgs, int co_tile) { pdt_conv3x3_wgrad_tune(target_wgs, co_tile); });
  m.def("bn_bwd_train", &bn_bwd_train);
  m.def("bn_bwd_coef", &bn_bwd_coef);
  m.def("bn_sync_fwd_stats", &bn_sync_fwd_stats, py::arg("x"), py::arg("row") = py::none());
  m.def("bn_sync_fwd_merge", &bn_sync_fwd_merge);
  m.def("bn_apply_coef", &bn_apply_coef);
  m.def("bn_sync_bwd_sums", &bn_sync_bwd_sums, py::arg("dy"), py::arg("x"), py::arg("mask"), py::arg("mean"),
        py::arg("relu"), py::arg("row") = py::none());
  m.def("bn_sync_bwd_merge", &bn_sync_bwd_merge);
  m.def("bn_bwd_apply_coef", &bn_bwd_apply_coef);
  m.def("conv1x1_bwd_fused", &conv1x1_bwd_fused, py::arg("dy"), py::arg("z"), py::arg("mz"), py::arg("mean"),
        py::arg("coef"), py::arg("w"), py::arg("xa"), py::arg("bn_x") = py::none(), py::arg("bn_mask") = py::none(),
        py::arg("bn_mean") = py::none(), py::arg("xcoef") = py::none(), py::arg("wt") = py::none());
  m.def("conv1x1_bwd_fused_tune", [](int grid) { pdt_conv1x1_bwd_fused_tune(grid); });
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ln_fwd", &ln_fwd, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("eps"), py::arg("res") = py::none());
  m.def("ln_fwd_fp8", &ln_fwd_fp8, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("eps"), py::arg("res"),
        py::arg("state_row"));
  m.def("ln_bwd", &ln_bwd, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("mean"), py::arg("rstd"),
        py::arg("dres") = py::none());
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("attn_fwd_out", &attn_fwd_out);
  m.def("attn_bwd_out", &attn_bwd_out);
  m.def("attn_fwd_drop_out", &attn_fwd_drop_out);
  m.def("attn_bwd_drop_out", &attn_bwd_drop_out);
  m.def("attn_fwd_gqa_out", &attn_fwd_gqa_out);
  m.def("attn_bwd_gqa_out", &attn_bwd_gqa_out);
  m.def("dropout_begin", &dropout_begin);
  m.def("dropout_fwd", &dropout_fwd);
  m.def("dropout_mask", &dropout_mask);
  m.def("ln_fwd_drop", &ln_fwd_drop);
  m.def("ln_bwd_drop", &ln_bwd_drop);
  m.def("colsum", &colsum);
  m.def("rms_fwd", &rms_fwd, py::arg("x"), py::arg("w"), py::arg("eps"), py::arg("res") = py::none(),
        py::arg("y_out") = py::none(), py::arg("rstd_out") = py::none(), py::arg("sum_out") = py::none());
  m.def("rms_bwd", &rms_bwd, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("rstd"),
        py::arg("dres") = py::none(), py::arg("dx_out") = py::none(), py::arg("dw_out") = py::none());
  m.def("rms_fwd_fp8", &rms_fwd_fp8, py::arg("x"), py::arg("w"), py::arg("eps"), py::arg("res"), py::arg("state_row"));
  m.def("rope_qkv", &rope_qkv, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("heads"),
        py::arg("conj") = false);
  m.def("rope_qkv_gqa", &rope_qkv_gqa, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("heads"),
        py::arg("kv_heads"), py::arg("conj") = false);
  m.def("rope_kv_append", &rope_kv_append, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("heads"),
        py::arg("kv_heads"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"));
  m.def("attn_decode_geo", &attn_decode_geo, py::arg("B"), py::arg("kv_heads"), py::arg("capacity"),
        py::arg("splits") = 0, py::arg("group") = 1);
  m.def("attn_decode", &attn_decode, py::arg("qkv"), py::arg("k_cache"), py::arg("v_cache"), py::arg("lens"),
        py::arg("heads"), py::arg("kv_heads"), py::arg("scale"), py::arg("splits"), py::arg("out"),
        py::arg("o_part") = py::none(), py::arg("ml_part") = py::none(), py::arg("lse") = py::none());
  m.def("swiglu_fwd", &swiglu_fwd, py::arg("gu"), py::arg("y_out") = py::none());
  m.def("swiglu_bwd", &swiglu_bwd, py::arg("dy"), py::arg("gu"), py::arg("dgu_out") = py::none());
  py::class_<P2PComm>(m, "P2PComm")
      .def(py::init<int, int, int64_t, int, int>(), py::arg("rank"), py::arg("world"), py::arg("capacity_bytes"),
           py::arg("max_blocks"), py::arg("device"))
      .def("handles", &P2PComm::handles)
      .def("open", &P2PComm::open)
      .def("allreduce", &P2PComm::allreduce)
      .def("capacity", &P2PComm::capacity);
  m.def("fp8_cast_transpose", &fp8_cast_transpose);
  m.def("fp8_update_scales", &fp8_update_scales);
  m.def("fp8_gelu_cast", &fp8_gelu_cast, py::arg("h"), py::arg("dg") = py::none(), py::arg("bias") = py::none(),
        py::arg("state_row"), py::arg("tanh_form") = false, py::arg("db_dtype") = at::kFloat);
  m.def("fp8_swiglu_cast", &fp8_swiglu_cast, py::arg("gu"), py::arg("dy") = py::none(), py::arg("state_row"));
  m.def("fp8_cast_multi", &fp8_cast_multi);
  m.def("fp8_cast_colsum", &fp8_cast_colsum);
  m.def("lenet_stem_fwd", &lenet_stem_fwd);
  m.def("lenet_stem_bwd", &lenet_stem_bwd);
  m.def("leaky_pool_fwd", &leaky_pool_fwd);
  m.def("leaky_pool_bwd", &leaky_pool_bwd);
  m.def("lenet_tail_fwd", &lenet_tail_fwd);
  m.def("lenet_tail_bwd", &lenet_tail_bwd);
  m.def("softmax_nll_small", &softmax_nll_small, py::arg("logits"), py::arg("target"), py::arg("mode"),
        py::arg("smoothing"), py::arg("want_loss"), py::arg("want_grad"), py::arg("dscale"), py::arg("acc"),
        py::arg("mean_scale") = 0.0);
}
