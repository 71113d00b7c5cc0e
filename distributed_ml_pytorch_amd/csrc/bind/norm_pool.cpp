// bn.hip, pool.hip, head.hip: BatchNorm, pooling, the GAP + Linear head and the
// ReLU backward (im2col.hip).
#include "util.h"

namespace dmp::bind {
namespace {

// ---------------------------------------------------------------- batchnorm
// x is a channels-last activation (N,C,H,W logical) or a [M, C] matrix.
int64_t channels_of(const Tensor& x) { return x.size(1); }

using OptTensors = std::initializer_list<const optional<Tensor>*>;

void check_bn_stats(const Tensor& stats, int64_t C) {
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.numel() == 4 * C,
              "bn: stats must be fp32 [4, C]");
}

// Shared front-end of the forwards: checks x, res and the given affine /
// running tensors, allocates the outputs.
struct BnFwd {
  int64_t C, M;
  at::TensorOptions fopt;
  Tensor y, stats, mask;
  std::vector<Tensor> result() const { return {y, stats, mask}; }
};

BnFwd bn_fwd_front(const Tensor& x, const optional<Tensor>& res, OptTensors affine, bool relu,
                   bool want_mask) {
  check_nhwc_bf16(x, "x");
  BnFwd f;
  f.C = channels_of(x);
  f.M = x.numel() / f.C;
  TORCH_CHECK(f.C % 8 == 0 && f.C <= 2048, "bn: C must be a multiple of 8 and <= 2048, got ", f.C);
  if (has(res)) {
    check_nhwc_bf16(*res, "res");
    same_shape(*res, x, "res");
  }
  check_vecs(affine, at::kFloat, f.C, "bn affine / running tensors");
  f.fopt = x.options().dtype(at::kFloat);
  f.y = at::empty_like(x);
  f.stats = at::empty({4, f.C}, f.fopt);
  // 1-bit ReLU mask [M][C/8] for the backward (instead of re-reading y)
  if (want_mask && relu) f.mask = at::empty({f.M, f.C / 8}, x.options().dtype(at::kByte));
  return f;
}

std::vector<Tensor> bn_fwd(Tensor x, optional<Tensor> res, optional<Tensor> gamma,
                           optional<Tensor> beta, optional<Tensor> running_mean,
                           optional<Tensor> running_var, double momentum, double eps,
                           bool training, bool relu, optional<Tensor> slots, bool want_mask) {
  TORCH_CHECK(training || (has(running_mean) && has(running_var)),
              "eval-mode bn needs running stats");
  auto f = bn_fwd_front(x, res, {&gamma, &beta, &running_mean, &running_var}, relu, want_mask);
  auto part = bn_slots(slots, f.C, f.fopt);
  dmp::launch_bn_fwd(bf16(x), bf16_or_null(res), bf16(f.y), ptr_or_null<float>(gamma),
                     ptr_or_null<float>(beta), ptr_or_null<float>(running_mean),
                     ptr_or_null<float>(running_var), f.stats.data_ptr<float>(),
                     part.data_ptr<float>(), f.M, (int)f.C, (float)momentum, (float)eps, training,
                     relu, cur_stream(), ptr_or_null<uint8_t>(f.mask));
  return f.result();
}

// part: the conv-epilogue slot sums.  Unlike its siblings this entry point has
// never checked the affine and running tensors; it still does not.
std::vector<Tensor> bn_fwd_from_partials(Tensor x, Tensor part, int64_t G, optional<Tensor> res,
                                         optional<Tensor> gamma, optional<Tensor> beta,
                                         optional<Tensor> running_mean,
                                         optional<Tensor> running_var, double momentum,
                                         double eps, bool relu, bool want_mask) {
  TORCH_CHECK(G == dmp::kBnSlots, "bn: partials must have ", dmp::kBnSlots, " slot rows");
  auto f = bn_fwd_front(x, res, {}, relu, want_mask);
  part = bn_slots(part, f.C, f.fopt);
  dmp::launch_bn_fwd_partials(bf16(x), bf16_or_null(res), bf16(f.y), ptr_or_null<float>(gamma),
                              ptr_or_null<float>(beta), ptr_or_null<float>(running_mean),
                              ptr_or_null<float>(running_var), f.stats.data_ptr<float>(),
                              part.data_ptr<float>(), f.M, (int)f.C, (float)momentum, (float)eps,
                              relu, cur_stream(), ptr_or_null<uint8_t>(f.mask));
  return f.result();
}

// BatchNorm with the finalize folded into the apply passes (bn.hip fold kernels).
// part: the forward slot sums (already filled by the producing conv when
// have_partials, else reduced here first); zero_buf: the layer's backward slots,
// zeroed by the apply for the next backward.
std::vector<Tensor> bn_fwd_fold(Tensor x, Tensor part, bool have_partials, optional<Tensor> res,
                                optional<Tensor> gamma, optional<Tensor> beta,
                                optional<Tensor> running_mean, optional<Tensor> running_var,
                                double momentum, double eps, bool relu, bool want_mask,
                                optional<Tensor> zero_buf) {
  auto f = bn_fwd_front(x, res, {&gamma, &beta, &running_mean, &running_var}, relu, want_mask);
  part = bn_slots(part, f.C, f.fopt);
  float* zb = other_slots(zero_buf, f.C, f.fopt, part);
  dmp::launch_bn_fwd_fold(bf16(x), bf16_or_null(res), bf16(f.y), ptr_or_null<float>(gamma),
                          ptr_or_null<float>(beta), ptr_or_null<float>(running_mean),
                          ptr_or_null<float>(running_var), f.stats.data_ptr<float>(),
                          part.data_ptr<float>(), zb, f.M, (int)f.C, (float)momentum, (float)eps,
                          relu, have_partials, cur_stream(), ptr_or_null<uint8_t>(f.mask));
  return f.result();
}

// Shared front-end of the backwards: checks x, dy (made channels_last), y,
// stats, the affine gradients and the ReLU mask, allocates dx / dres.
struct BnBwd {
  int64_t C, M;
  at::TensorOptions fopt;
  const uint16_t* y;     // null: the ReLU mask is `mask`, or recomputed from x and stats
  const uint8_t* mask;
  Tensor dx, dres;
  std::vector<Tensor> result() const { return {dx, dres}; }
};

BnBwd bn_bwd_front(const Tensor& x, Tensor& dy, const optional<Tensor>& y,
                   const optional<Tensor>& gamma, const Tensor& stats,
                   const optional<Tensor>& dgamma, const optional<Tensor>& dbeta, bool relu,
                   bool want_dres, const optional<Tensor>& mask) {
  check_nhwc_bf16(x, "x");
  BnBwd b;
  b.C = channels_of(x);
  b.M = x.numel() / b.C;
  TORCH_CHECK(b.C % 8 == 0 && b.C <= 2048, "bn: C must be a multiple of 8 and <= 2048, got ", b.C);
  if (!dy.is_contiguous(kCL) && x.dim() == 4) dy = dy.contiguous(kCL);
  check_nhwc_bf16(dy, "dy");
  same_shape(dy, x, "dy");
  b.y = nullptr;
  if (relu && has(y)) {
    check_nhwc_bf16(*y, "y");
    same_shape(*y, x, "y");
    b.y = bf16(*y);
  }
  check_bn_stats(stats, b.C);
  check_vecs({&gamma, &dgamma, &dbeta}, at::kFloat, b.C, "bn gamma / dgamma / dbeta");
  b.mask = relu_mask_ptr(mask, relu, b.M, b.C);
  b.fopt = x.options().dtype(at::kFloat);
  b.dx = at::empty_like(x);
  if (want_dres) b.dres = at::empty_like(x);
  return b;
}

std::vector<Tensor> bn_bwd(Tensor x, Tensor dy, optional<Tensor> y, optional<Tensor> gamma,
                           Tensor stats, optional<Tensor> dgamma, optional<Tensor> dbeta,
                           bool relu, bool want_dres, optional<Tensor> slots,
                           optional<Tensor> mask, bool batch_stats) {
  auto b = bn_bwd_front(x, dy, y, gamma, stats, dgamma, dbeta, relu, want_dres, mask);
  auto part = bn_slots(slots, b.C, b.fopt);
  auto coef = at::empty({3, b.C}, b.fopt);
  dmp::launch_bn_bwd(bf16(x), bf16(dy), b.y, ptr_or_null<float>(gamma), stats.data_ptr<float>(),
                     ptr_or_null<float>(dgamma), ptr_or_null<float>(dbeta), coef.data_ptr<float>(),
                     part.data_ptr<float>(), bf16(b.dx), bf16_or_null(b.dres), b.M, (int)b.C, relu,
                     cur_stream(), b.mask, batch_stats);
  return b.result();
}

// backward: reduce into `slots` (the layer's backward slots, zero on entry), then
// the folded apply; zero_buf: the forward slot sums this layer's forward read
std::vector<Tensor> bn_bwd_fold(Tensor x, Tensor dy, optional<Tensor> y, optional<Tensor> gamma,
                                Tensor stats, optional<Tensor> dgamma, optional<Tensor> dbeta,
                                bool relu, bool want_dres, Tensor slots, optional<Tensor> mask,
                                optional<Tensor> zero_buf) {
  auto b = bn_bwd_front(x, dy, y, gamma, stats, dgamma, dbeta, relu, want_dres, mask);
  auto part = bn_slots(slots, b.C, b.fopt);
  float* zb = other_slots(zero_buf, b.C, b.fopt, part);
  dmp::launch_bn_bwd_fold(bf16(x), bf16(dy), b.y, ptr_or_null<float>(gamma),
                          stats.data_ptr<float>(), ptr_or_null<float>(dgamma),
                          ptr_or_null<float>(dbeta), part.data_ptr<float>(), zb, bf16(b.dx),
                          bf16_or_null(b.dres), b.M, (int)b.C, relu, cur_stream(), b.mask);
  return b.result();
}

// BN + ReLU + max pool 3x3/s2/p1 with the finalize folded in (bn.hip): x is the
// raw conv output; returns the pooled output, its uint8 argmax taps and stats.
std::vector<Tensor> bn_relu_maxpool_fwd(Tensor x, Tensor part, bool have_partials,
                                        optional<Tensor> gamma, optional<Tensor> beta,
                                        optional<Tensor> running_mean,
                                        optional<Tensor> running_var, double momentum, double eps,
                                        optional<Tensor> zero_buf, int64_t K, int64_t S,
                                        int64_t P) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "bn_relu_maxpool expects 4-D input");
  TORCH_CHECK(dmp::guard::bf16_bytes_ok(x.size(0), x.size(2), x.size(3), x.size(1)),
              "bn_relu_maxpool: x over 2 GiB (32-bit offsets)");
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(dmp::bn_maxpool_supported(C, (int)K, (int)S, (int)P),
              "bn_relu_maxpool: needs C % 64 == 0, C <= 2048 and a 3x3/s2/p1 window");
  auto fopt = x.options().dtype(at::kFloat);
  part = bn_slots(part, C, fopt);
  float* zb = other_slots(zero_buf, C, fopt, part);
  check_vecs({&gamma, &beta, &running_mean, &running_var}, at::kFloat, C,
             "bn affine / running tensors");
  const int Ho = dmp::maxpool_out(H, (int)K, (int)S, (int)P);
  const int Wo = dmp::maxpool_out(W, (int)K, (int)S, (int)P);
  TORCH_CHECK(Ho > 0 && Wo > 0, "bn_relu_maxpool: window larger than input");
  auto y = at::empty({N, C, Ho, Wo}, x.options().memory_format(kCL));
  auto idx = at::empty({N, C, Ho, Wo}, x.options().dtype(at::kByte).memory_format(kCL));
  auto xm = at::empty({N, C, Ho, Wo}, x.options().memory_format(kCL));
  auto stats = at::empty({4, C}, fopt);
  dmp::launch_bn_relu_maxpool_fold(
      bf16(x), bf16(y), idx.data_ptr<uint8_t>(), bf16(xm), ptr_or_null<float>(gamma),
      ptr_or_null<float>(beta), ptr_or_null<float>(running_mean), ptr_or_null<float>(running_var),
      stats.data_ptr<float>(), part.data_ptr<float>(), zb, N, H, W, C, (float)momentum, (float)eps,
      have_partials, cur_stream());
  return {y, idx, stats, xm};
}

// backward of bn_relu_maxpool_fwd: dx of the raw conv output from the pooled
// gradient; slots = the layer's backward slots (zero on entry), zero_buf = the
// forward slot sums the forward read
Tensor maxpool_bn_bwd(Tensor x, Tensor dp, Tensor idx, Tensor xm, optional<Tensor> gamma,
                      Tensor stats, optional<Tensor> dgamma, optional<Tensor> dbeta, Tensor slots,
                      optional<Tensor> zero_buf, int64_t K, int64_t S, int64_t P) {
  check_nhwc_bf16(x, "x");
  dp = dp.contiguous(kCL);
  check_nhwc_bf16(dp, "dp");
  TORCH_CHECK(dmp::guard::bf16_bytes_ok(x.size(0), x.size(2), x.size(3), x.size(1)),
              "maxpool_bn_bwd: x over 2 GiB (32-bit offsets)");
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(dmp::bn_maxpool_supported(C, (int)K, (int)S, (int)P), "maxpool_bn_bwd: bad window");
  TORCH_CHECK(dp.size(0) == N && dp.size(1) == C &&
                  dp.size(2) == dmp::maxpool_out(H, (int)K, (int)S, (int)P) &&
                  dp.size(3) == dmp::maxpool_out(W, (int)K, (int)S, (int)P),
              "maxpool_bn_bwd: dp shape mismatch");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte && idx.sizes() == dp.sizes() &&
                  idx.is_contiguous(kCL),
              "maxpool_bn_bwd: idx mismatch");
  check_nhwc_bf16(xm, "xm");
  same_shape(xm, dp, "maxpool_bn_bwd: xm");
  check_bn_stats(stats, C);
  check_vecs({&gamma, &dgamma, &dbeta}, at::kFloat, C, "bn gamma / dgamma / dbeta");
  auto fopt = x.options().dtype(at::kFloat);
  auto part = bn_slots(slots, C, fopt);
  float* zb = other_slots(zero_buf, C, fopt, part);
  auto dx = at::empty_like(x);
  dmp::launch_maxpool_bn_bwd_fold(bf16(x), bf16(dp), idx.data_ptr<uint8_t>(), bf16(xm),
                                  ptr_or_null<float>(gamma), stats.data_ptr<float>(),
                                  ptr_or_null<float>(dgamma), ptr_or_null<float>(dbeta),
                                  part.data_ptr<float>(), zb, bf16(dx), N, H, W, C, cur_stream());
  return dx;
}

// Inference-time BatchNorm fold into the producing conv / GEMM (csrc/bn.hip):
// returns (w16 = bf16(w * s) with w's shape and memory format, t fp32 [CO],
// t bf16 [CO]), s = gamma / sqrt(running_var + eps), t = beta + (cbias - mean) * s.
std::vector<Tensor> bn_fold_weights(Tensor w, optional<Tensor> gamma, optional<Tensor> beta,
                                    Tensor rmean, Tensor rvar, optional<Tensor> cbias,
                                    double eps) {
  check_gpu(w, "w");
  TORCH_CHECK(w.scalar_type() == at::kFloat, "bn_fold_weights: fp32 master weight");
  const bool cl = w.dim() == 4 && w.is_contiguous(kCL);
  TORCH_CHECK(cl || w.is_contiguous(), "bn_fold_weights: contiguous or channels_last weight");
  const int64_t CO = w.size(0);
  const int64_t n = w.numel();
  TORCH_CHECK(n % CO == 0, "bn_fold_weights: weight [CO, ...] expected");
  check_vecs({&gamma, &beta, &cbias}, at::kFloat, CO, "bn_fold_weights: affine / bias tensors");
  check_vec(rmean, at::kFloat, CO, "bn_fold_weights: running mean");
  check_vec(rvar, at::kFloat, CO, "bn_fold_weights: running var");
  auto w16 = at::empty_like(w, w.options().dtype(at::kBFloat16));
  auto b32 = at::empty({CO}, w.options());
  auto b16 = at::empty({CO}, w.options().dtype(at::kBFloat16));
  dmp::launch_bn_fold_weights(w.data_ptr<float>(), ptr_or_null<float>(gamma),
                              ptr_or_null<float>(beta), rmean.data_ptr<float>(),
                              rvar.data_ptr<float>(), ptr_or_null<float>(cbias), bf16(w16),
                              b32.data_ptr<float>(), bf16(b16), n, (int)CO, (float)eps,
                              cur_stream());
  return {w16, b32, b16};
}

// ------------------------------------------------------------------ pooling
// fused GAP + Linear head: [y [B, N] bf16, f [B, C] bf16 (pooled features, kept
// for the weight gradient)]
std::vector<Tensor> gap_linear_fwd(Tensor x, Tensor w, optional<Tensor> bias) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "gap_linear expects NCHW (channels_last) input");
  const int B = (int)x.size(0), C = (int)x.size(1), HW = (int)(x.size(2) * x.size(3));
  check_gpu(w, "w");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.dim() == 2 && w.size(1) == C &&
                  w.is_contiguous(), "gap_linear: w must be contiguous bf16 [N, C]");
  const int N = (int)w.size(0);
  TORCH_CHECK(dmp::gap_linear_supported(C, N), "gap_linear: unsupported C / N");
  if (has(bias)) {
    check_gpu(*bias, "bias");
    check_vec(*bias, at::kBFloat16, N, "gap_linear: bias");
  }
  auto y = at::empty({B, N}, x.options().memory_format(at::MemoryFormat::Contiguous));
  auto f = at::empty({B, C}, x.options().memory_format(at::MemoryFormat::Contiguous));
  dmp::launch_gap_linear_fwd(bf16(x), bf16(w), bf16_or_null(bias), bf16(y), bf16(f), B, HW, C, N,
                             cur_stream());
  return {y, f};
}

// dx [B, C, H, W] channels-last; gw [N, C] fp32 (+=), gb [N] fp32 (+=)
Tensor gap_linear_bwd(Tensor dy, Tensor f, Tensor w, Tensor gw, optional<Tensor> gb, int64_t H,
                      int64_t W) {
  dy = dy.contiguous();
  check_gpu(dy, "dy");
  check_gpu(f, "f");
  check_gpu(w, "w");
  check_gpu(gw, "gw");
  const int B = (int)f.size(0), C = (int)f.size(1), N = (int)w.size(0);
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.dim() == 2 && dy.size(0) == B &&
                  dy.size(1) == N, "gap_linear_bwd: dy must be bf16 [B, N]");
  TORCH_CHECK(f.scalar_type() == at::kBFloat16 && f.is_contiguous(), "gap_linear_bwd: f bf16 [B, C]");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.is_contiguous() && w.size(1) == C,
              "gap_linear_bwd: w bf16 [N, C]");
  check_vec(gw, at::kFloat, (int64_t)N * C, "gap_linear_bwd: gw [N, C]");
  TORCH_CHECK(dmp::gap_linear_supported(C, N), "gap_linear: unsupported C / N");
  if (has(gb)) {
    check_gpu(*gb, "gb");
    check_vec(*gb, at::kFloat, N, "gap_linear_bwd: gb");
  }
  auto dx = at::empty({B, C, H, W}, dy.options().memory_format(kCL));
  dmp::launch_gap_linear_bwd(bf16(dy), bf16(f), bf16(w), bf16(dx), gw.data_ptr<float>(),
                             ptr_or_null<float>(gb), B, (int)(H * W), C, N, cur_stream());
  return dx;
}

Tensor gap_fwd(Tensor x) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "gap expects NCHW (channels_last) input");
  const int N = (int)x.size(0), C = (int)x.size(1), HW = (int)(x.size(2) * x.size(3));
  TORCH_CHECK(C % 8 == 0, "gap: C must be a multiple of 8");
  auto y = at::empty({N, C}, x.options().memory_format(at::MemoryFormat::Contiguous));
  dmp::launch_gap_fwd(bf16(x), bf16(y), N, HW, C, cur_stream());
  return y;
}

Tensor gap_bwd(Tensor dy, int64_t H, int64_t W) {
  dy = dy.contiguous();
  check_gpu(dy, "dy");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.dim() == 2, "gap_bwd expects bf16 [N, C]");
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  TORCH_CHECK(C % 8 == 0, "gap: C must be a multiple of 8");
  auto dx = at::empty({N, C, H, W}, dy.options().memory_format(kCL));
  dmp::launch_gap_bwd(bf16(dy), bf16(dx), N, (int)(H * W), C, cur_stream());
  return dx;
}

std::vector<Tensor> maxpool_fwd(Tensor x, int64_t K, int64_t S, int64_t P, bool nchw_out,
                                bool relu_in) {
  if (S < 0) S = K;
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "maxpool expects 4-D input");
  const int N = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(K >= 1 && K <= 15 && S >= 1 && P >= 0 && 2 * P <= K,
              "maxpool: 1 <= K <= 15, S >= 1, 0 <= P <= K/2");
  const int Ho = dmp::maxpool_out(H, (int)K, (int)S, (int)P);
  const int Wo = dmp::maxpool_out(W, (int)K, (int)S, (int)P);
  TORCH_CHECK(Ho > 0 && Wo > 0, "maxpool: window larger than input");
  const bool nchw = nchw_out && C % 8 == 0;
  auto y = at::empty({N, C, Ho, Wo},
                     x.options().memory_format(nchw ? at::MemoryFormat::Contiguous : kCL));
  auto idx = at::empty({N, C, Ho, Wo}, x.options().dtype(at::kByte).memory_format(kCL));
  dmp::launch_maxpool_fwd(bf16(x), bf16(y), idx.data_ptr<uint8_t>(), N, H, W, C, (int)K, (int)S,
                          (int)P, cur_stream(), nchw, relu_in);
  if (nchw_out && !nchw) y = y.contiguous();
  return {y, idx};
}

Tensor maxpool_bwd(Tensor dy, Tensor idx, int64_t H, int64_t W, int64_t K, int64_t S, int64_t P) {
  if (S < 0) S = K;
  // an NCHW-contiguous dy (gradient of an nchw_out forward) is read in place
  const bool nchw = dy.dim() == 4 && dy.size(1) % 8 == 0 && dy.is_contiguous() &&
                    !dy.is_contiguous(kCL);
  if (!nchw) {
    dy = dy.contiguous(kCL);
    check_nhwc_bf16(dy, "dy");
  } else {
    check_gpu(dy, "dy");
  }
  TORCH_CHECK(idx.sizes() == dy.sizes() && idx.is_contiguous(kCL), "maxpool idx mismatch");
  const int N = (int)dy.size(0), C = (int)dy.size(1);
  TORCH_CHECK(dy.size(2) == dmp::maxpool_out((int)H, (int)K, (int)S, (int)P) &&
                  dy.size(3) == dmp::maxpool_out((int)W, (int)K, (int)S, (int)P),
              "maxpool_bwd: shape mismatch");
  // gather-form kernel writes every input element (un-pooled borders get 0)
  Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(kCL));
  dmp::launch_maxpool_bwd(bf16(dy), idx.data_ptr<uint8_t>(), bf16(dx), N, (int)H, (int)W, C,
                          (int)K, (int)S, (int)P, cur_stream(), nchw);
  return dx;
}

// dx = y > 0 ? dy : 0 over dense bf16 tensors of one layout (out may alias dy)
Tensor relu_bwd(Tensor dy, Tensor y, optional<Tensor> out) {
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kBFloat16, "relu_bwd: bf16 GPU tensors");
  const auto mf = y.dim() == 4 && y.is_contiguous(kCL) && !y.is_contiguous()
                      ? kCL
                      : at::MemoryFormat::Contiguous;
  // the kernel reads / writes 16-B vectors over one dense layout: a strided y is
  // made dense in the layout dy is brought to, and an operand that is dense but
  // not 16-B aligned (an offset slice such as x[..., 1:]) goes through an aligned
  // copy (fresh allocations are 256-B aligned)
  y = y.contiguous(mf);
  dy = dy.contiguous(mf);
  if (!aligned(y)) y = y.clone(mf);
  if (!aligned(dy)) dy = dy.clone(mf);
  TORCH_CHECK(dy.sizes() == y.sizes() && dy.scalar_type() == at::kBFloat16, "relu_bwd: dy shape");
  Tensor dst = has(out) ? *out : at::empty_like(dy);
  TORCH_CHECK(dst.sizes() == y.sizes() && dst.is_contiguous(mf) &&
                  dst.scalar_type() == at::kBFloat16,
              "relu_bwd: out layout");
  Tensor dx = aligned(dst) ? dst : at::empty_like(dy);
  dmp::launch_relu_bwd(bf16(dy), bf16(y), bf16(dx), y.numel(), cur_stream());
  if (!dx.is_same(dst)) dst.copy_(dx);
  return dst;
}

}  // namespace

void bind_norm_pool(pybind11::module_& m) {
  m.def("bn_fold_weights", &bn_fold_weights,
        "inference-time BatchNorm fold: (bf16 w * s, fp32 shift, bf16 shift)", py::arg("w"),
        py::arg("gamma"), py::arg("beta"), py::arg("rmean"), py::arg("rvar"),
        py::arg("cbias") = py::none(), py::arg("eps") = 1e-5);
  m.def("bn_fwd_from_partials", &bn_fwd_from_partials, "BN forward from conv-epilogue partials",
        py::arg("x"), py::arg("part"), py::arg("G"), py::arg("res"), py::arg("gamma"),
        py::arg("beta"), py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"),
        py::arg("eps"), py::arg("relu"), py::arg("want_mask") = false);
  m.def("bn_fwd_fold", &bn_fwd_fold, "BN forward, finalize folded into the apply",
        py::arg("x"), py::arg("part"), py::arg("have_partials"), py::arg("res") = py::none(),
        py::arg("gamma") = py::none(), py::arg("beta") = py::none(),
        py::arg("running_mean") = py::none(), py::arg("running_var") = py::none(),
        py::arg("momentum") = 0.1, py::arg("eps") = 1e-5, py::arg("relu") = false,
        py::arg("want_mask") = false, py::arg("zero_buf") = py::none());
  m.def("bn_bwd_fold", &bn_bwd_fold, "BN backward, finalize folded into the apply",
        py::arg("x"), py::arg("dy"), py::arg("y"), py::arg("gamma"), py::arg("stats"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("relu"), py::arg("want_dres"),
        py::arg("slots"), py::arg("mask") = py::none(), py::arg("zero_buf") = py::none());
  m.def("bn_maxpool_supported",
        [](int64_t C, int64_t K, int64_t S, int64_t P) {
          return dmp::bn_maxpool_supported((int)C, (int)K, (int)S, (int)P);
        },
        "fused BN + ReLU + max pool applies to (C, K, S, P)");
  m.def("bn_relu_maxpool_fwd", &bn_relu_maxpool_fwd,
        "BN + ReLU + max pool forward, finalize folded in -> (y, idx, stats, x at the taps)",
        py::arg("x"),
        py::arg("part"), py::arg("have_partials"), py::arg("gamma"), py::arg("beta"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("momentum"), py::arg("eps"),
        py::arg("zero_buf"), py::arg("K"), py::arg("S"), py::arg("P"));
  m.def("maxpool_bn_bwd", &maxpool_bn_bwd, "backward of bn_relu_maxpool_fwd -> dx", py::arg("x"),
        py::arg("dp"), py::arg("idx"), py::arg("xm"), py::arg("gamma"), py::arg("stats"), py::arg("dgamma"),
        py::arg("dbeta"), py::arg("slots"), py::arg("zero_buf"), py::arg("K"), py::arg("S"),
        py::arg("P"));
  m.def("bn_fwd", &bn_fwd, "NHWC batchnorm(+residual)(+relu) forward", py::arg("x"),
        py::arg("res"), py::arg("gamma"), py::arg("beta"), py::arg("running_mean"),
        py::arg("running_var"), py::arg("momentum"), py::arg("eps"), py::arg("training"),
        py::arg("relu"), py::arg("slots") = py::none(), py::arg("want_mask") = false);
  m.def("bn_bwd", &bn_bwd, "NHWC batchnorm(+residual)(+relu) backward", py::arg("x"),
        py::arg("dy"), py::arg("y"), py::arg("gamma"), py::arg("stats"), py::arg("dgamma"),
        py::arg("dbeta"), py::arg("relu"), py::arg("want_dres"), py::arg("slots") = py::none(),
        py::arg("mask") = py::none(), py::arg("batch_stats") = true);
  m.def("relu_bwd", &relu_bwd, "ReLU backward from the saved output", py::arg("dy"), py::arg("y"),
        py::arg("out") = py::none());
  m.def("gap_fwd", &gap_fwd, "NHWC global average pool forward");
  m.def("gap_linear_fwd", &gap_linear_fwd, "fused NHWC global average pool + Linear forward",
        py::arg("x"), py::arg("w"), py::arg("bias") = py::none());
  m.def("gap_linear_bwd", &gap_linear_bwd, "fused GAP + Linear backward (dx, dW +=, db +=)",
        py::arg("dy"), py::arg("f"), py::arg("w"), py::arg("gw"), py::arg("gb") = py::none(),
        py::arg("H"), py::arg("W"));
  m.def("gap_linear_supported",
        [](int64_t C, int64_t N) { return dmp::gap_linear_supported((int)C, (int)N); },
        "fused GAP + Linear head applies to C channels / N classes");
  m.def("gap_bwd", &gap_bwd, "NHWC global average pool backward");
  m.def("maxpool_fwd", &maxpool_fwd, "NHWC KxK / stride S / pad P max pool forward",
        py::arg("x"), py::arg("K"), py::arg("S") = -1, py::arg("P") = 0,
        py::arg("nchw_out") = false, py::arg("relu_in") = false);
  m.def("maxpool_bwd", &maxpool_bwd, "NHWC KxK / stride S / pad P max pool backward",
        py::arg("dy"), py::arg("idx"), py::arg("H"), py::arg("W"), py::arg("K"),
        py::arg("S") = -1, py::arg("P") = 0);
}

}  // namespace dmp::bind
