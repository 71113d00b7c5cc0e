// conv.hip, conv_wgrad.hip, conv_small.hip, stem.hip, im2col.hip: convolutions.
// x: bf16 channels_last [B, CI, H, W]; w: bf16 channels_last [CO, CI, R, S].
#include "util.h"

namespace dmp::bind {
namespace {

struct ConvGeom {
  int B, CI, H, W, CO, R, S, OH, OW;
};

ConvGeom geom_of(const Tensor& x, const Tensor& w, int64_t OH, int64_t OW) {
  return {(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)w.size(0),
          (int)w.size(2), (int)w.size(3), (int)OH, (int)OW};
}

// cfg is a halo-tile id whose plan applies to this 3x3 geometry over C channels
bool halo_takes(int64_t cfg, int H, int W, int C, int R, int S, int64_t stride, int64_t pad) {
  return cfg >= dmp::conv_halo_base() && cfg < dmp::conv_halo_base() + dmp::conv_num_halo_configs() &&
         stride == 1 && pad == 1 &&
         dmp::conv_halo_ok((int)cfg, H, W, C, R, S, (int)stride, (int)pad);
}

// halo_cfg: the cfg id of a call that a halo tile certainly takes when it applies
// (-1: none).  Those tiles step 32 input channels at a time: CI % 32 == 0 will do.
ConvGeom conv_geom(const Tensor& x, const Tensor& w, int64_t stride, int64_t pad,
                   int64_t halo_cfg = -1) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "conv: 4-D tensors expected");
  TORCH_CHECK(w.size(1) == x.size(1), "conv: weight/input channel mismatch");
  TORCH_CHECK(stride >= 1 && pad >= 0, "conv: bad stride/pad");
  const int64_t OH = dmp::guard::conv_out(x.size(2), pad, w.size(2), stride);
  const int64_t OW = dmp::guard::conv_out(x.size(3), pad, w.size(3), stride);
  TORCH_CHECK(OH > 0 && OW > 0, "conv: empty output");
  // the kernels address operands with 32-bit byte offsets into buffer descriptors
  // (checked on the 64-bit sizes, before anything is narrowed to int)
  TORCH_CHECK(dmp::guard::conv_offsets_ok(x.size(0), x.size(2), x.size(3), x.size(1), OH, OW,
                                          w.size(0), w.size(2), w.size(3)),
              "native conv: tensor too large for 32-bit byte offsets");
  auto g = geom_of(x, w, OH, OW);
  const bool ci32 = g.CI % 32 == 0 && halo_takes(halo_cfg, g.H, g.W, g.CI, g.R, g.S, stride, pad);
  TORCH_CHECK((g.CI % 64 == 0 || ci32) && g.CO % 64 == 0,
              "native conv needs CI % 64 == 0 and CO % 64 == 0 (got ", g.CI, ", ", g.CO, ")");
  return g;
}

void check_dy(const Tensor& dy, const ConvGeom& g, const char* what) {
  TORCH_CHECK(dy.size(0) == g.B && dy.size(1) == g.CO && dy.size(2) == g.OH && dy.size(3) == g.OW,
              what, ": dy shape mismatch");
}

// residual operand of a fused epilogue, brought to channels_last
Tensor addend_cl(const Tensor& addend) {
  Tensor t = addend.contiguous(kCL);
  check_nhwc_bf16(t, "addend");
  return t;
}

std::vector<Tensor> conv_fwd(Tensor x, Tensor w, int64_t stride, int64_t pad, bool want_stats,
                             int64_t cfg, optional<Tensor> slots, optional<Tensor> bias,
                             bool relu, optional<Tensor> addend) {
  check_nhwc_bf16(x, "x");
  check_weight_cl(w, at::kBFloat16, "conv weight");
  // (a statistics forward with a bias / ReLU / addend leaves the halo tiles: launch_halo)
  const bool plain = !(want_stats && (has(bias) || relu || has(addend)));
  auto g = conv_geom(x, w, stride, pad, plain ? cfg : -1);
  auto y = at::empty({g.B, g.CO, g.OH, g.OW}, x.options().memory_format(kCL));
  check_vecs({&bias}, at::kFloat, g.CO, "conv bias");
  Tensor part;
  int64_t G = 0;
  if (want_stats) {
    G = dmp::kBnSlots;
    part = bn_slots(slots, g.CO, x.options());
  }
  Tensor add_t;
  if (has(addend)) {
    // residual added before the ReLU (inference-time BatchNorm fold, ops/eval_fold.py)
    add_t = addend_cl(*addend);
    same_shape(add_t, y, "conv_fwd: addend / output");
  }
  dmp::launch_conv_fwd(bf16(x), bf16(w), bf16(y), ptr_or_null<float>(part), g.B, g.H, g.W, g.CI,
                       g.OH, g.OW, g.CO, g.R, g.S, (int)stride, (int)pad, (int)cfg, cur_stream(),
                       ptr_or_null<float>(bias), relu, bf16_or_null(add_t));
  return {y, part, at::scalar_tensor(G, at::kLong)};
}

void conv_weight_transpose_batched(Tensor src, Tensor dst, Tensor table, int64_t max_elems) {
  check_gpu(src, "src");
  check_gpu(dst, "dst");
  TORCH_CHECK(src.scalar_type() == at::kBFloat16 && dst.scalar_type() == at::kBFloat16 &&
                  src.numel() == dst.numel(),
              "batched transpose: src/dst must be equal-size bf16 buffers");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong && table.dim() == 2 &&
                  table.size(1) == 4 && table.is_contiguous(),
              "batched transpose: table must be a [n, 4] int64 GPU tensor");
  dmp::launch_conv_weight_transpose_batched(bf16(src), bf16(dst), i64(table), (int)table.size(0),
                                            (long long)max_elems, cur_stream());
}

Tensor conv_dgrad(Tensor dy, Tensor w, int64_t H, int64_t W, int64_t stride, int64_t pad,
                  int64_t cfg, optional<Tensor> wt_pre, optional<Tensor> addend,
                  bool addend_sub, optional<Tensor> addend_mask) {
  dy = dy.contiguous(kCL);
  check_nhwc_bf16(dy, "dy");
  check_weight_cl(w, at::kBFloat16, "conv weight");
  const int B = (int)dy.size(0);
  ConvGeom g{B, (int)w.size(1), (int)H, (int)W, (int)w.size(0), (int)w.size(2), (int)w.size(3),
             (int)dy.size(2), (int)dy.size(3)};
  TORCH_CHECK(dy.size(1) == g.CO, "dgrad: dy channels mismatch");
  TORCH_CHECK((g.H + 2 * pad - g.R) / stride + 1 == g.OH && (g.W + 2 * pad - g.S) / stride + 1 == g.OW,
              "dgrad: geometry mismatch");
  // (the halo tiles reduce over dY's channels 32 at a time)
  const bool co32 =
      g.CO % 32 == 0 && halo_takes(cfg, g.H, g.W, g.CO, g.R, g.S, stride, pad);
  TORCH_CHECK(g.CI % 64 == 0 && (g.CO % 64 == 0 || co32), "native dgrad needs CI, CO % 64 == 0");
  Tensor wt;
  if (has(wt_pre)) {
    wt = *wt_pre;   // pre-transposed [CI][R][S][CO] (batched per step by the arena)
    check_gpu(wt, "wt");
    check_vec(wt, at::kBFloat16, (int64_t)g.CI * g.R * g.S * g.CO,
              "dgrad: pre-transposed weight [CI, R, S, CO]");
  } else {
    wt = at::empty({g.CI, g.R, g.S, g.CO}, w.options().memory_format(at::MemoryFormat::Contiguous));
    dmp::launch_conv_weight_transpose(bf16(w), bf16(wt), g.CO, g.R * g.S, g.CI, cur_stream());
  }
  auto dx = at::empty({B, g.CI, g.H, g.W}, dy.options().memory_format(kCL));
  Tensor add_t;
  if (has(addend)) {
    add_t = addend_cl(*addend);
    if (addend_sub) {
      // gradient of x[:, :, ::2, ::2] (a 1x1 / stride-2 shortcut's input): added on
      // the stride-2 data gradient's parity class (0, 0)
      TORCH_CHECK(stride == 2, "dgrad: a subsampled addend needs stride 2");
      TORCH_CHECK(add_t.size(0) == B && add_t.size(1) == g.CI && add_t.size(2) == (g.H + 1) / 2 &&
                      add_t.size(3) == (g.W + 1) / 2,
                  "dgrad: subsampled addend must be [B, CI, ceil(H/2), ceil(W/2)]");
    } else {
      same_shape(add_t, dx, "dgrad: addend / input");
    }
  }
  // deferred ReLU mask of the addend (the residual BN backward's dres not written)
  const uint8_t* amask = nullptr;
  if (has(addend_mask)) {
    TORCH_CHECK(add_t.defined(), "dgrad: addend_mask without an addend");
    amask = bit_mask_ptr(*addend_mask, add_t.numel(), "dgrad: addend_mask [pixels, C/8]");
  }
  dmp::launch_conv_dgrad(bf16(dy), bf16(wt), bf16(dx), B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.R,
                         g.S, (int)stride, (int)pad, (int)cfg, cur_stream(), bf16_or_null(add_t),
                         add_t.defined() && addend_sub, amask);
  return dx;
}

// dx[:, :, ::2, ::2] += xs in place (both channels_last bf16)
void add_subsampled2(Tensor dx, Tensor xs) {
  check_nhwc_bf16(dx, "dx");
  check_nhwc_bf16(xs, "xs");
  TORCH_CHECK(dx.dim() == 4 && dx.size(1) % 8 == 0 && xs.size(0) == dx.size(0) &&
                  xs.size(1) == dx.size(1) && xs.size(2) == (dx.size(2) + 1) / 2 &&
                  xs.size(3) == (dx.size(3) + 1) / 2,
              "add_subsampled2: xs must be [B, C, ceil(H/2), ceil(W/2)] of dx [B, C, H, W]");
  dmp::launch_add_subsampled2(bf16(dx), bf16(xs), (int)dx.size(0), (int)dx.size(2),
                              (int)dx.size(3), (int)dx.size(1), cur_stream());
}

// x[:, :, ::2, ::2] of a channels_last bf16 activation, gathered (channels_last out)
Tensor subsample2(Tensor x) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(1) % 8 == 0, "subsample2: [B, C, H, W] with C % 8 == 0");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  auto xs = at::empty({B, C, (H + 1) / 2, (W + 1) / 2}, x.options().memory_format(kCL));
  dmp::launch_subsample2(bf16(x), bf16(xs), (int)B, (int)H, (int)W, (int)C, cur_stream());
  return xs;
}

void conv_wgrad(Tensor dy, Tensor x, Tensor dw, int64_t stride, int64_t pad, int64_t cfg,
                optional<Tensor> dbias) {
  dy = dy.contiguous(kCL);
  check_nhwc_bf16(dy, "dy");
  check_nhwc_bf16(x, "x");
  check_weight_cl(dw, at::kFloat, "dw");
  auto g = conv_geom(x, dw, stride, pad);
  check_dy(dy, g, "wgrad");
  check_vecs({&dbias}, at::kFloat, g.CO, "wgrad: dbias");
  float* db = ptr_or_null<float>(dbias);
  Tensor ws;   // slab-mode halo cfg: per-split partials, reduced into dw after the kernel
  if (db == nullptr) {
    const long long se = dmp::conv_wgrad_halo_slab_elems((int)cfg, g.B, g.H, g.W, g.CI, g.CO, g.R,
                                                         g.S, (int)stride, (int)pad);
    if (se > 0) ws = at::empty({(int64_t)se}, dw.options().memory_format(at::MemoryFormat::Contiguous));
  }
  dmp::launch_conv_wgrad(bf16(dy), bf16(x), dw.data_ptr<float>(), g.B, g.H, g.W, g.CI, g.OH, g.OW,
                         g.CO, g.R, g.S, (int)stride, (int)pad, (int)cfg, cur_stream(), db,
                         ptr_or_null<float>(ws));
}

// few-input-channel (stem) convolutions: x any dense bf16 4-D layout,
// w bf16 channels_last [CO, CI, R, S] with CO % 64 == 0 and R*S*CI <= 384
ConvGeom small_geom(const Tensor& x, const Tensor& w, int64_t stride, int64_t pad) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "small conv: 4-D tensors expected");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, "small conv: x must be bf16 GPU");
  TORCH_CHECK(w.size(1) == x.size(1), "small conv: weight/input channel mismatch");
  TORCH_CHECK(stride >= 1 && pad >= 0 && w.size(2) <= 255 && w.size(3) <= 255,
              "small conv: bad geometry");
  TORCH_CHECK(w.size(0) % 64 == 0, "small conv: CO must be a multiple of 64");
  TORCH_CHECK(w.size(1) * w.size(2) * w.size(3) <= dmp::conv_small_max_k(),
              "small conv: R*S*CI too large");
  const int64_t OH = dmp::guard::conv_out(x.size(2), pad, w.size(2), stride);
  const int64_t OW = dmp::guard::conv_out(x.size(3), pad, w.size(3), stride);
  TORCH_CHECK(OH > 0 && OW > 0, "small conv: empty output");
  TORCH_CHECK(dmp::guard::small_conv_ok(x.size(0), OH, OW, w.size(0), x.numel()),
              "small conv: tensor too large for 32-bit indexing");
  return geom_of(x, w, OH, OW);
}

// ImageNet stem (csrc/stem.hip): x [B, 3, H, W] channels_last bf16, w [64, 3, 7, 7]
// channels_last bf16 -> (y [B, 64, H/2, W/2] channels_last, BN slots, xs for the wgrad)
void check_stem_weight(const Tensor& w, at::ScalarType dt, const char* name) {
  check_weight_cl(w, dt, name);
  TORCH_CHECK(w.size(0) == 64 && w.size(1) == 3 && w.size(2) == 7 && w.size(3) == 7, name,
              " must be [64, 3, 7, 7]");
}

std::vector<Tensor> stem_fwd(Tensor x, Tensor w, bool want_stats, optional<Tensor> slots,
                             optional<Tensor> bias, bool relu) {
  check_gpu(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 4 && x.size(1) == 3 &&
                  x.is_contiguous(kCL),
              "stem: x must be a channels_last bf16 [B, 3, H, W] tensor");
  check_stem_weight(w, at::kBFloat16, "stem: w");
  const int64_t B = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(dmp::stem_supported((int)H, (int)W), "stem: unsupported input size ", H, "x", W);
  TORCH_CHECK(dmp::guard::stem_batch_ok(B, H, W), "stem: batch too large");
  auto xs = at::empty({B, H / 2, W / 2, 16}, x.options());
  auto wp = at::empty({64, 256}, w.options());
  auto y = at::empty({B, 64, H / 2, W / 2}, x.options().memory_format(kCL));
  Tensor part;
  if (want_stats) part = bn_slots(slots, 64, x.options());
  if (has(bias)) {
    check_gpu(*bias, "bias");
    check_vec(*bias, at::kFloat, 64, "stem: bias");
  }
  auto st = cur_stream();
  dmp::launch_stem_s2d(bf16(x), bf16(xs), (int)B, (int)H, (int)W, st);
  dmp::launch_stem_wpack(bf16(w), bf16(wp), st);
  dmp::launch_stem_fwd(bf16(xs), bf16(wp), bf16(y), ptr_or_null<float>(part), (int)B, (int)H,
                       (int)W, st, ptr_or_null<float>(bias), relu);
  return {y, part, xs};
}

// dw (fp32 [64, 3, 7, 7] channels_last) += stem weight gradient from dY and the s2d input
void stem_wgrad(Tensor dy, Tensor xs, Tensor dw) {
  dy = dy.contiguous(kCL);
  check_nhwc_bf16(dy, "dy");
  check_gpu(xs, "xs");
  check_stem_weight(dw, at::kFloat, "stem: dw");
  TORCH_CHECK(xs.scalar_type() == at::kBFloat16 && xs.dim() == 4 && xs.size(3) == 16 &&
                  xs.is_contiguous(), "stem: bad s2d input");
  const int64_t B = xs.size(0), H = 2 * xs.size(1), W = 2 * xs.size(2);
  TORCH_CHECK(dy.size(0) == B && dy.size(1) == 64 && dy.size(2) == H / 2 && dy.size(3) == W / 2,
              "stem: dy shape mismatch");
  TORCH_CHECK(dmp::stem_supported((int)H, (int)W), "stem: unsupported input size");
  auto dwp = at::empty({64, 256}, dw.options().memory_format(at::MemoryFormat::Contiguous));
  auto st = cur_stream();
  dmp::launch_stem_wgrad(bf16(dy), bf16(xs), dwp.data_ptr<float>(), (int)B, (int)H, (int)W, st);
  dmp::launch_stem_wfold(dwp.data_ptr<float>(), dw.data_ptr<float>(), st);
}

// 3x3/s1/p1, CI <= 3, CO = 64 stems on MFMA (conv_small.hip stem3_*); DMP_STEM3=0
// keeps the VALU kernels (A/B)
bool stem3_route(int64_t CI, int64_t R, int64_t S, int64_t CO, int64_t stride, int64_t pad,
                 int64_t W) {
  static const bool on = [] {
    const char* e = std::getenv("DMP_STEM3");
    return e == nullptr || std::atoi(e) != 0;
  }();
  return on && std::max({CI, R, S, CO, stride, pad, W}) < (int64_t(1) << 30) &&
         dmp::stem3_supported((int)CI, (int)R, (int)S, (int)CO, (int)stride, (int)pad, (int)W);
}

bool stem3_applies(const ConvGeom& g, int64_t stride, int64_t pad) {
  return stem3_route(g.CI, g.R, g.S, g.CO, stride, pad, g.W);
}

std::vector<Tensor> conv_small_fwd(Tensor x, Tensor w, int64_t stride, int64_t pad,
                                   bool want_stats, optional<Tensor> slots) {
  check_weight_cl(w, at::kBFloat16, "conv weight");
  auto g = small_geom(x, w, stride, pad);
  auto y = at::empty({g.B, g.CO, g.OH, g.OW}, x.options().memory_format(kCL));
  Tensor part;
  int64_t G = 0;
  if (want_stats) {
    G = dmp::kBnSlots;
    part = bn_slots(slots, g.CO, x.options());
  }
  const int xbytes = (int)(2 * x.numel());
  const int sb = (int)x.stride(0), sh = (int)x.stride(2), sw = (int)x.stride(3),
            sc = (int)x.stride(1);
  if (stem3_applies(g, stride, pad)) {
    dmp::launch_stem3_fwd(bf16(x), xbytes, sb, sh, sw, sc, bf16(w), bf16(y),
                          ptr_or_null<float>(part), g.B, g.H, g.W, g.CI, cur_stream());
  } else {
    dmp::launch_conv_small_fwd(bf16(x), xbytes, sb, sh, sw, sc, bf16(w), bf16(y),
                               ptr_or_null<float>(part), g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO,
                               g.R, g.S, (int)stride, (int)pad, cur_stream());
  }
  return {y, part, at::scalar_tensor(G, at::kLong)};
}

void conv_small_wgrad(Tensor dy, Tensor x, Tensor dw, int64_t stride, int64_t pad) {
  dy = dy.contiguous(kCL);
  check_nhwc_bf16(dy, "dy");
  check_weight_cl(dw, at::kFloat, "dw");
  auto g = small_geom(x, dw, stride, pad);
  check_dy(dy, g, "small wgrad");
  const int xbytes = (int)(2 * x.numel());
  const int sb = (int)x.stride(0), sh = (int)x.stride(2), sw = (int)x.stride(3),
            sc = (int)x.stride(1);
  if (stem3_applies(g, stride, pad)) {
    dmp::launch_stem3_wgrad(bf16(dy), bf16(x), xbytes, sb, sh, sw, sc, dw.data_ptr<float>(), g.B,
                            g.H, g.W, g.CI, cur_stream());
    return;
  }
  const long long P = (long long)g.B * g.OH * g.OW;
  const int G = dmp::conv_small_wgrad_blocks(P, g.CO, g.R, g.S, g.CI);
  auto ws = at::empty({(int64_t)G * g.CO * g.R * g.S * g.CI}, dw.options());
  dmp::launch_conv_small_wgrad(bf16(dy), bf16(x), xbytes, sb, sh, sw, sc, dw.data_ptr<float>(),
                               ws.data_ptr<float>(), g.B, g.H, g.W, g.CI, g.OH, g.OW, g.CO, g.R,
                               g.S, (int)stride, (int)pad, cur_stream());
}

// The CIFAR stem's BatchNorm + ReLU backward and conv weight gradient in one pass
// (conv_small.hip stem3_bn_bwd_*).  dy, x0: channels_last bf16 [B, 64, H, W] (x0 =
// the stem conv's stored output, the BN's input); x: the conv's bf16 input, any
// dense layout; stats: the BN forward's [4, 64].  dgamma / dbeta (fp32 [64]) and
// dw (fp32 channels_last [64, CI, 3, 3]) are accumulated; None = frozen.  scratch:
// the layer's persistent zeroed fp32 buffer (left zeroed); zero_buf: the layer's
// forward BN slot sums, zeroed here.
void stem3_bn_bwd(Tensor dy, Tensor x0, Tensor x, Tensor stats, optional<Tensor> gamma,
                  optional<Tensor> dgamma, optional<Tensor> dbeta, optional<Tensor> dw,
                  Tensor scratch, optional<Tensor> zero_buf, int64_t blocks) {
  check_nhwc_bf16(dy, "dy");
  check_nhwc_bf16(x0, "x0");
  TORCH_CHECK(dy.dim() == 4 && x0.dim() == 4, "stem3_bn_bwd: 4-D dy / x0 expected");
  same_shape(dy, x0, "stem3_bn_bwd: dy / x0");
  TORCH_CHECK(x.dim() == 4 && x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  (x.is_contiguous() || x.is_contiguous(kCL)),
              "stem3_bn_bwd: x must be a dense 4-D bf16 GPU tensor");
  TORCH_CHECK(dy.device() == x.device() && x0.device() == x.device() &&
                  stats.device() == x.device() && scratch.device() == x.device(),
              "stem3_bn_bwd: tensors on different devices");
  const int64_t B = x.size(0), CI = x.size(1), H = x.size(2), W = x.size(3), C = dy.size(1);
  TORCH_CHECK(dy.size(0) == B && dy.size(2) == H && dy.size(3) == W,
              "stem3_bn_bwd: dy / x shape mismatch");
  TORCH_CHECK(CI >= 1 && CI <= 3 && dmp::stem3_supported((int)CI, 3, 3, (int)C, 1, 1, (int)W),
              "stem3_bn_bwd: needs a 3x3/s1/p1 stem with CI <= 3, CO = 64 and W % 8 == 0");
  // 32-bit element offsets into dy | x0 and byte offsets into x
  TORCH_CHECK(B > 0 && H > 0 && dmp::guard::small_conv_ok(B, H, W, 2 * C, x.numel()),
              "stem3_bn_bwd: tensor too large for 32-bit indexing");
  check_vec(stats, at::kFloat, 4 * C, "stem3_bn_bwd: stats [4, C]");
  check_vecs({&gamma, &dgamma, &dbeta}, at::kFloat, C, "stem3_bn_bwd: gamma / dgamma / dbeta");
  if (has(dw)) {
    check_weight_cl(*dw, at::kFloat, "stem3_bn_bwd: dw");
    TORCH_CHECK(dw->size(0) == C && dw->size(1) == CI && dw->size(2) == 3 && dw->size(3) == 3 &&
                    dw->device() == x.device(),
                "stem3_bn_bwd: dw must be [64, CI, 3, 3]");
  }
  TORCH_CHECK(scratch.is_cuda() && scratch.scalar_type() == at::kFloat &&
                  scratch.is_contiguous() &&
                  scratch.numel() >= dmp::stem3_bn_bwd_scratch_floats(),
              "stem3_bn_bwd: scratch must be a contiguous fp32 GPU tensor of at least ",
              dmp::stem3_bn_bwd_scratch_floats(), " elements");
  float* zb = nullptr;
  if (has(zero_buf)) {
    zb = bn_slots(zero_buf, C, x.options()).data_ptr<float>();
    TORCH_CHECK(zero_buf->device() == x.device(), "stem3_bn_bwd: zero_buf on another device");
  }
  TORCH_CHECK(blocks >= 0 && blocks <= (1 << 20), "stem3_bn_bwd: bad block target");
  TORCH_CHECK(dmp::stem3_bn_bwd_steps(B * H * W, (int)blocks) > 0, "stem3_bn_bwd: bad grid");
  dmp::launch_stem3_bn_bwd(bf16(dy), bf16(x0), bf16(x), (int)(2 * x.numel()), (int)x.stride(0),
                           (int)x.stride(2), (int)x.stride(3), (int)x.stride(1),
                           stats.data_ptr<float>(), ptr_or_null<float>(gamma),
                           ptr_or_null<float>(dgamma), ptr_or_null<float>(dbeta),
                           ptr_or_null<float>(dw), scratch.data_ptr<float>(), zb, (int)B, (int)H,
                           (int)W, (int)CI, (int)blocks, cur_stream());
}

// ----------------------------------------------------------------- im2col
// x: bf16 channels_last [B, CI, H, W] -> [B*OH*OW, Kp] patch rows, k = (r, s, ci)
Tensor im2col(Tensor x, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t Kp) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "im2col: 4-D input");
  const int B = (int)x.size(0), CI = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  TORCH_CHECK(R >= 1 && S >= 1 && stride >= 1 && pad >= 0, "im2col: bad geometry");
  const int OH = (int)((H + 2 * pad - R) / stride + 1), OW = (int)((W + 2 * pad - S) / stride + 1);
  TORCH_CHECK(OH > 0 && OW > 0, "im2col: window larger than the padded input");
  const int64_t K = R * S * CI;
  TORCH_CHECK(Kp >= K && Kp % 8 == 0, "im2col: Kp must be >= R*S*CI and a multiple of 8");
  TORCH_CHECK(2LL * B * OH * OW * Kp < (1LL << 40), "im2col: patch matrix too large");
  Tensor cols = at::empty({(int64_t)B * OH * OW, Kp}, x.options());
  dmp::launch_im2col(bf16(x), bf16(cols), B, H, W, CI, OH, OW, (int)R, (int)S, (int)stride,
                     (int)pad, (int)K, (int)Kp, cur_stream());
  return cols;
}

// dcols [B*OH*OW, Kp] -> dX bf16 channels_last [B, CI, H, W]
Tensor col2im(Tensor dcols, int64_t B, int64_t CI, int64_t H, int64_t W, int64_t R, int64_t S,
              int64_t stride, int64_t pad) {
  check_gpu(dcols, "dcols");
  TORCH_CHECK(dcols.scalar_type() == at::kBFloat16 && dcols.dim() == 2 && dcols.is_contiguous(),
              "col2im: dcols must be a contiguous bf16 [M, Kp] tensor");
  const int OH = (int)((H + 2 * pad - R) / stride + 1), OW = (int)((W + 2 * pad - S) / stride + 1);
  TORCH_CHECK(dcols.size(0) == B * OH * OW && dcols.size(1) >= R * S * CI,
              "col2im: dcols shape does not match the conv geometry");
  Tensor dx = at::empty({B, CI, H, W}, dcols.options().memory_format(kCL));
  dmp::launch_col2im(bf16(dcols), bf16(dx), (int)B, (int)H, (int)W, (int)CI, OH, OW, (int)R,
                     (int)S, (int)stride, (int)pad, (int)dcols.size(1), cur_stream());
  return dx;
}

// ------------------------------------------------------------ config tables
std::vector<std::vector<int64_t>> conv_configs() {
  return config_table(dmp::conv_num_configs(), dmp::conv_config_info, 5);
}

// halo-tile cfg ids applicable to a conv over a [*, C, H, W] input (3x3 / stride 1 / pad 1)
std::vector<int64_t> conv_halo_configs(int64_t H, int64_t W, int64_t C, int64_t R, int64_t S,
                                       int64_t stride, int64_t pad) {
  std::vector<int64_t> out;
  config_ids(out, dmp::conv_halo_base(), dmp::conv_num_halo_configs(), [&](int c) {
    return dmp::conv_halo_ok(c, (int)H, (int)W, (int)C, (int)R, (int)S, (int)stride, (int)pad);
  });
  return out;
}

// stride-2 halo dgrad cfg ids applicable to dX [*, CI, H, W] from dY [*, CO, OH, OW]
std::vector<int64_t> conv_dgrad_s2_configs(int64_t H, int64_t W, int64_t OH, int64_t OW,
                                           int64_t CO, int64_t CI, int64_t R, int64_t S,
                                           int64_t stride, int64_t pad) {
  std::vector<int64_t> out;
  config_ids(out, dmp::conv_dgrad_s2_base(), dmp::conv_dgrad_s2_num_configs(), [&](int c) {
    return dmp::conv_dgrad_s2_ok(c, (int)H, (int)W, (int)OH, (int)OW, (int)CO, (int)CI, (int)R,
                                 (int)S, (int)stride, (int)pad);
  });
  return out;
}

// halo wgrad cfg ids applicable to dW of a conv over [B, CI, H, W] -> CO channels
std::vector<int64_t> conv_wgrad_halo_configs(int64_t B, int64_t H, int64_t W, int64_t CI,
                                             int64_t CO, int64_t R, int64_t S, int64_t stride,
                                             int64_t pad) {
  std::vector<int64_t> out;
  for (int base : {dmp::conv_wgrad_halo_base(), dmp::conv_wgrad_halo_slab_base()})
    config_ids(out, base, dmp::conv_wgrad_num_halo_configs(), [&](int c) {
      return dmp::conv_wgrad_halo_ok(c, (int)B, (int)H, (int)W, (int)CI, (int)CO, (int)R, (int)S,
                                     (int)stride, (int)pad);
    });
  return out;
}

}  // namespace

void bind_conv(pybind11::module_& m) {
  m.def("conv_fwd", &conv_fwd, "NHWC bf16 implicit-GEMM conv forward (+BN partials)",
        py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"), py::arg("want_stats"),
        py::arg("cfg") = -1, py::arg("slots") = py::none(), py::arg("bias") = py::none(),
        py::arg("relu") = false, py::arg("addend") = py::none());
  m.def("conv_dgrad", &conv_dgrad, "NHWC bf16 implicit-GEMM conv data gradient", py::arg("dy"),
        py::arg("w"), py::arg("H"), py::arg("W"), py::arg("stride"), py::arg("pad"),
        py::arg("cfg") = -1, py::arg("wt") = py::none(), py::arg("addend") = py::none(),
        py::arg("addend_sub") = false, py::arg("addend_mask") = py::none());
  m.def("subsample2", &subsample2, "x[:, :, ::2, ::2] of a channels_last bf16 activation",
        py::arg("x"));
  m.def("add_subsampled2", &add_subsampled2, "dx[:, :, ::2, ::2] += xs in place",
        py::arg("dx"), py::arg("xs"));
  m.def("conv_weight_transpose_batched", &conv_weight_transpose_batched,
        "transpose every conv weight of a flat bf16 shadow in one launch");
  m.def("conv_wgrad", &conv_wgrad, "NHWC bf16 conv weight gradient (fp32 accumulate)",
        py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("stride"), py::arg("pad"),
        py::arg("cfg") = -1, py::arg("dbias") = py::none());
  m.def("conv_configs", &conv_configs, "[(id, BM, BN, BK, threads)] of the compiled conv tiles");
  m.def("conv_wgrad_halo_configs", &conv_wgrad_halo_configs,
        "3x3 stride-1 / stride-2 halo wgrad cfg ids applicable to (B, H, W, CI, CO, R, S, stride, pad)");
  m.def("conv_dgrad_s2_configs", &conv_dgrad_s2_configs,
        "3x3/stride-2 halo data-gradient cfg ids for (H, W, OH, OW, CO, CI, R, S, stride, pad)");
  m.def("conv_halo_configs", &conv_halo_configs,
        "3x3/stride-1 halo-tile cfg ids applicable to (H, W, C, R, S, stride, pad)");
  m.def("conv_halo_pm", [](bool on) { return dmp::conv_halo_pm(on); },
        "position-major halo tiles on 4 x 4 maps: set the process-wide switch, return the "
        "previous value (never inside a graph capture)", py::arg("on"));
  m.def("conv_halo_pm_ok",
        [](int64_t cfg, int64_t H, int64_t W, int64_t C, int64_t R, int64_t S, int64_t stride,
           int64_t pad) {
          return dmp::conv_halo_pm_ok((int)cfg, (int)H, (int)W, (int)C, (int)R, (int)S, (int)stride,
                                      (int)pad);
        },
        "halo cfg id runs position-major on (H, W, C, R, S, stride, pad) when the switch is on");
  m.def("stem_supported", [](int64_t H, int64_t W) { return dmp::stem_supported((int)H, (int)W); },
        "ImageNet 7x7/2 stem kernel applies to an H x W input");
  m.def("stem_fwd", &stem_fwd, "ImageNet stem conv forward (+BN partials) via space-to-depth",
        py::arg("x"), py::arg("w"), py::arg("want_stats"), py::arg("slots") = py::none(),
        py::arg("bias") = py::none(), py::arg("relu") = false);
  m.def("stem_wgrad", &stem_wgrad, "ImageNet stem conv weight gradient (fp32 +=)", py::arg("dy"),
        py::arg("xs"), py::arg("dw"));
  m.def("conv_small_fwd", &conv_small_fwd, "few-input-channel conv forward (+BN partials)",
        py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"), py::arg("want_stats"),
        py::arg("slots") = py::none());
  m.def("conv_small_wgrad", &conv_small_wgrad, "few-input-channel conv weight gradient (fp32 +=)",
        py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("stride"), py::arg("pad"));
  m.def("stem3_route", &stem3_route,
        "conv_small_fwd / conv_small_wgrad run the MFMA stem kernels for this geometry",
        py::arg("CI"), py::arg("R"), py::arg("S"), py::arg("CO"), py::arg("stride"),
        py::arg("pad"), py::arg("W"));
  m.def("stem3_bn_bwd_scratch_floats", [] { return (int64_t)dmp::stem3_bn_bwd_scratch_floats(); },
        "fp32 elements of stem3_bn_bwd's persistent scratch");
  m.def("stem3_bn_bwd", &stem3_bn_bwd,
        "CIFAR stem: BN + ReLU backward and conv weight gradient in one pass (all +=)",
        py::arg("dy"), py::arg("x0"), py::arg("x"), py::arg("stats"), py::arg("gamma"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("dw"), py::arg("scratch"),
        py::arg("zero_buf") = py::none(), py::arg("blocks") = 0);
  m.def("im2col", &im2col, "NHWC patch rows [B*OH*OW, Kp], k = (r, s, ci), zero-padded",
        py::arg("x"), py::arg("R"), py::arg("S"), py::arg("stride"), py::arg("pad"), py::arg("Kp"));
  m.def("col2im", &col2im, "gather-form inverse of im2col -> channels_last dX", py::arg("dcols"),
        py::arg("B"), py::arg("CI"), py::arg("H"), py::arg("W"), py::arg("R"), py::arg("S"),
        py::arg("stride"), py::arg("pad"));
}

}  // namespace dmp::bind
