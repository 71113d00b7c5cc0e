// Bindings of dwconv.hip (depthwise K x K conv, three passes) and
// layer_scale.hip (the layer-scale residual add and its backward).
#include "dwconv_plan.h"
#include "util.h"

namespace dmp::bind {
namespace {

struct DwGeom {
  int N, H, W, C, K;
};

// x: [N, C, H, W] channels_last bf16; w: the [C, 1, K, K] bf16 shadow ([C][K*K] in memory)
DwGeom dw_geom(const Tensor& x, const Tensor& w, const char* fn) {
  check_nhwc_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, fn, ": x must be [N, C, H, W] channels_last");
  check_gpu(w, "w");
  TORCH_CHECK(w.dim() == 4 && w.size(1) == 1 && w.size(2) == w.size(3) &&
                  w.size(0) == x.size(1) && w.is_contiguous(kCL),
              fn, ": weight must be a dense [C, 1, K, K] tensor with C = ", x.size(1), ", got ",
              w.sizes());
  TORCH_CHECK(w.device() == x.device(), fn, ": weight must be on ", x.device());
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3), K = w.size(2);
  TORCH_CHECK(dmp::guard::dwconv_ok(N, H, W, C, K), fn, ": geometry [", N, ", ", H, ", ", W, ", ",
              C, "] with a ", K, " x ", K,
              " window is outside the depthwise kernels (K in {3, 5, 7}, C % 8 == 0, at most "
              "65535 images, the activation under 2 GiB for its 32-bit offsets)");
  return {(int)N, (int)H, (int)W, (int)C, (int)K};
}

// y = dwconv(x, w) + bias; flip + addend: the data gradient over dy, plus the
// residual stream's own gradient
Tensor dwconv_fwd(Tensor x, Tensor w, optional<Tensor> bias, bool flip, optional<Tensor> addend) {
  const DwGeom g = dw_geom(x, w, "dwconv_fwd");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16, "dwconv_fwd: weight must be bf16");
  check_vecs({&bias}, at::kFloat, g.C, "dwconv_fwd: bias");
  if (has(addend)) {
    check_nhwc_bf16(*addend, "addend");
    same_shape(*addend, x, "dwconv_fwd: addend");
    TORCH_CHECK(addend->is_contiguous(kCL), "dwconv_fwd: addend must be channels_last");
  }
  auto y = at::empty_like(x, x.options().memory_format(kCL));
  dmp::launch_dwconv(bf16(x), bf16(w), ptr_or_null<float>(bias), bf16_or_null(addend), bf16(y),
                     g.N, g.H, g.W, g.C, g.K, flip, cur_stream());
  return y;
}

// fp32 words of a layer's weight-gradient slab: a function of (C, K) alone, so a
// slab never has to be replaced when the batch or the map changes
int64_t dwconv_slab_numel(int64_t C, int64_t K) {
  TORCH_CHECK(dmp::guard::dwconv_ok(1, 1, 1, C, K), "dwconv_slab_numel: C = ", C, ", K = ", K,
              " is outside the depthwise kernels");
  return dmp::dwconv_slab_floats((int)C, (int)K);
}

// dw (fp32 [C, 1, K, K]) += weight gradient, db (fp32 [C]) += colsum(dy)
void dwconv_wgrad(Tensor dy, Tensor x, Tensor dw, optional<Tensor> db, optional<Tensor> slab) {
  const DwGeom g = dw_geom(x, dw, "dwconv_wgrad");
  TORCH_CHECK(dw.scalar_type() == at::kFloat, "dwconv_wgrad: dw must be fp32");
  check_nhwc_bf16(dy, "dy");
  same_shape(dy, x, "dwconv_wgrad: dy");
  TORCH_CHECK(dy.is_contiguous(kCL), "dwconv_wgrad: dy must be channels_last");
  check_vecs({&db}, at::kFloat, g.C, "dwconv_wgrad: db");
  const int64_t need = dwconv_slab_numel(g.C, g.K);
  Tensor sl;
  if (has(slab)) {
    TORCH_CHECK(slab->is_cuda() && slab->scalar_type() == at::kFloat && slab->is_contiguous() &&
                    slab->numel() >= need && slab->device() == x.device(),
                "dwconv_wgrad: slab must be a contiguous fp32 GPU tensor of at least ", need,
                " elements");
    sl = *slab;
  } else {
    sl = at::empty({need}, x.options().dtype(at::kFloat));
  }
  dmp::launch_dwconv_wgrad(bf16(dy), bf16(x), dw.data_ptr<float>(), ptr_or_null<float>(db),
                           sl.data_ptr<float>(), g.N, g.H, g.W, g.C, g.K, cur_stream());
}

// (TH, TW, CC, tiles_h, tiles_w, chunks, LDS bytes) of the forward / dgrad kernel
std::vector<int64_t> dwconv_plan(int64_t H, int64_t W, int64_t C, int64_t K) {
  const dmp::DwPlan p = dmp::plan_dwconv((int)H, (int)W, (int)C, (int)K);
  TORCH_CHECK(p.ok, "dwconv_plan: no plan for H ", H, " W ", W, " C ", C, " K ", K);
  return {p.TH, p.TW, p.CC, p.tiles_h, p.tiles_w, p.chunks, p.lds_bytes};
}

// ------------------------------------------------------------ layer scale
struct LsGeom {
  int64_t rows;
  int C, tokens;
};

LsGeom ls_geom(const Tensor& x, const Tensor& r, const Tensor& gamma,
               const optional<Tensor>& rscale, const char* fn) {
  check_rows_bf16(x, "x");
  check_rows_bf16(r, "r");
  same_shape(r, x, fn);
  TORCH_CHECK(x.dim() >= 2 && x.numel() > 0, fn, ": rows of channels expected");
  const int64_t C = x.size(-1), rows = x.numel() / C;
  TORCH_CHECK(C % 8 == 0 && C <= dmp::layer_scale_max_channels(), fn, ": C = ", C,
              " must be a multiple of 8, at most ", dmp::layer_scale_max_channels());
  check_vec(gamma, at::kFloat, C, "layer scale gamma");
  TORCH_CHECK(gamma.device() == x.device() && r.device() == x.device(), fn,
              ": operands must share a device");
  int64_t tokens = 1;
  if (has(rscale)) {
    const int64_t B = rscale->numel();
    TORCH_CHECK(B >= 1 && rows % B == 0 && rows / B <= INT32_MAX, fn,
                ": rscale needs one scale per sample, its count dividing the ", rows, " rows");
    check_vec(*rscale, at::kFloat, B, "rscale (one scale per sample)");
    TORCH_CHECK(rscale->device() == x.device(), fn, ": rscale must be on ", x.device());
    tokens = rows / B;
  }
  return {rows, (int)C, (int)tokens};
}

Tensor layer_scale_fwd(Tensor x, Tensor r, Tensor gamma, optional<Tensor> rscale) {
  const LsGeom g = ls_geom(x, r, gamma, rscale, "layer_scale_fwd");
  auto h = at::empty_like(x);
  dmp::launch_layer_scale_fwd(bf16(x), bf16(r), gamma.data_ptr<float>(), ptr_or_null<float>(rscale),
                              bf16(h), g.rows, g.C, g.tokens, cur_stream());
  return h;
}

// returns dr (undefined -> None when !need_dr); dgamma += its gradient when given
py::object layer_scale_bwd(Tensor dh, Tensor r, Tensor gamma, optional<Tensor> rscale,
                           optional<Tensor> dgamma, optional<Tensor> slots, bool need_dr) {
  const LsGeom g = ls_geom(dh, r, gamma, rscale, "layer_scale_bwd");
  check_vecs({&dgamma}, at::kFloat, g.C, "layer_scale_bwd: dgamma");
  Tensor sl;
  if (has(dgamma)) {
    const int64_t n = (int64_t)dmp::layer_scale_num_slots() * g.C;
    if (has(slots)) {
      check_vec(*slots, at::kFloat, n, "layer scale slots");
      sl = *slots;
    } else {
      sl = at::empty({n}, dh.options().dtype(at::kFloat));
    }
  }
  Tensor dr;
  if (need_dr) dr = at::empty_like(dh);
  if (!need_dr && !has(dgamma)) return py::none();
  dmp::launch_layer_scale_bwd(bf16(dh), bf16(r), gamma.data_ptr<float>(),
                              ptr_or_null<float>(rscale), bf16_or_null(dr),
                              ptr_or_null<float>(dgamma), ptr_or_null<float>(sl), g.rows, g.C,
                              g.tokens, cur_stream());
  return need_dr ? py::cast(dr) : py::none();
}

}  // namespace

void bind_dwconv(py::module_& m) {
  m.def("dwconv_fwd", &dwconv_fwd, "depthwise KxK conv, stride 1, pad K/2 (flip: data gradient)",
        py::arg("x"), py::arg("w"), py::arg("bias") = py::none(), py::arg("flip") = false,
        py::arg("addend") = py::none());
  m.def("dwconv_wgrad", &dwconv_wgrad, "depthwise conv weight (+ bias) gradient, slab-reduced",
        py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("db") = py::none(),
        py::arg("slab") = py::none());
  m.def("dwconv_slab_numel", &dwconv_slab_numel, "fp32 words of a layer's wgrad slab");
  m.def("dwconv_plan", &dwconv_plan, "(TH, TW, CC, tiles_h, tiles_w, chunks, lds) of a geometry");
  m.def("layer_scale_fwd", &layer_scale_fwd, "h = x + gamma * r (* rscale[sample])", py::arg("x"),
        py::arg("r"), py::arg("gamma"), py::arg("rscale") = py::none());
  m.def("layer_scale_bwd", &layer_scale_bwd, "dr and dgamma of layer_scale_fwd", py::arg("dh"),
        py::arg("r"), py::arg("gamma"), py::arg("rscale") = py::none(),
        py::arg("dgamma") = py::none(), py::arg("slots") = py::none(),
        py::arg("need_dr") = true);
  m.def("layer_scale_num_slots", &dmp::layer_scale_num_slots);
  m.def("layer_scale_max_channels", &dmp::layer_scale_max_channels);
}

}  // namespace dmp::bind
