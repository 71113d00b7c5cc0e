// gemm.hip, linear.hip: the bf16 MFMA GEMM of the linear layers, bias gradients
// and the padded-row weight copies of the im2col convs (im2col.hip).
#include "util.h"

namespace dmp::bind {
namespace {

// ----------------------------------------------------------- bias gradients
// out[n] += sum over rows of dy[..., n]; dy: bf16 with the channel dim
// innermost in memory (contiguous [.., N] or channels_last NCHW)
void colsum_acc(Tensor dy, Tensor out, optional<Tensor> slots) {
  check_gpu(dy, "dy");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16, "colsum_acc: dy must be bf16");
  int64_t N;
  if (dy.dim() == 4) {
    N = dy.size(1);
    if (!dy.is_contiguous(kCL)) dy = dy.contiguous(kCL);
  } else {
    N = dy.size(-1);
    dy = dy.contiguous();
  }
  TORCH_CHECK(N % 8 == 0, "colsum_acc: the summed-into dim must be a multiple of 8, got ", N);
  check_vec(out, at::kFloat, N, "colsum_acc: out");
  const int64_t M = dy.numel() / N;
  if (M == 0) return;
  // per-device persistent zeroed scratch (every call re-zeroes it; calls on one
  // stream are ordered, and a graph replays them in the same order)
  const int64_t need = (int64_t)dmp::colsum_num_slots() * N;
  Tensor sl;
  if (has(slots)) {
    TORCH_CHECK(slots->is_cuda() && slots->scalar_type() == at::kFloat &&
                    slots->is_contiguous() && slots->numel() >= need,
                "colsum_acc: slots must be a zeroed contiguous fp32 GPU tensor of >= ", need);
    sl = *slots;
  } else {
    sl = at::zeros({need}, out.options());
  }
  dmp::launch_colsum_acc(bf16(dy), out.data_ptr<float>(), sl.data_ptr<float>(), M, (int)N,
                         cur_stream());
}

void pad_rows_batched(Tensor src, Tensor dst, Tensor table, int64_t max_elems) {
  check_gpu(src, "src");
  check_gpu(dst, "dst");
  TORCH_CHECK(src.scalar_type() == at::kBFloat16 && dst.scalar_type() == at::kBFloat16,
              "pad_rows_batched: bf16 buffers");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong && table.dim() == 2 &&
                  table.size(1) == 5 && table.is_contiguous(),
              "pad_rows_batched: table must be a [n, 5] int64 GPU tensor");
  dmp::launch_pad_rows_batched(bf16(src), bf16(dst), i64(table), (int)table.size(0),
                               (long long)max_elems, cur_stream());
}

// ------------------------------------------------------------------- GEMM
// 2-D operand with a unit inner stride: checked and its row stride returned
int64_t mat_ld(const Tensor& t, at::ScalarType dt, int64_t rows, int64_t cols,
               const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.dim() == 2, name, " must be a 2-D ", dt,
              " GPU tensor");
  TORCH_CHECK(t.size(0) == rows && t.size(1) == cols, name, " is ", t.sizes(), ", expected [",
              rows, ", ", cols, "]");
  TORCH_CHECK(t.stride(1) == 1, name, " must have a unit inner stride");
  const int64_t ld = rows <= 1 ? cols : t.stride(0);
  TORCH_CHECK(ld >= cols, name, ": row stride smaller than the row");
  TORCH_CHECK(dmp::guard::rows_bytes_ok(t.element_size(), rows, ld), name,
              " exceeds the 2 GiB 32-bit offset range of the GEMM kernels");
  return ld;
}

// C = epilogue(sum_k A(m, k) B(n, k)); see csrc/gemm.hip.  mode 0: a [M,K], b [N,K];
// mode 1: a [M,K], b [K,N]; mode 2: a [K,M], b [K,N], c fp32 accumulated.
void gemm(int64_t mode, int64_t epi, int64_t cfg, Tensor a, Tensor b, Tensor c,
          optional<Tensor> c2, optional<Tensor> bias, optional<Tensor> aux,
          optional<Tensor> dbias, int64_t splits, bool relu, optional<Tensor> part, bool slab,
          optional<Tensor> auxmask) {
  TORCH_CHECK(!relu || epi == 0, "gemm: relu only with the store epilogue");
  TORCH_CHECK(mode >= 0 && mode <= 2, "gemm: mode must be 0 (fwd), 1 (dgrad) or 2 (wgrad)");
  TORCH_CHECK(c.dim() == 2 && a.dim() == 2 && b.dim() == 2, "gemm: 2-D operands expected");
  TORCH_CHECK((mode == 0 && (epi == 0 || epi == 1)) ||
                  (mode == 1 && (epi == 0 || epi == 2 || epi == 4)) || (mode == 2 && epi == 3),
              "gemm: epilogue ", epi, " not available in mode ", mode);
  TORCH_CHECK(dmp::gemm_config_ok((int)mode, (int)cfg), "gemm: config ", cfg,
              " is not available in mode ", mode);
  TORCH_CHECK(splits <= 1 || mode == 2,
              "gemm: split-K only in the weight-gradient mode, got splits ", splits, " in mode ",
              mode);
  const int64_t M = c.size(0), N = c.size(1);
  const int64_t K = mode == 2 ? a.size(0) : a.size(1);
  const int64_t lda = mat_ld(a, at::kBFloat16, mode == 2 ? K : M, mode == 2 ? M : K, "a");
  const int64_t ldb = mat_ld(b, at::kBFloat16, mode == 0 ? N : K, mode == 0 ? K : N, "b");
  const int64_t ldc = mat_ld(c, mode == 2 ? at::kFloat : at::kBFloat16, M, N, "c");
  if (M == 0 || N == 0) return;
  auto same_as_c = [&](const Tensor& t, const char* name) {
    TORCH_CHECK(mat_ld(t, at::kBFloat16, M, N, name) == ldc, name,
                " must have the output's row stride");
    TORCH_CHECK(aligned(t), name, " must be 16-byte aligned");
    return bf16(t);
  };
  uint16_t* c2p = nullptr;
  if (epi == 1) {
    TORCH_CHECK(has(c2), "gemm: GELU epilogue needs c2");
    c2p = same_as_c(*c2, "c2");
  }
  const uint16_t* auxp = nullptr;
  if (has(aux)) {
    TORCH_CHECK(epi == 0 || epi == 2 || epi == 4, "gemm: aux only with epilogues 0 / 2 / 4");
    auxp = same_as_c(*aux, "aux");
  }
  // deferred ReLU bit mask of the addend (ops/functional.py deferred residual mask)
  const uint8_t* amp = nullptr;
  if (has(auxmask)) {
    TORCH_CHECK(auxp != nullptr && epi == 0 && cfg >= 0,
                "gemm: auxmask needs an addend, the store epilogue and an MFMA tile config");
    TORCH_CHECK(ldc == N && N % 8 == 0, "gemm: auxmask needs a dense output with N % 8 == 0");
    amp = bit_mask_ptr(*auxmask, M * N, "gemm: auxmask [M * N / 8]");
  }
  TORCH_CHECK(epi != 2 || auxp != nullptr, "gemm: GELU-backward epilogue needs aux = h");
  TORCH_CHECK(epi != 4 || auxp != nullptr, "gemm: ReLU-backward epilogue needs aux = the input");
  if (has(bias)) {
    TORCH_CHECK(epi == 0 || epi == 1, "gemm: bias only in the forward epilogues");
    check_vec(*bias, at::kBFloat16, N, "gemm: bias");
    TORCH_CHECK(aligned(*bias, 8), "gemm: bias must be 8-byte aligned");
  }
  if (has(dbias)) {
    TORCH_CHECK(mode == 2, "gemm: dbias only in wgrad mode");
    check_vec(*dbias, at::kFloat, M, "gemm: dbias");
  }
  float* partp = nullptr;
  if (has(part)) {
    TORCH_CHECK(epi == 0 && cfg >= 0, "gemm: BN partial sums need the MFMA store epilogue");
    TORCH_CHECK(N % 8 == 0 && ldc % 8 == 0, "gemm: BN partial sums need N % 8 == 0");
    partp = bn_slots(part, N, c.options()).data_ptr<float>();
  }
  if (cfg >= 0) {
    // MFMA tiles: 16-B DMA pieces along k (row-major operand) or along the
    // row (k-strided operand), 8-B bf16x4 output stores
    TORCH_CHECK(aligned(a) && aligned(b),
                "gemm: operands must be 16-byte aligned for the MFMA kernels");
    // bf16 output rows are stored as 16-B pieces when ldc allows
    TORCH_CHECK(mode == 2 || aligned(c), "gemm: the bf16 output must be 16-byte aligned");
    TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0, "gemm: operand row strides must be multiples of 8");
    auto c8 = [](int64_t v) { return (v + 7) / 8 * 8; };
    if (mode == 0) TORCH_CHECK(K % 8 == 0, "gemm: K must be a multiple of 8 (else cfg -1)");
    if (mode == 1)
      TORCH_CHECK(K % 8 == 0 && (N % 8 == 0 || ldb >= c8(N)),
                  "gemm: K must be a multiple of 8, N too unless padded in b's row stride");
    // k-strided operands are fetched in 8-column pieces: a partial last piece
    // may read into the row padding, never past the row stride
    if (mode == 2)
      TORCH_CHECK((M % 8 == 0 || lda >= c8(M)) && (N % 8 == 0 || ldb >= c8(N)),
                  "gemm: wgrad M, N must be multiples of 8 or padded in the row stride");
    // bf16 outputs: 16-B row segments, or element stores when N / ldc are not
    // multiples of 8 (any width)
  }
  // wgrad split-K through a plain-store slab + reduce pass instead of atomics
  Tensor ws;
  if (slab && mode == 2 && cfg >= 0) {
    const int sp = dmp::gemm_effective_splits((int)K, (int)std::max<int64_t>(1, splits));
    if (sp > 1) ws = at::empty({(int64_t)sp * M * N}, c.options().dtype(at::kFloat));
  }
  dmp::launch_gemm((int)mode, (int)epi, (int)cfg, bf16(a), (int)lda, bf16(b), (int)ldb,
                   c.data_ptr(), (int)ldc, c2p, bf16_or_null(bias), auxp,
                   ptr_or_null<float>(dbias), (int)M, (int)N, (int)K,
                   (int)std::max<int64_t>(1, splits), cur_stream(), relu, partp,
                   ptr_or_null<float>(ws), amp);
}

std::vector<std::vector<int64_t>> gemm_configs() {
  return config_table(dmp::gemm_num_configs(), dmp::gemm_config_info, 5);
}

}  // namespace

void bind_gemm(pybind11::module_& m) {
  m.def("pad_rows_batched", &pad_rows_batched, "padded-row copies of im2col conv weights");
  m.def("colsum_acc", &colsum_acc, "bias gradient: out[n] += sum_m dy[m][n] (bf16 -> fp32)",
        py::arg("dy"), py::arg("out"), py::arg("slots") = py::none());
  m.def("colsum_num_slots", &dmp::colsum_num_slots, "slot rows of the colsum scratch");
  m.def("gemm", &gemm, "bf16 MFMA GEMM (fwd / dgrad / wgrad modes, fused epilogues)",
        py::arg("mode"), py::arg("epi"), py::arg("cfg"), py::arg("a"), py::arg("b"), py::arg("c"),
        py::arg("c2") = py::none(), py::arg("bias") = py::none(), py::arg("aux") = py::none(),
        py::arg("dbias") = py::none(), py::arg("splits") = 1, py::arg("relu") = false,
        py::arg("part") = py::none(), py::arg("slab") = false, py::arg("auxmask") = py::none());
  m.def("gemm_config_ok", &dmp::gemm_config_ok, "tile config usable in this mode");
  m.def("gemm_set_xcd_k", &dmp::gemm_set_xcd_k, "split-major XCD deal of wgrad split-K on/off");
  m.def("gemm_configs", &gemm_configs, "[(id, BM, BN, threads, stages, BK)] of the GEMM tiles");
}

}  // namespace dmp::bind
