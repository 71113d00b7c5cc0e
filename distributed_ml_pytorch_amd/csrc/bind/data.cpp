// data.hip: the batch assembler of the device-resident datasets.
#include "util.h"

namespace dmp::bind {
namespace {

// the first `count` rows of out_x as dense NHWC bf16 (a slice of a larger
// channels_last buffer qualifies; an NCHW-contiguous tensor does not)
void check_out_x(const Tensor& x, int64_t count, int64_t C, int64_t H, int64_t W) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "batch_assemble: out_x must be a bf16 GPU tensor, got ", x.scalar_type());
  TORCH_CHECK(x.dim() == 4 && x.size(0) >= count && x.size(1) == C && x.size(2) == H &&
                  x.size(3) == W,
              "batch_assemble: out_x must be [>= ", count, ", ", C, ", ", H, ", ", W, "], got ",
              x.sizes());
  const bool rows = x.size(0) <= 1 || x.stride(0) == H * W * C;
  const bool nhwc = (C == 1 || x.stride(1) == 1) && (H == 1 || x.stride(2) == W * C) &&
                    (W == 1 || x.stride(3) == C);
  TORCH_CHECK(rows && nhwc, "batch_assemble: out_x must be channels_last (dense NHWC rows), got "
              "strides ", x.strides());
  TORCH_CHECK(aligned(x, 2), "batch_assemble: out_x must be 2-byte aligned");
}

// the tensor and range checks both forms of the assembler share
void check_assemble(const Tensor& data, const Tensor& labels, const Tensor& lut,
                    const Tensor& index, int64_t count, const Tensor& out_x, const Tensor& out_y,
                    const optional<Tensor>& draws, int64_t pad, int64_t epoch, int64_t path) {
  TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kByte && data.dim() == 4 &&
                  data.is_contiguous(),
              "batch_assemble: data must be a contiguous uint8 [N, H, W, C] GPU tensor");
  const int64_t N = data.size(0), H = data.size(1), W = data.size(2), C = data.size(3);
  TORCH_CHECK(dmp::guard::dataset_ok(N, H, W, C),
              "batch_assemble: a dataset needs 1..", dmp::guard::kDatasetMaxChannels,
              " channels and N*H*W*C < 2 GiB, got ", data.sizes());
  TORCH_CHECK(pad >= 0 && pad <= dmp::guard::kDatasetMaxPad, "batch_assemble: 0 <= pad <= ",
              dmp::guard::kDatasetMaxPad, ", got ", pad);
  TORCH_CHECK(count >= 0 && dmp::guard::assemble_ok(count, H, W, C, pad),
              "batch_assemble: a batch of ", count, " images is out of range");
  TORCH_CHECK(epoch >= 0 && epoch <= 0xffffffffLL, "batch_assemble: epoch out of range");
  TORCH_CHECK(path == -1 || path == 0, "batch_assemble: path is -1 (automatic) or 0 (direct)");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.is_contiguous() &&
                  labels.numel() == N,
              "batch_assemble: labels must be a contiguous int64 GPU tensor of ", N, " elements");
  TORCH_CHECK(lut.is_cuda() && lut.scalar_type() == at::kBFloat16 && lut.is_contiguous() &&
                  lut.dim() == 2 && lut.size(0) == C && lut.size(1) == 256,
              "batch_assemble: lut must be a contiguous bf16 [", C, ", 256] GPU tensor");
  TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kInt && index.is_contiguous() &&
                  index.numel() >= count,
              "batch_assemble: index must be a contiguous int32 GPU tensor of >= ", count,
              " elements");
  check_out_x(out_x, count, C, H, W);
  TORCH_CHECK(out_y.is_cuda() && out_y.scalar_type() == at::kLong && out_y.is_contiguous() &&
                  out_y.numel() >= count,
              "batch_assemble: out_y must be a contiguous int64 GPU tensor of >= ", count,
              " elements");
  if (has(draws))
    TORCH_CHECK(draws->is_cuda() && draws->scalar_type() == at::kChar && draws->is_contiguous() &&
                    draws->numel() >= 3 * count,
                "batch_assemble: draws must be a contiguous int8 [>= ", count, ", 3] GPU tensor");
  for (const Tensor* t : {&labels, &lut, &index, &out_x, &out_y})
    TORCH_CHECK(t->device() == data.device(), "batch_assemble: every tensor must be on ",
                data.device(), ", got one on ", t->device());
  TORCH_CHECK(!has(draws) || draws->device() == data.device(),
              "batch_assemble: draws must be on ", data.device());
}

void batch_assemble(Tensor data, Tensor labels, Tensor lut, Tensor index, int64_t count,
                    Tensor out_x, Tensor out_y, optional<Tensor> draws, int64_t pad, bool flip,
                    uint64_t seed, int64_t epoch, int64_t path) {
  check_assemble(data, labels, lut, index, count, out_x, out_y, draws, pad, epoch, path);
  const int64_t N = data.size(0), H = data.size(1), W = data.size(2), C = data.size(3);
  dmp::launch_batch_assemble(data.data_ptr<uint8_t>(), i64(labels), bf16(lut),
                             index.data_ptr<int>(), (int)count, (int)N, (int)H, (int)W, (int)C,
                             bf16(out_x), i64(out_y), ptr_or_null<signed char>(draws), (int)pad,
                             flip, (unsigned long long)seed, (uint32_t)epoch, (int)path,
                             cur_stream());
}

// Mixup / CutMix form: row b blended with row count - 1 - b (data.hip)
void batch_assemble_mix(Tensor data, Tensor labels, Tensor lut, Tensor index, int64_t count,
                        Tensor out_x, Tensor out_y, Tensor out_y2, Tensor out_lam,
                        optional<Tensor> draws, int64_t pad, bool flip, uint64_t seed,
                        int64_t epoch, double pix_lam, double label_lam, int64_t y0, int64_t y1,
                        int64_t x0, int64_t x1, int64_t path) {
  check_assemble(data, labels, lut, index, count, out_x, out_y, draws, pad, epoch, path);
  const int64_t N = data.size(0), H = data.size(1), W = data.size(2), C = data.size(3);
  TORCH_CHECK(out_y2.is_cuda() && out_y2.scalar_type() == at::kLong && out_y2.is_contiguous() &&
                  out_y2.numel() >= count && out_y2.device() == data.device(),
              "batch_assemble_mix: out_y2 must be a contiguous int64 tensor of >= ", count,
              " elements on ", data.device());
  TORCH_CHECK(out_lam.is_cuda() && out_lam.scalar_type() == at::kFloat &&
                  out_lam.is_contiguous() && out_lam.numel() >= count &&
                  out_lam.device() == data.device(),
              "batch_assemble_mix: out_lam must be a contiguous float32 tensor of >= ", count,
              " elements on ", data.device());
  TORCH_CHECK(dmp::guard::mix_ok(H, W, y0, y1, x0, x1, pix_lam, label_lam),
              "batch_assemble_mix: the box must satisfy 0 <= y0 <= y1 <= ", H,
              " and 0 <= x0 <= x1 <= ", W, " and pix_lam, label_lam must lie in [0, 1]; got box (",
              y0, ", ", y1, ", ", x0, ", ", x1, "), pix_lam ", pix_lam, ", label_lam ", label_lam);
  dmp::launch_batch_assemble_mix(data.data_ptr<uint8_t>(), i64(labels), bf16(lut),
                                 index.data_ptr<int>(), (int)count, (int)N, (int)H, (int)W, (int)C,
                                 bf16(out_x), i64(out_y), i64(out_y2), out_lam.data_ptr<float>(),
                                 ptr_or_null<signed char>(draws), (int)pad, flip,
                                 (unsigned long long)seed, (uint32_t)epoch, (float)pix_lam,
                                 (float)label_lam, (int)y0, (int)y1, (int)x0, (int)x1, (int)path,
                                 cur_stream());
}

bool batch_assemble_is_staged(Tensor data) {
  TORCH_CHECK(data.dim() == 4, "data must be [N, H, W, C]");
  return dmp::batch_assemble_staged(data.data_ptr(), (int)data.size(1), (int)data.size(2),
                                    (int)data.size(3));
}

}  // namespace

void bind_data(pybind11::module_& m) {
  m.def("batch_assemble", &batch_assemble,
        "gather + crop/flip + normalise a batch of a device-resident uint8 dataset",
        py::arg("data_u8"), py::arg("labels"), py::arg("lut"), py::arg("index_i32"),
        py::arg("count"), py::arg("out_x"), py::arg("out_y"), py::arg("draws"), py::arg("pad"),
        py::arg("flip"), py::arg("seed"), py::arg("epoch"), py::arg("path") = -1);
  m.def("batch_assemble_mix", &batch_assemble_mix,
        "batch_assemble with Mixup / CutMix of row b and row count - 1 - b; also writes the "
        "partner's labels and the label weight",
        py::arg("data_u8"), py::arg("labels"), py::arg("lut"), py::arg("index_i32"),
        py::arg("count"), py::arg("out_x"), py::arg("out_y"), py::arg("out_y2"),
        py::arg("out_lam"), py::arg("draws"), py::arg("pad"), py::arg("flip"), py::arg("seed"),
        py::arg("epoch"), py::arg("pix_lam"), py::arg("label_lam"), py::arg("y0"), py::arg("y1"),
        py::arg("x0"), py::arg("x1"), py::arg("path") = -1);
  m.def("batch_assemble_is_staged", &batch_assemble_is_staged,
        "whether batch_assemble stages this dataset's images through LDS");
}

}  // namespace dmp::bind
