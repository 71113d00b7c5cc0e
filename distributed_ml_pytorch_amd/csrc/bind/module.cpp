// The _native extension module: one bind_<family>() per csrc/bind/<family>.cpp,
// mirroring the .hip files.  A new op goes into its family's file.
#include <pybind11/pybind11.h>

namespace dmp::bind {
void bind_optim(pybind11::module_& m);
void bind_norm_pool(pybind11::module_& m);
void bind_conv(pybind11::module_& m);
void bind_gemm(pybind11::module_& m);
void bind_transformer(pybind11::module_& m);
void bind_data(pybind11::module_& m);
}  // namespace dmp::bind

PYBIND11_MODULE(_native, m) {
  m.doc() = "gfx950 (MI355X) HIP kernels for distributed_ml_pytorch_amd";
  dmp::bind::bind_optim(m);
  dmp::bind::bind_norm_pool(m);
  dmp::bind::bind_conv(m);
  dmp::bind::bind_gemm(m);
  dmp::bind::bind_transformer(m);
  dmp::bind::bind_data(m);
  m.attr("arch") = "gfx950";
}
