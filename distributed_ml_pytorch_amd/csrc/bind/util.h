// Shared vocabulary of the Python bindings (csrc/bind/*.cpp).  Every op checks
// device, dtype, contiguity and alignment on the host before launching (a
// mis-shaped launch of a hand-written kernel must fail loudly here, never fault
// on the GPU), and launches on the caller's current HIP stream so ops compose
// with torch streams, events and hipGraph capture.
//
// The only header that includes torch, and the only place a bf16 pointer cast
// or an alignment test is written.  It lives under bind/ so that the kernel
// objects, which depend on csrc/*.h, do not rebuild when a helper changes.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "geom_guard.h"
#include "launchers.h"

namespace dmp::bind {

using at::Tensor;
using c10::optional;

constexpr auto kCL = at::MemoryFormat::ChannelsLast;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// an optional tensor that is present and defined (None arrives as nullopt)
inline bool has(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

inline bool aligned(const Tensor& t, uintptr_t bytes = 16) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0;
}

// ----------------------------------------------------------------- pointers
// bf16 storage as the kernels' uint16_t (converts to const uint16_t* for inputs)
inline uint16_t* bf16(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

inline uint16_t* bf16_or_null(const Tensor& t) { return t.defined() ? bf16(t) : nullptr; }

inline uint16_t* bf16_or_null(const optional<Tensor>& t) { return has(t) ? bf16(*t) : nullptr; }

template <typename T>
T* ptr_or_null(const Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

template <typename T>
T* ptr_or_null(const optional<Tensor>& t) {
  return has(t) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

// int64 storage as the kernels' long long
inline long long* i64(const Tensor& t) { return reinterpret_cast<long long*>(t.data_ptr()); }

// ------------------------------------------------------------------- checks
inline void check_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous() || t.is_contiguous(kCL), name,
              " must be dense (contiguous or channels_last)");
  TORCH_CHECK(aligned(t), name, " must be 16-byte aligned");
}

inline void check_flat(const Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
  check_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.numel() == n, name, " has ", t.numel(), " elements, expected ", n);
}

// per-channel / per-column vector (affine, running stats, bias, parameter
// gradients): contiguous, n elements, any shape
inline void check_vec(const Tensor& t, at::ScalarType dt, int64_t n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.numel() == n, what,
              " must be a contiguous ", dt, " GPU tensor of ", n, " elements");
}

// the optional ones among `ts` that are given
inline void check_vecs(std::initializer_list<const optional<Tensor>*> ts, at::ScalarType dt,
                       int64_t n, const char* what) {
  for (auto* t : ts)
    if (has(*t)) check_vec(**t, dt, n, what);
}

// channels-last activation (N, C, H, W logical) or an [M, C] matrix
inline void check_nhwc_bf16(const Tensor& x, const char* name) {
  check_gpu(x, name);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, name, " must be bf16");
  if (x.dim() == 4) {
    TORCH_CHECK(x.is_contiguous(kCL), name, " must be channels_last");
  } else {
    TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), name, " must be [M, C] contiguous");
  }
}

inline void check_rows_bf16(const Tensor& t, const char* name) {
  check_gpu(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.is_contiguous(), name,
              " must be a contiguous bf16 tensor");
}

// conv weight (bf16) or weight gradient (fp32): channels_last [CO, CI, R, S]
inline void check_weight_cl(const Tensor& w, at::ScalarType dt, const char* name) {
  check_gpu(w, name);
  TORCH_CHECK(w.scalar_type() == dt && w.dim() == 4 && w.is_contiguous(kCL), name,
              " must be a ", dt, " channels_last [CO, CI, R, S] tensor");
}

inline void same_shape(const Tensor& a, const Tensor& b, const char* what) {
  TORCH_CHECK(a.sizes() == b.sizes(), what, " shape mismatch: ", a.sizes(), " vs ", b.sizes());
}

// uint8 bit mask of `bits` flags, 8 per byte
inline const uint8_t* bit_mask_ptr(const Tensor& mask, int64_t bits, const char* what) {
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kByte && mask.is_contiguous() &&
                  mask.numel() == bits / 8,
              what, " must be a contiguous uint8 GPU bit mask of ", bits / 8, " bytes");
  return mask.data_ptr<uint8_t>();
}

// ---------------------------------------------------------------- BatchNorm
// BatchNorm slot sums [2][kBnSlots][C] (+ kBnTail): a persistent per-layer
// buffer (zeroed once, re-zeroed by every finalize) or a fresh zeroed one
inline Tensor bn_slots(const optional<Tensor>& slots, int64_t C, const at::TensorOptions& opt) {
  const int64_t n = 2 * dmp::kBnSlots * C + dmp::kBnTail;
  if (!has(slots)) return at::zeros({n}, opt.dtype(at::kFloat));
  TORCH_CHECK(slots->is_cuda() && slots->scalar_type() == at::kFloat && slots->is_contiguous() &&
                  slots->numel() == n,
              "BN slot buffer must be a contiguous fp32 GPU tensor of 2*", dmp::kBnSlots, "*C+",
              dmp::kBnTail, " elements");
  return *slots;
}

// the other direction's slots, zeroed by a folded apply for their next use
inline float* other_slots(const optional<Tensor>& zero_buf, int64_t C,
                          const at::TensorOptions& opt, const Tensor& part) {
  if (!has(zero_buf)) return nullptr;
  float* zb = bn_slots(zero_buf, C, opt).data_ptr<float>();
  TORCH_CHECK(zb != part.data_ptr<float>(),
              "bn fold: zero_buf must not alias the slots being reduced");
  return zb;
}

// 1-bit ReLU mask [M][C/8] of a BatchNorm forward (null: recomputed or no ReLU)
inline const uint8_t* relu_mask_ptr(const optional<Tensor>& mask, bool relu, int64_t M,
                                    int64_t C) {
  return relu && has(mask) ? bit_mask_ptr(*mask, M * C, "bn: ReLU mask [M, C/8]") : nullptr;
}

// ------------------------------------------------------------ config tables
// [(id, info[0], ..., info[width - 1])] of n compiled tile configs
template <typename F>
std::vector<std::vector<int64_t>> config_table(int n, F info_fn, int width) {
  std::vector<std::vector<int64_t>> out;
  for (int i = 0; i < n; ++i) {
    int info[8];
    info_fn(i, info);
    out.push_back({i});
    out.back().insert(out.back().end(), info, info + width);
  }
  return out;
}

// the ids base + [0, n) that `ok` accepts, appended to out
template <typename F>
void config_ids(std::vector<int64_t>& out, int base, int n, F ok) {
  for (int c = base; c < base + n; ++c)
    if (ok(c)) out.push_back(c);
}

}  // namespace dmp::bind
