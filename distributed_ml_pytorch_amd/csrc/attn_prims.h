// Device helpers shared by the fused attention kernels (attention.hip: resident
// route, attention_stream.hip: streaming route): the row-major [token][kRS] LDS
// image, its transposed fragment read and the packed bf16 stores.
#pragma once

#include "attn_plan.h"
#include "common.h"
#include "mfma_prims.h"

namespace dmp {
namespace {

constexpr int kDH = kAttnHeadDim;     // head dim
constexpr int kRS = kAttnRowStride;   // row stride (elements) of row-major [token][64] LDS tiles

__device__ __forceinline__ bf16x8 pack8(const f32x4& lo, const f32x4& hi) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r.v[i] = f2bf(lo[i]);
    r.v[4 + i] = f2bf(hi[i]);
  }
  return r;
}

__device__ __forceinline__ bf16x8 ld16(const u16* p) { return *reinterpret_cast<const bf16x8*>(p); }

__device__ __forceinline__ void st4(u16* p, const f32x4& v, float s) {
  uint2 w;
  w.x = (u32)f2bf(v[0] * s) | ((u32)f2bf(v[1] * s) << 16);
  w.y = (u32)f2bf(v[2] * s) | ((u32)f2bf(v[3] * s) << 16);
  *reinterpret_cast<uint2*>(p) = w;
}

// k-permuted operand read TRANSPOSED out of a row-major [token][kRS] image with
// ds_read_b64_tr_b16: lane 16g + 4q + p addresses token row0 + 4g + q (and
// row0 + 16 + 4g + q), head dims col0 + 4p .. col0 + 4p + 3; lane 16g + i gets
// head dim col0 + i of those 4 tokens, i.e. A[i][k] for k = {4g..4g+3,
// 16+4g..16+4g+3}.  The gather crosses lanes, so EXEC must be full: every call
// site sits in wave-uniform control flow.
__device__ __forceinline__ bf16x8 ld_tr_perm(const u16* img, int row0, int col0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const u16* a = img + (row0 + 4 * g + q) * kRS + col0 + 4 * p;
  const s16x4_t lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(a + 16 * kRS));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <typename K>
void allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace
}  // namespace dmp
