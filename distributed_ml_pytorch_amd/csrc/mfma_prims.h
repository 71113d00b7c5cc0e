// MFMA / LDS-DMA primitives shared by the gfx950 tensor-core kernel files
// (conv.hip, conv_wgrad.hip, stem.hip, conv_small.hip, gemm.hip, attention.hip).
// Include after common.h.
#pragma once

#include "common.h"

namespace dmp {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_bf16: D[16][16] += A[16][32] * B[32][16]
__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                 __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// LDS DMA (buffer_load_dwordx4 ... lds, 16 B per lane into a lane-linear 1 KiB
// wave slice at m0) from inline asm on purpose: the compiler models the builtin
// as an LDS store it cannot tell from the ring slot being read, and puts
// s_waitcnt vmcnt(0) in front of the very next ds_read -- serialising every
// stage's DMA with the MFMA work.  Completion is tracked by hand (wait_vm),
// counted per wave.  32-bit byte offsets into a buffer descriptor; offsets >=
// its num_records (kOOB) read as zeros: that is how padding taps and rows past
// the end of an operand are fetched.
constexpr unsigned kOOB = 0x80000000u;
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, unsigned voff,
                                      u16* lds_wave_base) {
  const unsigned m0 = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds_wave_base;
  asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rs),
               "{m0}"(m0));
}

// wait until at most N of this wave's vector-memory ops are outstanding (and
// all of its LDS ops have completed)
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0070);
}

// vmcnt wait with a launch-time (wave-uniform) count in [1, MAXN]; any other
// count waits for everything (the cases above MAXN fall through to the default)
template <int MAXN>
__device__ __forceinline__ void wait_vm_n(int n) {
  static_assert(MAXN >= 1 && MAXN <= 40, "extend the case list");
  switch (n) {
#define DMP_WV(k)               \
  case k:                       \
    if constexpr (k <= MAXN) {  \
      wait_vm<k>();             \
      break;                    \
    }
    DMP_WV(1) DMP_WV(2) DMP_WV(3) DMP_WV(4) DMP_WV(5) DMP_WV(6) DMP_WV(7) DMP_WV(8) DMP_WV(9)
    DMP_WV(10) DMP_WV(11) DMP_WV(12) DMP_WV(13) DMP_WV(14) DMP_WV(15) DMP_WV(16) DMP_WV(17)
    DMP_WV(18) DMP_WV(19) DMP_WV(20) DMP_WV(21) DMP_WV(22) DMP_WV(23) DMP_WV(24) DMP_WV(25)
    DMP_WV(26) DMP_WV(27) DMP_WV(28) DMP_WV(29) DMP_WV(30) DMP_WV(31) DMP_WV(32) DMP_WV(33)
    DMP_WV(34) DMP_WV(35) DMP_WV(36) DMP_WV(37) DMP_WV(38) DMP_WV(39) DMP_WV(40)
#undef DMP_WV
    default:
      wait_vm<0>();
  }
}

// sum of v over the 16 lanes of each DPP row, valid in lane 15 of the row:
// four v_add_f32_dpp row_shr steps (bound_ctrl zero-fills lanes shifted in
// from outside the row) instead of four ds_bpermute round trips
__device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}

// Block-level flush of per-channel BatchNorm sums (sum, sum of squares) that
// every lane holds for its D^T fragments: lane l of a wave owns channels
// 4 * (l >> 4) .. + 3 of each 16-channel column tile j, for one row in 16.
// row_sum16 -> lane 15 of every DPP row writes red[wave row][BN] -> barrier ->
// one atomic pair per channel into slot rows `slot` and kBnSlots + slot of
// part [2][kBnSlots][CO].  WR wave rows (wave: row wrow, channels from ncol)
// cover the BN-channel block tile at n0; NT threads.  red: 2 * WR * BN floats
// of LDS that nobody reads or fills any more (the caller synchronised).
template <int WR, int BN, int NT, int TN>
__device__ __forceinline__ void slot_sum_flush(float (&s_sum)[TN][4], float (&s_sq)[TN][4],
                                               float* red, int wrow, int ncol, int tid, int lane,
                                               float* part, int n0, int CO, int slot) {
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s_sum[j][r] = row_sum16(s_sum[j][r]);
      s_sq[j][r] = row_sum16(s_sq[j][r]);
    }
  if ((lane & 15) == 15) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nl = ncol + j * 16 + 4 * (lane >> 4) + r;
        red[wrow * BN + nl] = s_sum[j][r];
        red[WR * BN + wrow * BN + nl] = s_sq[j][r];
      }
  }
  __syncthreads();
  for (int nl = tid; nl < BN; nl += NT) {
    const int n = n0 + nl;
    if (n < CO) {
      float ss = 0.f, qq = 0.f;
#pragma unroll
      for (int w = 0; w < WR; ++w) { ss += red[w * BN + nl]; qq += red[WR * BN + w * BN + nl]; }
      atomicAdd(part + (long long)slot * CO + n, ss);
      atomicAdd(part + (long long)(kBnSlots + slot) * CO + n, qq);
    }
  }
}

// [rows][R] bf16 image read transposed (R >= 128 = whole 256-B bank rows): 32-B
// granule u of row r holds logical granule u ^ tf(r).  One half-wave tr read
// touches rows {8g + q : g = 0,1, q = 0..3} of one granule column; tf gives
// those 8 rows 8 distinct granules of the bank row -> conflict-free.
__device__ __forceinline__ int tf(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }
template <int R>
__device__ __forceinline__ int toff(int row, int col) {
  return row * R + (((col >> 4) ^ tf(row)) << 4) + (col & 15);
}

}  // namespace dmp
