// Stochastic depth (drop path, Huang et al. 2016 in its per-sample form) for
// the ViT residual branches.
//
// One draw launch per training forward fills the whole [branches][B] fp32
// scale table: S[j][b] = 1 / (1 - p_j) when sample b keeps branch j, 0 when it
// drops it.  The draw of (b, j) at step t is word b & 3 of
//   philox4x32_10(ctr = (b >> 2, j, t, "drop"), key = (seed_lo, seed_hi)),
// kept when the word >= thr[j] (dropout's threshold formula).  t is a
// device-side int64 the launch reads and advances, so a captured step draws a
// fresh table on every replay.  The table is consumed by the row-scaled
// add+LayerNorm kernels (transformer.hip); drop_path_rows_kernel scales a
// branch on the routes that do not go through the fused add.
#include "common.h"
#include "philox.h"

namespace dmp {

constexpr u32 kDropDomain = 0x64726F70u;   // "drop": counter word 3, as "data" is for data.hip

// ONE block: thread = one Philox call = four samples of one branch.  Every
// thread reads the counter before the barrier and thread 0 advances it after,
// so a single block needs no arrival ticket.
__global__ void __launch_bounds__(256) drop_path_draw_kernel(
    float* __restrict__ table, long long* __restrict__ state, const long long* __restrict__ thr,
    const float* __restrict__ scale, int branches, int B, unsigned long long seed) {
  const long long t = state[0];
  const uint2 key = make_uint2((u32)seed, (u32)(seed >> 32));
  const int groups = (B + 3) / 4;
  const int work = branches * groups;
  for (int w = threadIdx.x; w < work; w += blockDim.x) {
    const int j = w / groups, g = w - j * groups;
    const uint4 r = philox4x32_10(make_uint4((u32)g, (u32)j, (u32)t, kDropDomain), key);
    const u32 d[4] = {r.x, r.y, r.z, r.w};
    const u32 th = (u32)thr[j];
    const float sc = scale[j];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int b = g * 4 + k;
      if (b < B) table[(long long)j * B + b] = d[k] >= th ? sc : 0.f;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) state[0] = t + 1;
}

// y = bf16(x * s[sample]) over 16-byte vectors, `per` vectors per sample; the
// forward of a scaled branch and, on the gradient, its backward.
__global__ void __launch_bounds__(256) drop_path_rows_kernel(const u16* __restrict__ x,
                                                             const float* __restrict__ rscale,
                                                             u16* __restrict__ y, long long per,
                                                             long long nvec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += stride) {
    const float s = rscale[v / per];
    const bf16x8 a = reinterpret_cast<const bf16x8*>(x)[v];
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.v[k] = f2bf(bf2f(a.v[k]) * s);
    reinterpret_cast<bf16x8*>(y)[v] = o;
  }
}

void launch_drop_path_draw(float* table, long long* state, const long long* thr,
                           const float* scale, int branches, int B, unsigned long long seed,
                           hipStream_t s) {
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(1), dim3(256), 0, s, table, state, thr, scale,
                     branches, B, seed);
}

void launch_drop_path_rows(const u16* x, const float* rscale, u16* y, long long per,
                           long long nvec, hipStream_t s) {
  if (nvec <= 0) return;
  hipLaunchKernelGGL(drop_path_rows_kernel, dim3(stream_grid(nvec, 256)), dim3(256), 0, s, x,
                     rscale, y, per, nvec);
}

}  // namespace dmp
