// Layer-scale residual add, the closing op of a ConvNeXt block (and of CaiT /
// DeiT-III blocks): h = x + gamma[c] * r, optionally times the per-sample
// stochastic-depth scale s of the drop-path table (drop_path.hip).
//
// Rounding is pinned, contraction off:
//   t = fl32(gamma * r); t = fl32(t * s) when scaled; h = bf16_rne(fl32(x + t))
// so (x.float() + (gamma * r.float()) * s).to(bf16) in torch is the kernel bit
// for bit.  A sample with s == 0 copies x and does not read r.
// Backward: dr = bf16(fl32(fl32(dh * gamma) * s)); dgamma[c] = sum dh r s in fp32;
// dx is dh itself (no kernel).
//
// Layout, both kernels: thread = (row group, 16-byte channel vector); a
// workgroup reads RG = 256 / (C / 8) consecutive rows at a time (one contiguous
// span) and strides over the rows by grid.  A thread's channels never change, so
// gamma sits in 8 registers and the backward keeps 8 fp32 dgamma sums; the row
// groups are added in LDS in index order, each workgroup overwrites its own slot
// row, and layer_scale_dgamma_kernel adds the slot rows in index order into the
// arena gradient: no atomics, bitwise reproducible, nothing to zero.
#include "common.h"

namespace dmp {

constexpr int kLsSlots = 512;              // most workgroups of the backward = slot rows
constexpr int kLsMaxC = 2048;              // C / 8 channel vectors fit one workgroup

int layer_scale_max_channels() { return kLsMaxC; }
int layer_scale_num_slots() { return kLsSlots; }

__device__ __forceinline__ void ls_widen(const bf16x8& v, float (&f)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = bf2f(v.v[k]);
}

template <bool SCALED>
__global__ void __launch_bounds__(256) layer_scale_fwd_kernel(
    const u16* __restrict__ x, const u16* __restrict__ r, const float* __restrict__ gamma,
    const float* __restrict__ rscale, u16* __restrict__ h, long long rows, int CV, int tokens) {
#pragma clang fp contract(off)
  const int RG = 256 / CV, col = threadIdx.x % CV, rg = threadIdx.x / CV;
  if (rg >= RG) return;
  float g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = gamma[col * 8 + k];
  for (long long row = (long long)blockIdx.x * RG + rg; row < rows;
       row += (long long)gridDim.x * RG) {
    const long long v = row * CV + col;
    const bf16x8 xv = reinterpret_cast<const bf16x8*>(x)[v];
    float s = 1.f;
    if constexpr (SCALED) {
      s = rscale[row / tokens];
      if (s == 0.f) {
        reinterpret_cast<bf16x8*>(h)[v] = xv;
        continue;
      }
    }
    float xf[8], rf[8];
    ls_widen(xv, xf);
    ls_widen(reinterpret_cast<const bf16x8*>(r)[v], rf);
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = g[k] * rf[k];
      if constexpr (SCALED) t = t * s;
      o.v[k] = f2bf(xf[k] + t);
    }
    reinterpret_cast<bf16x8*>(h)[v] = o;
  }
}

template <bool SCALED>
__global__ void __launch_bounds__(256) layer_scale_bwd_kernel(
    const u16* __restrict__ dh, const u16* __restrict__ r, const float* __restrict__ gamma,
    const float* __restrict__ rscale, u16* __restrict__ dr, float* __restrict__ slots,
    long long rows, int CV, int tokens) {
#pragma clang fp contract(off)
  __shared__ float red[256 * 8];             // [RG][C]
  const int RG = 256 / CV, col = threadIdx.x % CV, rg = threadIdx.x / CV, C = CV * 8;
  float g[8], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    g[k] = rg < RG ? gamma[col * 8 + k] : 0.f;
    acc[k] = 0.f;
  }
  if (rg < RG) {
    for (long long row = (long long)blockIdx.x * RG + rg; row < rows;
         row += (long long)gridDim.x * RG) {
      const long long v = row * CV + col;
      float df[8];
      ls_widen(reinterpret_cast<const bf16x8*>(dh)[v], df);
      float s = 1.f;
      if constexpr (SCALED) s = rscale[row / tokens];
      if (dr) {
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float t = df[k] * g[k];
          if constexpr (SCALED) t = t * s;
          o.v[k] = f2bf(t);
        }
        reinterpret_cast<bf16x8*>(dr)[v] = o;
      }
      if (slots && s != 0.f) {
        float rf[8];
        ls_widen(reinterpret_cast<const bf16x8*>(r)[v], rf);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float t = df[k] * rf[k];
          if constexpr (SCALED) t = t * s;
          acc[k] += t;
        }
      }
    }
  }
  if (slots == nullptr) return;
  if (rg < RG) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[rg * C + col * 8 + k] = acc[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < C; e += 256) {
    float v = 0.f;
    for (int q = 0; q < RG; ++q) v += red[q * C + e];
    slots[(long long)blockIdx.x * C + e] = v;
  }
}

// dgamma[c] += sum over the `n` slot rows, in index order
__global__ void __launch_bounds__(256) layer_scale_dgamma_kernel(const float* __restrict__ slots,
                                                                 float* __restrict__ dgamma, int C,
                                                                 int n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float v = 0.f;
  for (int q = 0; q < n; ++q) v += slots[(long long)q * C + c];
  dgamma[c] += v;
}

static int ls_grid(long long rows, int CV, int cap) {
  const int RG = 256 / CV;
  const long long g = (rows + RG - 1) / RG;
  return (int)(g < cap ? (g < 1 ? 1 : g) : cap);
}

void launch_layer_scale_fwd(const u16* x, const u16* r, const float* gamma, const float* rscale,
                            u16* h, long long rows, int C, int tokens, hipStream_t s) {
  if (rows <= 0) return;
  const int CV = C / 8;
  const dim3 grid(ls_grid(rows, CV, 2048));
  if (rscale)
    hipLaunchKernelGGL((layer_scale_fwd_kernel<true>), grid, dim3(256), 0, s, x, r, gamma, rscale,
                       h, rows, CV, tokens);
  else
    hipLaunchKernelGGL((layer_scale_fwd_kernel<false>), grid, dim3(256), 0, s, x, r, gamma, rscale,
                       h, rows, CV, tokens);
}

void launch_layer_scale_bwd(const u16* dh, const u16* r, const float* gamma, const float* rscale,
                            u16* dr, float* dgamma, float* slots, long long rows, int C, int tokens,
                            hipStream_t s) {
  if (rows <= 0) return;
  const int CV = C / 8;
  const int nblk = ls_grid(rows, CV, kLsSlots);
  float* sl = dgamma ? slots : nullptr;
  if (rscale)
    hipLaunchKernelGGL((layer_scale_bwd_kernel<true>), dim3(nblk), dim3(256), 0, s, dh, r, gamma,
                       rscale, dr, sl, rows, CV, tokens);
  else
    hipLaunchKernelGGL((layer_scale_bwd_kernel<false>), dim3(nblk), dim3(256), 0, s, dh, r, gamma,
                       rscale, dr, sl, rows, CV, tokens);
  if (sl)
    hipLaunchKernelGGL(layer_scale_dgamma_kernel, dim3((C + 255) / 256), dim3(256), 0, s, sl,
                       dgamma, C, nblk);
}

}  // namespace dmp
