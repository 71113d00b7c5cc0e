// Depthwise K x K convolution (K in {3, 5, 7}), stride 1, "same" padding, NHWC
// bf16 with fp32 accumulation: the spatial mixing of ConvNeXt (Liu et al. 2022)
// and of the MobileNet / EfficientNet family.  groups == CI == CO == C, so there
// is no channel reduction and nothing for MFMA to do: VALU + LDS kernels.
//
// Forward and data gradient, dwconv_kernel<K>.  A workgroup owns a TH x TW output
// tile of one image and CC channels (dwconv_plan.h picks them per geometry).  It
// stages the (TH + K - 1) x (TW + K - 1) x CC input tile once, by 16-byte loads
// (positions outside the image or past C are written as zeros: a predicate on
// the load, no out-of-range address is ever formed), and the chunk's taps,
// transposed from the shadow's [C][K*K] bf16 to tap-major [K*K][CC] fp32.  The
// data gradient is the same kernel over dy with the taps mirrored at staging.
// A lane owns 8 channels (one 16-byte vector) and kDwRun = 4 consecutive outputs
// along W.  Per tap row it holds the row's K tap vectors in registers, reads the
// 4 + K - 1 window pixels from LDS and widens each once (a shift or a mask per
// value) for the up to K outputs that use it: K (4 + K - 1) / 4 window reads per
// output vector instead of K * K (17.5 instead of 49 at K = 7).  Taps are kept in fp32 so the
// inner loop has no conversion of them; lanes of equal channel vector read the
// same tap address (a broadcast).  The bf16 dot2 builtin was not kept: it pairs
// two CHANNELS' products into one sum, which a depthwise conv never adds, and
// pairing two TAPS instead needs a pixel-pair interleave of the staged image
// that costs more VALU than the fp32 FMAs it saves.  The file is built without
// the packed fp32 VALU forms (_build.py NO_PACKED_FP32): with them the compiler
// pairs the accumulators, and the forward kernels need 117 / 118 VGPRs at K = 5 /
// 7 and the K = 7 weight gradient 136, against the 84-95 below: a wave per SIMD
// less (4 instead of 5) in kernels that live on hiding LDS latency.
// LDS pitch: dw_pitch() pads a staged pixel and dw_row_pad() a staged row so that
// the 16 lanes one ds_read_b128 cycle serves touch distinct 16-byte granules of
// the 256-byte bank row.  Checked by enumerating every 16-lane group's addresses
// on the host (dw_read_ways(), dwconv_plan.h) over H, W in 1..64, K in {3, 5, 7}
// and twelve channel counts: see the counts quoted at dw_row_pad.
// Epilogue: + bias (forward), + the residual stream's own gradient (data
// gradient of a block whose input also feeds the layer-scale add), one bf16
// rounding, 16-byte stores.
//
// Weight and bias gradient, dwconv_wgrad_kernel<K>: one pass over x and dy.  A
// workgroup owns 32 channels and walks tiles of (image, TH x TW); per tile it
// stages dy and x with its halo.  Lane = (4-channel group, tap row r, row
// group): for its rows it slides along W with the K-pixel x window rotating
// through registers (the loop is unrolled K times) and accumulates K taps x 4
// channels in fp32; lanes of tap row 0 also sum dy for the bias.  After the
// last tile the row groups are added in LDS in a fixed order and the workgroup
// writes ONE [K*K + 1][32] partial into the layer's slab;
// dwconv_wgrad_reduce_kernel adds the partials in index order into the fp32
// arena gradients.  No atomics: bitwise reproducible, and every slab word that
// is read was written by the same launch (nothing to zero, graph-capturable).
//
// Registers (hipcc 7, -O3, gfx950; no scratch in any of them):
//   dwconv_kernel<3> 89, <5> 84, <7> 89 VGPRs (5 waves per SIMD);
//   dwconv_wgrad_kernel<3> 60, <5> 79, <7> 95 VGPRs.
#include <stdexcept>

#include "common.h"
#include "dwconv_plan.h"

namespace dmp {

__device__ __forceinline__ void widen8(const uint4 v, float (&f)[8]) {
  const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = __uint_as_float(w[k] << 16);
    f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
  }
}

// rows x cols pixels of image n from (h0, w0), CV 16-byte channel vectors from
// channel c0, into lds[row * rowpitch + col * pitch + cv * 16]; zeros outside
__device__ __forceinline__ void dw_stage(const u16* __restrict__ src, unsigned char* lds, int n,
                                         int h0, int w0, int rows, int cols, int c0, int cvshift,
                                         int rowpitch, int pitch, int H, int W, int C) {
  const int CV = 1 << cvshift, total = rows * cols << cvshift;
  for (int v = threadIdx.x; v < total; v += kDwThreads) {
    const int cv = v & (CV - 1), pix = v >> cvshift;
    const int row = pix / cols, col = pix - row * cols;
    const int ih = h0 + row, iw = w0 + col, c = c0 + cv * 8;
    uint4 val = make_uint4(0u, 0u, 0u, 0u);
    if (ih >= 0 && ih < H && iw >= 0 && iw < W && c < C)
      val = *reinterpret_cast<const uint4*>(src + (((long long)n * H + ih) * W + iw) * C + c);
    *reinterpret_cast<uint4*>(lds + row * rowpitch + col * pitch + cv * 16) = val;
  }
}

template <int K>
__global__ void __launch_bounds__(kDwThreads) dwconv_kernel(
    const u16* __restrict__ x, const u16* __restrict__ w, const float* __restrict__ bias,
    const u16* __restrict__ addend, u16* __restrict__ y, int H, int W, int C, int TH, int TW,
    int CC, int cvshift, int tiles_w, int pitch, int rowpitch, int flip) {
  constexpr int P = K / 2, WIN = kDwRun + K - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* taps = reinterpret_cast<float*>(smem);                  // [K*K][CC]
  unsigned char* img = smem + K * K * CC * 4;
  const int th0 = (blockIdx.x / tiles_w) * TH, tw0 = (blockIdx.x % tiles_w) * TW;
  const int c0 = blockIdx.y * CC, n = blockIdx.z;
  const int cols = TW + K - 1;

  for (int e = threadIdx.x; e < K * K * CC; e += kDwThreads) {
    const int c = e / (K * K), t = e - c * (K * K);              // coalesced over [c][t]
    const float v = c0 + c < C ? bf2f(w[(long long)(c0 + c) * (K * K) + t]) : 0.f;
    taps[(flip ? K * K - 1 - t : t) * CC + c] = v;
  }
  dw_stage(x, img, n, th0 - P, tw0 - P, TH + K - 1, cols, c0, cvshift, rowpitch, pitch, H, W, C);
  __syncthreads();

  const int CV = 1 << cvshift, runs = TW / kDwRun, items = (TH * runs) << cvshift;
  for (int item = threadIdx.x; item < items; item += kDwThreads) {
    const int cv = item & (CV - 1), t = item >> cvshift;
    const int row = t / runs, run = t - row * runs;
    const int oh = th0 + row, ow = tw0 + run * kDwRun, c = c0 + cv * 8;
    if (oh >= H || ow >= W || c >= C) continue;
    float acc[kDwRun][8];
#pragma unroll
    for (int o = 0; o < kDwRun; ++o)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[o][k] = 0.f;
    const unsigned char* base = img + row * rowpitch + run * kDwRun * pitch + cv * 16;
    const float* tp = taps + cv * 8;
    // one tap row at a time (not unrolled: the K rows' loads would all be hoisted
    // and spill): its K tap vectors stay in registers while the window pixels
    // stream through, each widened once and used by up to K of the 4 outputs
#pragma unroll 1
    for (int r = 0; r < K; ++r) {
      float wr[K][8];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(tp + (r * K + s) * CC);
        const float4 b = *reinterpret_cast<const float4*>(tp + (r * K + s) * CC + 4);
        wr[s][0] = a.x; wr[s][1] = a.y; wr[s][2] = a.z; wr[s][3] = a.w;
        wr[s][4] = b.x; wr[s][5] = b.y; wr[s][6] = b.z; wr[s][7] = b.w;
      }
      const unsigned char* rowp = base + r * rowpitch;
#pragma unroll
      for (int j = 0; j < WIN; ++j) {
        float px[8];
        widen8(*reinterpret_cast<const uint4*>(rowp + j * pitch), px);
#pragma unroll
        for (int s = 0; s < K; ++s) {
          const int o = j - s;
          if (o >= 0 && o < kDwRun) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[o][k] = __fmaf_rn(px[k], wr[s][k], acc[o][k]);
          }
        }
      }
    }
    float bv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bv[k] = bias ? bias[c + k] : 0.f;
#pragma unroll
    for (int o = 0; o < kDwRun; ++o) {
      if (ow + o >= W) break;
      const long long off = (((long long)n * H + oh) * W + ow + o) * C + c;
      float av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (addend) widen8(*reinterpret_cast<const uint4*>(addend + off), av);
      bf16x8 out;
#pragma unroll
      for (int k = 0; k < 8; ++k) out.v[k] = f2bf(acc[o][k] + bv[k] + av[k]);
      *reinterpret_cast<bf16x8*>(y + off) = out;
    }
  }
}

template <int K>
__global__ void __launch_bounds__(kDwThreads) dwconv_wgrad_kernel(
    const u16* __restrict__ dy, const u16* __restrict__ x, float* __restrict__ slab, int N, int H,
    int W, int C, int TH, int TW, int RG, int tiles_h, int tiles_w, int xrow, int dyrow) {
  constexpr int P = K / 2, CG = kDwWgChunk / kDwWgVec, PIX = kDwWgChunk * 2, T1 = K * K + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ximg = smem;
  unsigned char* dimg = smem + (TH + K - 1) * xrow;
  const int c0 = blockIdx.y * kDwWgChunk;
  const int cg = threadIdx.x % CG, r = (threadIdx.x / CG) % K, rg = threadIdx.x / (CG * K);
  const bool active = rg < RG;
  float acc[K][kDwWgVec], bsum[kDwWgVec];
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int k = 0; k < kDwWgVec; ++k) acc[s][k] = 0.f;
#pragma unroll
  for (int k = 0; k < kDwWgVec; ++k) bsum[k] = 0.f;

  const long long tiles = (long long)N * tiles_h * tiles_w;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int n = (int)(tile / (tiles_h * tiles_w)), tt = (int)(tile - (long long)n * tiles_h * tiles_w);
    const int th0 = (tt / tiles_w) * TH, tw0 = (tt % tiles_w) * TW;
    __syncthreads();                       // the previous tile's readers are done
    dw_stage(x, ximg, n, th0 - P, tw0 - P, TH + K - 1, TW + K - 1, c0, 2, xrow, PIX, H, W, C);
    dw_stage(dy, dimg, n, th0, tw0, TH, TW, c0, 2, dyrow, PIX, H, W, C);
    __syncthreads();
    if (!active) continue;
    for (int h = rg; h < TH; h += RG) {
      const unsigned char* xr = ximg + (h + r) * xrow + cg * 8;
      const unsigned char* dr = dimg + h * dyrow + cg * 8;
      float win[K][kDwWgVec];              // slot (w + s) % K holds x[w + s]
      auto load4 = [](const unsigned char* p, float (&f)[kDwWgVec]) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        f[0] = __uint_as_float(v.x << 16);
        f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16);
        f[3] = __uint_as_float(v.y & 0xffff0000u);
      };
#pragma unroll
      for (int s = 0; s < K - 1; ++s) load4(xr + s * PIX, win[s]);
      for (int wb = 0; wb < TW; wb += K) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          load4(xr + (wb + j + K - 1) * PIX, win[(j + K - 1) % K]);
          float d[kDwWgVec];
          load4(dr + (wb + j) * PIX, d);
#pragma unroll
          for (int s = 0; s < K; ++s)
#pragma unroll
            for (int k = 0; k < kDwWgVec; ++k)
              acc[s][k] = __fmaf_rn(d[k], win[(j + s) % K][k], acc[s][k]);
          if (r == 0) {
#pragma unroll
            for (int k = 0; k < kDwWgVec; ++k) bsum[k] += d[k];
          }
        }
      }
    }
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);                   // [RG][K*K + 1][32]
  if (active) {
    float* mine = red + (rg * T1) * kDwWgChunk + cg * kDwWgVec;
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int k = 0; k < kDwWgVec; ++k) mine[(r * K + s) * kDwWgChunk + k] = acc[s][k];
    if (r == 0) {
#pragma unroll
      for (int k = 0; k < kDwWgVec; ++k) mine[K * K * kDwWgChunk + k] = bsum[k];
    }
  }
  __syncthreads();
  float* out = slab + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (T1 * kDwWgChunk);
  for (int e = threadIdx.x; e < T1 * kDwWgChunk; e += kDwThreads) {
    float v = 0.f;
    for (int g = 0; g < RG; ++g) v += red[g * T1 * kDwWgChunk + e];
    out[e] = v;
  }
}

// dw[c][t] += sum_part slab[chunk][part][t][c % 32], db[c] += ... [K*K]: parts in order
__global__ void __launch_bounds__(256) dwconv_wgrad_reduce_kernel(
    const float* __restrict__ slab, float* __restrict__ dw, float* __restrict__ db, int C, int KK,
    int parts) {
  const int e = blockIdx.x * 256 + threadIdx.x;                  // over [C][KK + 1]
  if (e >= C * (KK + 1)) return;
  const int c = e / (KK + 1), t = e - c * (KK + 1);
  const float* p = slab + ((long long)(c / kDwWgChunk) * parts * (KK + 1) + t) * kDwWgChunk +
                   c % kDwWgChunk;
  float v = 0.f;
  for (int g = 0; g < parts; ++g) v += p[(long long)g * (KK + 1) * kDwWgChunk];
  if (t < KK) dw[(long long)c * KK + t] += v;
  else if (db) db[c] += v;
}

template <int K>
static void dwconv_launch(const u16* x, const u16* w, const float* bias, const u16* addend, u16* y,
                          int N, int H, int W, int C, bool flip, const DwPlan& p, hipStream_t s) {
  int cvshift = 0;
  while ((kDwVec << cvshift) < p.CC) ++cvshift;
  hipLaunchKernelGGL((dwconv_kernel<K>), dim3(p.tiles_h * p.tiles_w, p.chunks, N),
                     dim3(kDwThreads), p.lds_bytes, s, x, w, bias, addend, y, H, W, C, p.TH, p.TW,
                     p.CC, cvshift, p.tiles_w, p.pitch, p.rowpitch, flip ? 1 : 0);
}

// y = dwconv(x, w) (+ bias) (+ addend); flip: taps mirrored (the data gradient).
// w: bf16 [C][K*K].  Geometry checked by the caller (guard::dwconv_ok).
void launch_dwconv(const u16* x, const u16* w, const float* bias, const u16* addend, u16* y, int N,
                   int H, int W, int C, int K, bool flip, hipStream_t s) {
  const DwPlan p = plan_dwconv(H, W, C, K);
  if (!p.ok) throw std::runtime_error("dwconv: no plan for this geometry");
  if (K == 3) dwconv_launch<3>(x, w, bias, addend, y, N, H, W, C, flip, p, s);
  else if (K == 5) dwconv_launch<5>(x, w, bias, addend, y, N, H, W, C, flip, p, s);
  else dwconv_launch<7>(x, w, bias, addend, y, N, H, W, C, flip, p, s);
}

template <int K>
static void dwconv_wgrad_launch(const u16* dy, const u16* x, float* slab, int N, int H, int W,
                                int C, const DwWgPlan& p, hipStream_t s) {
  hipLaunchKernelGGL((dwconv_wgrad_kernel<K>), dim3(p.parts, p.chunks), dim3(kDwThreads),
                     p.lds_bytes, s, dy, x, slab, N, H, W, C, p.TH, p.TW, p.row_groups, p.tiles_h,
                     p.tiles_w, p.xrow, p.dyrow);
}

// dw [C][K*K] += the weight gradient, db [C] += colsum(dy) (null: skipped); slab:
// dwconv_slab_floats(C, K) fp32 words, of which this launch overwrites and reads
// the first p.parts partials of every chunk
void launch_dwconv_wgrad(const u16* dy, const u16* x, float* dw, float* db, float* slab, int N,
                         int H, int W, int C, int K, hipStream_t s) {
  const DwWgPlan p = plan_dwconv_wgrad(N, H, W, C, K);
  if (!p.ok) throw std::runtime_error("dwconv wgrad: no plan for this geometry");
  if (K == 3) dwconv_wgrad_launch<3>(dy, x, slab, N, H, W, C, p, s);
  else if (K == 5) dwconv_wgrad_launch<5>(dy, x, slab, N, H, W, C, p, s);
  else dwconv_wgrad_launch<7>(dy, x, slab, N, H, W, C, p, s);
  const int total = C * (K * K + 1);
  hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s, slab,
                     dw, db, C, K * K, p.parts);
}

}  // namespace dmp
