// Few-input-channel convolutions (network stems: CIFAR ResNet 3x3x3, ImageNet
// ResNet 7x7x3, AlexNet 11x11x3) on gfx950.
//
// K = R*S*CI is tiny (27 .. 363), so the implicit GEMM has nothing to feed the
// matrix cores with and MIOpen spends its time in layout shuffles and
// zero-fills around a K=27 GEMM.  These are VALU kernels shaped so that most
// per-FMA operand traffic is an LDS broadcast:
//
//   forward  lane = 4 consecutive output pixels, wave = 16 of the 64 output
//            channels of the tile (64 fp32 accumulators per lane).  The weight
//            tile [K][64] sits in LDS as fp32; all lanes of a wave read the same
//            row (broadcast ds_read_b128), so 4 LDS reads feed 64 FMAs.  Patch
//            taps are gathered 8 at a time through an LDS tap table (no integer
//            division in the loop).  Epilogue: bf16 NHWC store + per-channel BN
//            partial sums (recursive-halving butterfly over the lanes, lane l
//            ends up owning channel l & 15), added into the same
//            [2][kBnSlots][CO] slot sums as the implicit-GEMM epilogue.
//   wgrad    dW[co][k] = sum_p dY[p][co] * patch_p[k]: a block owns a chunk of
//            P, a 64-channel x 32-tap output tile; 64-pixel slabs of dY and of
//            the patches are staged to LDS as fp32, each lane accumulates a 4 x 8
//            outer product per pixel, the 4 waves split the slab rows and are
//            summed through LDS, then fp32 atomics into the arena gradient.
// The input image is read with explicit element strides (any dense layout of
// the bf16 activations).
#include <cstdlib>

#include "common.h"
#include "mfma_prims.h"

namespace dmp {

struct SmallConvArgs {
  const u16* x;     // input, element strides below (bf16)
  const u16* w;     // [CO][R][S][CI] bf16
  const u16* dy;    // [P][CO] bf16 (wgrad)
  u16* y;           // [P][CO] bf16 (forward)
  float* part;      // [2][kBnSlots][CO] BN slot sums (forward, optional, accumulated)
  float* dw;        // [CO][R][S][CI] fp32 (wgrad, accumulated)
  float* ws;        // wgrad: [G][CO][K] per-block partial tiles
  int sb, sh, sw, sc;           // input strides in elements (input < 2^30 elements)
  int xbytes;                   // input extent in bytes (buffer descriptor bound)
  int B, H, W, CI, OH, OW, CO, R, S, stride, pad, K;
  long long P;
  int chunk;        // wgrad: pixels per block
};

// tap table entry: r | s << 8 | ci << 16 (k >= K -> -1)
__device__ __forceinline__ int tap_of(const SmallConvArgs& a, int k) {
  if (k >= a.K) return -1;
  const int ci = k % a.CI, rs = k / a.CI;
  return (rs / a.S) | ((rs % a.S) << 8) | (ci << 16);
}

// raw buffer descriptor over the input image (gfx9 dword3); a load whose
// offset is past num_records returns 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const SmallConvArgs& a) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
}

// boff = b * sb (element offset of the image).  Padding / masked taps get an
// out-of-range offset and read 0 from the buffer unit: no branch per tap, so a
// thread's gathers issue back to back and retire under one wait.
__device__ __forceinline__ float load_tap(const SmallConvArgs& a, __amdgpu_buffer_rsrc_t rs,
                                          int tap, int boff, int ih0, int iw0) {
  const int ih = ih0 + (tap & 255), iw = iw0 + ((tap >> 8) & 255), ci = tap >> 16;
  const bool ok = tap >= 0 && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
  const int off = ok ? 2 * (boff + ih * a.sh + iw * a.sw + ci * a.sc) : 0x7ffffff0;
  return bf2f(__builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
}

// output pixel p (< 2^31) -> {b * sb, oh * stride - pad, ow * stride - pad}
__device__ __forceinline__ int3 decode_pixel(const SmallConvArgs& a, int p) {
  const int ow = p % a.OW, t = p / a.OW;
  const int oh = t % a.OH, b = t / a.OH;
  return make_int3(b * a.sb, oh * a.stride - a.pad, ow * a.stride - a.pad);
}

// v[0..2H) -> v[0..H): lanes with bit H set keep the upper half
template <int H>
__device__ __forceinline__ void halve(float* v, int lane) {
  const bool up = lane & H;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float send = up ? v[i] : v[i + H];
    const float keep = up ? v[i + H] : v[i];
    v[i] = keep + __shfl_xor(send, H, 64);
  }
}
// forward: lane = 4 consecutive output pixels, wave = 16 output channels of the
// 64-channel tile -> each broadcast weight read (4 x ds_read_b128) feeds 64 FMAs
constexpr int kOutPitch = 72;   // bf16 per staged output row (144 B: 16-B aligned, odd x 16 B)
__global__ void __launch_bounds__(256) conv_small_fwd_kernel(SmallConvArgs a) {
  constexpr int TC = 8;                          // taps gathered per pass
  extern __shared__ float smem[];
  float* wl = smem;                              // [K][64] fp32
  const int K = a.K, Kp = (K + TC - 1) / TC * TC;
  int* taps = reinterpret_cast<int*>(smem + K * 64);   // [Kp]
  u16* ot = reinterpret_cast<u16*>(smem + ((K * 64 + Kp + 3) & ~3));   // [256][kOutPitch]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int co0 = blockIdx.y * 64;
  for (int i = tid; i < K * 64; i += 256) {
    const int k = i >> 6, c = i & 63;
    wl[i] = bf2f(a.w[(long long)(co0 + c) * K + k]);
  }
  for (int k = tid; k < Kp; k += 256) taps[k] = tap_of(a, k);
  __syncthreads();

  const int pbase = blockIdx.x * 256 + lane * 4;
  int pb[4], ph[4], pw[4];
  bool pv_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pv_ok[i] = pbase + i < a.P;
    const int3 d = decode_pixel(a, pv_ok[i] ? pbase + i : 0);
    pb[i] = d.x;
    ph[i] = d.y;
    pw[i] = d.z;
  }
  float acc[4][16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[i][c] = 0.f;
  const float* wcol = wl + wid * 16;
  const __amdgpu_buffer_rsrc_t rs = image_rsrc(a);
  for (int k0 = 0; k0 < K; k0 += TC) {
    float pv[4][TC];
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      const int tap = taps[k0 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i) pv[i][j] = load_tap(a, rs, pv_ok[i] ? tap : -1, pb[i], ph[i], pw[i]);
    }
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      if (k0 + j < K) {
        const float4* wr = reinterpret_cast<const float4*>(wcol + (k0 + j) * 64);
        float wv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 w4 = wr[q];
          wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 16; ++c) acc[i][c] += pv[i][j] * wv[c];
      }
    }
  }
  // round to the stored bf16 values (BN statistics describe what is stored)
  float s1[16], s2[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) { s1[c] = 0.f; s2[c] = 0.f; }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32 packed[8];
#pragma unroll
    for (int c = 0; c < 16; c += 2) {
      const u16 lo = f2bf(acc[i][c]), hi = f2bf(acc[i][c + 1]);
      packed[c / 2] = (u32)lo | ((u32)hi << 16);
      if (pv_ok[i]) {
        const float flo = bf2f(lo), fhi = bf2f(hi);
        s1[c] += flo; s2[c] += flo * flo;
        s1[c + 1] += fhi; s2[c + 1] += fhi * fhi;
      }
    }
    // stage the block's [256 px][64 ch] bf16 tile in LDS: a lane's own pixels are
    // 4 rows apart in the output, so direct 16-B stores would scatter
    uint4* t = reinterpret_cast<uint4*>(ot + (lane * 4 + i) * kOutPitch + wid * 16);
    t[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    t[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
  }
  __syncthreads();
  // coalesced write-out: 8 threads per 128-B pixel row
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int idx = pass * 256 + tid;
    const int row = idx >> 3, ch = idx & 7;
    const int p = blockIdx.x * 256 + row;
    if (p < a.P)
      *reinterpret_cast<uint4*>(a.y + (long long)p * a.CO + co0 + ch * 8) =
          *reinterpret_cast<const uint4*>(ot + row * kOutPitch + ch * 8);
  }
  if (a.part == nullptr) return;
  // 16 channels x 64 lanes: halve over lane bits 3..0 (lane ends up owning
  // channel lane & 15), then fold lane bits 4, 5
  halve<8>(s1, lane); halve<4>(s1, lane); halve<2>(s1, lane); halve<1>(s1, lane);
  halve<8>(s2, lane); halve<4>(s2, lane); halve<2>(s2, lane); halve<1>(s2, lane);
  float t1 = s1[0], t2 = s2[0];
  t1 += __shfl_xor(t1, 16, 64); t2 += __shfl_xor(t2, 16, 64);
  t1 += __shfl_xor(t1, 32, 64); t2 += __shfl_xor(t2, 32, 64);
  if (lane < 16) {
    const int c = co0 + wid * 16 + lane;
    const int slot = blockIdx.x % kBnSlots;
    atomicAdd(a.part + (long long)slot * a.CO + c, t1);
    atomicAdd(a.part + (long long)(kBnSlots + slot) * a.CO + c, t2);
  }
}

// wgrad: blockIdx.z = 32-tap pass.  Lane = (co quad cq = lane & 15, tap octet
// ko = lane >> 4) -> 4 x 8 outputs per lane, 32 FMAs per (float4 dY + 2 float4
// patch) LDS reads; the 4 waves split each 64-pixel slab's rows and are summed
// through LDS.  Each block stores its [64][32] tile to ws[blockIdx.x] (plain
// stores); conv_small_wgrad_reduce then adds the G tiles into dW -- every
// block hitting the same 1.7k addresses with fp32 atomics serialises at the
// memory-side atomic units.
__global__ void __launch_bounds__(256) conv_small_wgrad_kernel(SmallConvArgs a) {
  constexpr int SLAB = 64, KT = 32;
  // [SLAB][64] dY slab + [SLAB][KT] patch slab; afterwards the same 24 KiB
  // hold waves 1..3's [64][KT] tiles for the cross-wave sum
  __shared__ __attribute__((aligned(16))) float smem[SLAB * 64 + SLAB * KT];
  static_assert(3 * 64 * KT == SLAB * 64 + SLAB * KT, "reduction tile reuses the slabs");
  __shared__ int taps[KT];
  __shared__ int4 rows[2][SLAB];   // pixel decode of slab s in rows[s & 1]
  float* dyl = smem;
  float* pl = smem + SLAB * 64;
  float* red = smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int co0 = blockIdx.y * 64, k0 = blockIdx.z * KT;
  const int cq = lane & 15, ko = lane >> 4;
  const __amdgpu_buffer_rsrc_t rs = image_rsrc(a);
  const int p_begin = blockIdx.x * a.chunk;
  const int p_end = min((int)a.P, p_begin + a.chunk);
  const int nslab = (p_end - p_begin + SLAB - 1) / SLAB;
  auto fill_rows = [&](int sl) {       // threads 0..63, slab sl
    const int p = p_begin + sl * SLAB + tid;
    const bool ok = sl < nslab && p < p_end;
    const int3 d = decode_pixel(a, ok ? p : p_begin);
    rows[sl & 1][tid] = make_int4(d.x, d.y, d.z, ok);
  };
  // slab operands in registers: this thread's 16 dY values and 8 patch taps
  uint4 rdy0, rdy1;
  float rg[SLAB * KT / 256];
  auto load_slab = [&](int sl) {
    {
      const int r = tid >> 2, c = (tid & 3) * 16;
      const int p = p_begin + sl * SLAB + r;
      if (sl < nslab && p < p_end) {
        const uint4* src = reinterpret_cast<const uint4*>(a.dy + (long long)p * a.CO + co0 + c);
        rdy0 = src[0];
        rdy1 = src[1];
      } else {
        rdy0 = rdy1 = make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int it = 0; it < SLAB * KT / 256; ++it) {
      const int i = it * 256 + tid;
      const int r = i / KT, k = i % KT;
      const int4 e = rows[sl & 1][r];
      rg[it] = load_tap(a, rs, e.w ? taps[k] : -1, e.x, e.y, e.z);
    }
  };
  auto store_slab = [&]() {
    const int r = tid >> 2, c = (tid & 3) * 16;
    float4* d = reinterpret_cast<float4*>(dyl + r * 64 + c);
    const u32 u[8] = {rdy0.x, rdy0.y, rdy0.z, rdy0.w, rdy1.x, rdy1.y, rdy1.z, rdy1.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      d[q] = make_float4(bf2f((u16)(u[2 * q] & 0xffff)), bf2f((u16)(u[2 * q] >> 16)),
                         bf2f((u16)(u[2 * q + 1] & 0xffff)), bf2f((u16)(u[2 * q + 1] >> 16)));
#pragma unroll
    for (int it = 0; it < SLAB * KT / 256; ++it) pl[it * 256 + tid] = rg[it];
  };

  float acc[4][8];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[c][j] = 0.f;
  // prologue: tables for slabs 0 and 1, slab 0 staged
  if (tid < KT) taps[tid] = tap_of(a, k0 + tid);
  if (tid < SLAB) fill_rows(0);
  __syncthreads();
  load_slab(0);
  store_slab();
  if (tid < SLAB) fill_rows(1);
  __syncthreads();
  for (int sl = 0; sl < nslab; ++sl) {
    // next slab's global loads fly while this one is consumed from LDS
    if (sl + 1 < nslab) load_slab(sl + 1);
#pragma unroll 4
    for (int rr = 0; rr < SLAB / 4; ++rr) {
      const int r = rr * 4 + wid;
      const float4 d = *reinterpret_cast<const float4*>(dyl + r * 64 + cq * 4);
      const float4 v0 = *reinterpret_cast<const float4*>(pl + r * KT + ko * 8);
      const float4 v1 = *reinterpret_cast<const float4*>(pl + r * KT + ko * 8 + 4);
      const float dv[4] = {d.x, d.y, d.z, d.w};
      const float pv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c][j] += dv[c] * pv[j];
    }
    __syncthreads();   // slab sl consumed; its row table slot is free
    if (sl + 1 < nslab) {
      store_slab();
      if (tid < SLAB) fill_rows(sl + 2);
    }
    __syncthreads();
  }
  // sum the 4 waves: waves 1..3 park their tiles, wave 0 adds and stores
  __syncthreads();
  if (wid > 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[((wid - 1) * 64 + cq * 4 + c) * KT + ko * 8 + j] = acc[c][j];
  }
  __syncthreads();
  if (wid == 0) {
    float* tile = a.ws + (long long)blockIdx.x * a.CO * a.K;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int co = co0 + cq * 4 + c;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kl = ko * 8 + j;
        float v = acc[c][j];
#pragma unroll
        for (int w = 0; w < 3; ++w) v += red[(w * 64 + cq * 4 + c) * KT + kl];
        if (k0 + kl < a.K) tile[(long long)co * a.K + k0 + kl] = v;
      }
    }
  }
}

// dw[i] += sum_g ws[g][i]: block (x, y) sums outputs [64x, 64x+64) over the
// y-th 1/16 of the G tiles (4 waves split it), one fp32 atomic per output
__global__ void __launch_bounds__(256) conv_small_wgrad_reduce(const float* __restrict__ ws,
                                                               float* __restrict__ dw, int n,
                                                               int G) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int w = threadIdx.x >> 6;
  const int g0 = (int)((long long)G * blockIdx.y / gridDim.y);
  const int g1 = (int)((long long)G * (blockIdx.y + 1) / gridDim.y);
  __shared__ float red[4][64];
  float v0 = 0.f, v1 = 0.f;
  if (i < n) {
    int g = g0 + w;
    for (; g + 4 < g1; g += 8) {
      v0 += ws[(long long)g * n + i];
      v1 += ws[(long long)(g + 4) * n + i];
    }
    for (; g < g1; g += 4) v0 += ws[(long long)g * n + i];
  }
  red[w][threadIdx.x & 63] = v0 + v1;
  __syncthreads();
  if (threadIdx.x < 64 && i < n)
    atomicAdd(dw + i, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                          red[3][threadIdx.x]);
}

static SmallConvArgs small_args(const u16* x, int xbytes, int sb, int sh, int sw, int sc, int B, int H, int W, int CI, int OH, int OW, int CO,
                                int R, int S, int stride, int pad) {
  SmallConvArgs a{};
  a.x = x;
  a.xbytes = xbytes;
  a.sb = sb; a.sh = sh; a.sw = sw; a.sc = sc;
  a.B = B; a.H = H; a.W = W; a.CI = CI; a.OH = OH; a.OW = OW; a.CO = CO;
  a.R = R; a.S = S; a.stride = stride; a.pad = pad; a.K = R * S * CI;
  a.P = (long long)B * OH * OW;
  return a;
}

int conv_small_max_k() { return 384; }   // forward weight tile [K][64] fp32 must fit LDS

long long conv_small_fwd_blocks(long long P) { return (P + 255) / 256; }

void launch_conv_small_fwd(const u16* x, int xbytes, int sb, int sh, int sw, int sc,
                           const u16* w, u16* y, float* part, int B, int H, int W, int CI, int OH,
                           int OW, int CO, int R, int S, int stride, int pad, hipStream_t s) {
  SmallConvArgs a = small_args(x, xbytes, sb, sh, sw, sc, B, H, W, CI, OH, OW, CO, R, S, stride, pad);
  a.w = w;
  a.y = y;
  a.part = part;
  const int Kp = (a.K + 7) / 8 * 8;
  const size_t lds = (size_t)((a.K * 64 + Kp + 3) & ~3) * 4 + 256 * kOutPitch * 2;
  const dim3 grid((unsigned)conv_small_fwd_blocks(a.P), (unsigned)(CO / 64));
  hipLaunchKernelGGL(conv_small_fwd_kernel, grid, dim3(256), lds, s, a);
}

int conv_small_wgrad_blocks(long long P, int CO, int R, int S, int CI) {
  (void)CO; (void)R; (void)S; (void)CI;
  // ~4 blocks (16 waves) per CU: one 4-wave block per CU leaves every SIMD a
  // single wave and the LDS -> FMA chains unhidden; whole 64-pixel slabs
  long long chunk = (P + 1023) / 1024;
  chunk = (chunk + 63) / 64 * 64;
  if (chunk < 256) chunk = 256;
  return (int)((P + chunk - 1) / chunk);
}

void launch_conv_small_wgrad(const u16* dy, const u16* x, int xbytes, int sb, int sh, int sw, int sc,
                             float* dw, float* ws, int B, int H, int W, int CI, int OH, int OW,
                             int CO, int R, int S, int stride, int pad, hipStream_t s) {
  SmallConvArgs a = small_args(x, xbytes, sb, sh, sw, sc, B, H, W, CI, OH, OW, CO, R, S, stride, pad);
  a.dy = dy;
  a.dw = dw;
  a.ws = ws;
  const int G = conv_small_wgrad_blocks(a.P, CO, R, S, CI);
  a.chunk = (int)((a.P + G - 1) / G);
  a.chunk = (a.chunk + 63) / 64 * 64;
  const dim3 grid((unsigned)G, (unsigned)(CO / 64), (unsigned)((a.K + 31) / 32));
  hipLaunchKernelGGL(conv_small_wgrad_kernel, grid, dim3(256), 0, s, a);
  const int n = CO * a.K;
  hipLaunchKernelGGL(conv_small_wgrad_reduce, dim3((n + 63) / 64, 16), dim3(256), 0, s, ws, dw, n,
                     G);
}


// ------------------------------------------------------------------------------
// CIFAR-style stem on the matrix cores: 3x3, stride 1, pad 1, CI <= 3 (K = 9*CI
// <= 27 padded to one 32-deep MFMA k-step), CO = 64.  The VALU kernels above spend
// ~60 us per ResNet-18 bs512 step in each direction on 1.8 GFLOP; here both
// passes are a handful of v_mfma_f32_16x16x32_bf16 per 16 / 32 pixels and run at
// the output / dY streaming rate.
//
// forward: D[co][px] = W[co][k] X[k][px].  The four 16-row weight fragments (all
//   64 output channels) live in registers for the whole block; a lane gathers its
//   B fragment (8 taps k = 8*(lane>>4)+i of pixel lane & 15) straight from the
//   L2-resident input through the buffer unit (padding taps read 0 via an
//   out-of-range offset).  The D layout gives a lane 4 consecutive channels of one
//   pixel: 8-B stores, and the BN partial sums of the stored (bf16-rounded)
//   values accumulate in registers, reduced once per block over the 16 pixel
//   lanes (xor shuffles) and the 4 waves (LDS) into slot blockIdx % kBnSlots.
// wgrad: D[co][k] = dY^T[co][px] X[px][k] over 32-pixel k-steps.  dY[32 px][64]
//   is staged row-major into a [32][128] LDS image (chunk-swizzled like the GEMM's
//   transposed operands, mfma_prims.h toff) and read with ds_read_b64_tr_b16, which
//   hands a lane 8 consecutive pixels of one channel; X fragments (8 consecutive
//   pixels of one tap: one image row when W % 8 == 0) are gathered from L2.  Each
//   wave owns a 32-pixel slice of a 128-pixel step, 8 MFMAs; the 4 waves' 64 x 32
//   tiles are summed in LDS and flushed with one fp32 atomic per weight per block.
struct Stem3Args {
  const u16* x;
  const u16* w;     // [64][3][3][CI] bf16
  const u16* dy;    // [P][64]
  u16* y;           // [P][64]
  float* part;      // [2][kBnSlots][64]
  float* dw;        // [64][K] fp32 (+=)
  int sb, sh, sw, sc, xbytes;
  int H, W, CI, K;
  long long P;
  int groups;       // forward: 16-pixel groups per wave; wgrad: 128-pixel steps per block
};

// per-lane tap table for k = 8*(lane>>4) + i: (dr, ds) in [-1, 1], ci; invalid k -> r = 9
__device__ __forceinline__ void s3_taps(int CI, int K, int kg, int dr[8], int ds[8], int ci[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = kg * 8 + i;
    const int c = k % CI, rs = k / CI;
    dr[i] = k < K ? rs / 3 - 1 : 9;
    ds[i] = rs % 3 - 1;
    ci[i] = c;
  }
}

__global__ void __launch_bounds__(256) stem3_fwd_kernel(Stem3Args a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int kg = lane >> 4, col = lane & 15;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
  // weight fragments: row co = 16j + col, k = 8kg..8kg+7
  bf16x8 wf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kg * 8 + i;
      wf[j].v[i] = k < a.K ? a.w[(16 * j + col) * a.K + k] : (u16)0;
    }
  int dr[8], ds[8], ci[8];
  s3_taps(a.CI, a.K, kg, dr, ds, ci);
  float s[4][4], q[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s[j][r] = 0.f; q[j][r] = 0.f; }
  const long long base = ((long long)blockIdx.x * 4 + wid) * a.groups * 16;
  __shared__ __attribute__((aligned(16))) u16 stg[4][16][72];   // per wave: 16 pixels x 64 ch (+pad)
  // the 8-tap gather of group gi+1 is issued before group gi's MFMAs and stores:
  // one dependent L2 round trip per group otherwise set the kernel time (a wave
  // walks its groups in sequence at 2 waves / SIMD)
  auto gather = [&](int gi, bf16x8& xf) {
    const long long px = base + gi * 16 + col;
    const bool pv = px < a.P;
    const int p32 = pv ? (int)px : 0;
    const int ow = p32 % a.W, t = p32 / a.W;
    const int oh = t % a.H, b = t / a.H;
    const int boff = b * a.sb;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ih = oh + dr[i], iw = ow + ds[i];
      const bool ok = pv && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      const int off = ok ? 2 * (boff + ih * a.sh + iw * a.sw + ci[i] * a.sc) : 0x7ffffff0;
      xf.v[i] = __builtin_bit_cast(u16, __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
    }
  };
  bf16x8 xnext;
  gather(0, xnext);
  for (int gi = 0; gi < a.groups; ++gi) {
    const long long px = base + gi * 16 + col;
    const bool pv = px < a.P;
    const bf16x8 xf = xnext;
    if (gi + 1 < a.groups) gather(gi + 1, xnext);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mfma16(wf[j], xf, f32x4{0.f, 0.f, 0.f, 0.f});
    // D: lane holds channels 16j + 4kg + r of pixel `col`... of THIS group's pixel px
    // (D row = co, D col = pixel: lane = (row block kg, col))
    // the D fragments (8 B per lane: 16 pixels x 32 B per store instruction) go
    // through a wave-private LDS tile and leave as whole 128-B pixel rows (16 B
    // per lane, 8 pixels per instruction); LDS ops of one wave complete in order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o.v[r] = f2bf(acc[j][r]);
        const float v = pv ? bf2f(o.v[r]) : 0.f;
        s[j][r] += v;
        q[j][r] += v * v;
      }
      *reinterpret_cast<bf16x4*>(&stg[wid][col][16 * j + 4 * kg]) = o;
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int pr = hh * 8 + (lane >> 3), ck = lane & 7;
      const long long pxo = base + gi * 16 + pr;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(&stg[wid][pr][ck * 8]);
      if (pxo < a.P) *reinterpret_cast<bf16x8*>(a.y + pxo * 64 + ck * 8) = v;
    }
  }
  if (a.part == nullptr) return;
  // reduce over the 16 pixel lanes sharing kg
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        s[j][r] += __shfl_xor(s[j][r], o, 64);
        q[j][r] += __shfl_xor(q[j][r], o, 64);
      }
  __shared__ float red[4][2][64];
  if (col == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[wid][0][16 * j + 4 * kg + r] = s[j][r];
        red[wid][1][16 * j + 4 * kg + r] = q[j][r];
      }
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = threadIdx.x & 63, h = threadIdx.x >> 6;
    const float v = red[0][h][c] + red[1][h][c] + red[2][h][c] + red[3][h][c];
    const int slot = blockIdx.x % kBnSlots;
    atomicAdd(a.part + (long long)(h * kBnSlots + slot) * 64 + c, v);
  }
}

// (dY stages as a [32][128] bf16 transposed-read image: toff<128>, mfma_prims.h)
__global__ void __launch_bounds__(256) stem3_wgrad_kernel(Stem3Args a) {
  __shared__ __attribute__((aligned(16))) u16 img[4][32 * 128];
  __shared__ float tile[64][33];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kg = lane >> 4, col = lane & 15;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
  // this lane's two B columns: taps 16t + col, t = 0, 1
  int tdr[2], tds[2], tci[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = 16 * t + col;
    tdr[t] = k < a.K ? (k / a.CI) / 3 - 1 : 9;
    tds[t] = (k / a.CI) % 3 - 1;
    tci[t] = k % a.CI;
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) { acc[j][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[j][1] = acc[j][0]; }
  u16* im = img[wid];
  const long long blk0 = (long long)blockIdx.x * a.groups * 128;
  // step st+1's dY chunks and X taps are loaded into registers before step st's
  // LDS image write and MFMAs (each step was one dependent round trip)
  auto load_step = [&](int st, bf16x8 (&dv)[4], bf16x8 (&xf)[2]) {
    const long long p0 = blk0 + (long long)st * 128 + wid * 32;   // this wave's 32 pixels
    // dY[p0 .. p0+32)[0..64) : 256 real 16-B chunks per wave image, 4 per lane
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = u * 64 + lane;              // logical chunk: row e >> 3, cols (e & 7) * 8
      const int row = e >> 3, c0 = (e & 7) * 8;
      const long long p = p0 + row;
      if (p < a.P) dv[u] = *reinterpret_cast<const bf16x8*>(a.dy + p * 64 + c0);
      else {
#pragma unroll
        for (int i = 0; i < 8; ++i) dv[u].v[i] = 0;
      }
    }
    // X fragments: pixels p0 + 8kg + i (one image row when W % 8 == 0), taps 16t + col
    {
      const long long pb = p0 + 8 * kg;
      const bool pv = pb < a.P;
      const int p32 = pv ? (int)pb : 0;
      const int ow0 = p32 % a.W, t0 = p32 / a.W;
      const int oh = t0 % a.H, b = t0 / a.H;
      const int boff = b * a.sb;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ih = oh + tdr[t];
        const bool rok = pv && (unsigned)ih < (unsigned)a.H;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int iw = ow0 + i + tds[t];
          const bool ok = rok && (unsigned)iw < (unsigned)a.W && pb + i < a.P;
          const int off = ok ? 2 * (boff + ih * a.sh + iw * a.sw + tci[t] * a.sc) : 0x7ffffff0;
          xf[t].v[i] = __builtin_bit_cast(u16, __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
        }
      }
    }
  };
  bf16x8 dnext[4], xnext[2];
  load_step(0, dnext, xnext);
  for (int st = 0; st < a.groups; ++st) {
    bf16x8 dcur[4], xf[2];
#pragma unroll
    for (int u = 0; u < 4; ++u) dcur[u] = dnext[u];
    xf[0] = xnext[0];
    xf[1] = xnext[1];
    if (st + 1 < a.groups) load_step(st + 1, dnext, xnext);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = u * 64 + lane;
      *reinterpret_cast<bf16x8*>(im + toff<128>(e >> 3, (e & 7) * 8)) = dcur[u];   // 8 cols stay in one granule
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS image writes landed
    __builtin_amdgcn_wave_barrier();
    // A fragments (co tile j): lane row co = 16j + col... read transposed: 8 consecutive
    // pixels (k) 8kg..8kg+7 of channel column
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = lane >> 4, li = lane & 15, qq = li >> 2, pp = li & 3;
      const int row = 8 * g + qq;
      const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4_t*)(im + toff<128>(row, 16 * j + 4 * pp)));
      const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4_t*)(im + toff<128>(row + 4, 16 * j + 4 * pp)));
      const bf16x8 af = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      acc[j][0] = mfma16(af, xf[0], acc[j][0]);
      acc[j][1] = mfma16(af, xf[1], acc[j][1]);
    }
    __builtin_amdgcn_wave_barrier();
  }
  // sum the 4 waves' [64 co][32 k] tiles, one atomic per weight per block
  // D: lane holds rows co = 16j + 4kg + r, column k = 16t + col
  for (int w = 0; w < 4; ++w) {
    if (wid == w) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float& d = tile[16 * j + 4 * kg + r][16 * t + col];
            d = (w == 0 ? 0.f : d) + acc[j][t][r];
          }
    }
    __syncthreads();
  }
  for (int e = tid; e < 64 * a.K; e += 256) {
    const int co = e / a.K, k = e % a.K;
    atomicAdd(a.dw + e, tile[co][k]);
  }
}

// ------------------------------------------------------------------------------
// Stem backward in one pass: BatchNorm(+ReLU) backward and the conv's weight
// gradient together.  The stem's input is data, so the BN's dx exists only for
// the weight gradient to read back, and it is affine per channel:
//   dx = k1 dz + Cc x0 + Bc,   dz = dy [y > 0]   (k1, Cc, Bc: bn.hip fold_bwd_coefs)
//   dW[co][k] = sum_p dx[p][co] patch[p][k] = k1 G1[co][k] + Cc G2[co][k] + Bc G3[k]
//   G1 = sum_p dz patch,  G2 = sum_p x0 patch,  G3 = sum_p patch
// G1, G2, G3 and the BN sums S1 = sum dz, S2 = sum dz xhat come from ONE pass over
// dy and x0 (the conv's stored output); the coefficients, which need S1 and S2
// complete, are applied afterwards to 64 x K numbers (stem3_bn_bwd_finalize_kernel,
// one block).  dx is never written, x0 and dy are read once instead of twice, and
// the bf16 rounding of dx is gone.
//
// The pass is stem3_wgrad_kernel with a double-width LDS image: toff<128> spreads
// a row over all 128 columns already, so dz takes columns 0..63 and x0 columns
// 64..127 of the same 8 KiB per wave, and the 8 extra MFMAs for G2 reuse the
// gathered patch fragments.  A lane's four 16-B chunks per step always cover the
// same 8 channels (lane & 7), so the mask parameters and S1 / S2 live in
// registers.  Block end: the four waves' tiles are summed in LDS (over the image
// storage) and flushed with one fp32 atomic per element into the layer's
// persistent scratch, laid out as below; the finalize kernel re-zeroes it.
constexpr int kS3KP = 32;                         // K padded to the MFMA k-step
constexpr int kS3G1 = 0;                          // [64][kS3KP]
constexpr int kS3G2 = kS3G1 + 64 * kS3KP;         // [64][kS3KP]
constexpr int kS3G3 = kS3G2 + 64 * kS3KP;         // [kS3KP]
constexpr int kS3S1 = kS3G3 + kS3KP;              // [64]
constexpr int kS3S2 = kS3S1 + 64;                 // [64]
constexpr int kS3Scratch = kS3S2 + 64;

struct Stem3BnArgs {
  const u16* x;       // the conv's input image (element strides below)
  const u16* x0;      // [P][64] the conv's stored output = the BN's input
  const u16* dy;      // [P][64] gradient of the BN + ReLU output
  const float* stats; // [4][64] mean | invstd | scale | shift of the forward
  float* scratch;     // [kS3Scratch] (+=)
  int sb, sh, sw, sc, xbytes;
  int H, W, CI, K;
  long long P;
  int groups;         // 128-pixel steps per block
};

__global__ void __launch_bounds__(256) stem3_bn_bwd_kernel(Stem3BnArgs a) {
  // per wave [32 px][dz 64 | x0 64] transposed-read image; afterwards the same
  // storage holds the block's G1 / G2 / G3 tiles
  __shared__ __attribute__((aligned(16))) u16 img[4][32 * 128];
  __shared__ float red[4][2][64];
  __shared__ __attribute__((aligned(16))) float prm[3][64];   // mean | scale | shift
  static_assert(sizeof(img) >= (2 * 64 * 33 + kS3KP) * sizeof(float), "tiles reuse the image");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kg = lane >> 4, col = lane & 15;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.xbytes, 0x00020000);
  int tdr[2], tds[2], tci[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int k = 16 * t + col;
    tdr[t] = k < a.K ? (k / a.CI) / 3 - 1 : 9;
    tds[t] = (k / a.CI) % 3 - 1;
    tci[t] = k % a.CI;
  }
  // this lane's 8 channels of every chunk it loads.  The mask parameters are read
  // from LDS four channels at a time inside the loop: held in registers for the
  // whole kernel (24 of them) they cost a wave per SIMD
  const int c0 = (lane & 7) * 8;
  if (tid < 192) prm[tid >> 6][tid & 63] = a.stats[(tid < 64 ? 0 : (tid >> 6) + 1) * 64 + (tid & 63)];
  __syncthreads();
  float s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  float g3[2] = {0.f, 0.f};
  f32x4 acc1[4][2], acc2[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      acc1[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc2[j][t] = acc1[j][t];
    }
  u16* im = img[wid];
  const long long blk0 = (long long)blockIdx.x * a.groups * 128;
  auto load_step = [&](int st, bf16x8 (&dv)[4], bf16x8 (&xv)[4], bf16x8 (&xf)[2]) {
    const long long p0 = blk0 + (long long)st * 128 + wid * 32;   // this wave's 32 pixels
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = p0 + u * 8 + (lane >> 3);
      if (p < a.P) {
        dv[u] = *reinterpret_cast<const bf16x8*>(a.dy + p * 64 + c0);
        xv[u] = *reinterpret_cast<const bf16x8*>(a.x0 + p * 64 + c0);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { dv[u].v[i] = 0; xv[u].v[i] = 0; }
      }
    }
    // patch fragments: pixels p0 + 8kg + i (one image row: W % 8 == 0), taps 16t + col
    {
      const long long pb = p0 + 8 * kg;
      const bool pv = pb < a.P;
      const int p32 = pv ? (int)pb : 0;
      const int ow0 = p32 % a.W, t0 = p32 / a.W;
      const int oh = t0 % a.H, b = t0 / a.H;
      const int boff = b * a.sb;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ih = oh + tdr[t];
        const bool rok = pv && (unsigned)ih < (unsigned)a.H;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int iw = ow0 + i + tds[t];
          const bool ok = rok && (unsigned)iw < (unsigned)a.W && pb + i < a.P;
          const int off = ok ? 2 * (boff + ih * a.sh + iw * a.sw + tci[t] * a.sc) : 0x7ffffff0;
          xf[t].v[i] = __builtin_bit_cast(u16, __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0));
        }
      }
    }
  };
  // dy / x0 chunks and patch taps of one step: loaded for step st + 1 as soon as
  // step st's are staged to LDS, so the loads fly during the tr reads and MFMAs (a
  // second register set for a full-step prefetch costs a wave per SIMD)
  bf16x8 dv[4], xv[4], xn[2];
  load_step(0, dv, xv, xn);
  for (int st = 0; st < a.groups; ++st) {
    int pofs = c0;
    asm volatile("" : "+v"(pofs));        // keeps the parameter reads inside the loop
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {      // four channels' parameters at a time
      const float4 m4 = *reinterpret_cast<const float4*>(&prm[0][pofs + 4 * hf]);
      const float4 c4 = *reinterpret_cast<const float4*>(&prm[1][pofs + 4 * hf]);
      const float4 h4 = *reinterpret_cast<const float4*>(&prm[2][pofs + 4 * hf]);
      const float mean[4] = {m4.x, m4.y, m4.z, m4.w}, msc[4] = {c4.x, c4.y, c4.z, c4.w},
                  msh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int i = 4 * hf + ii;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float xx = bf2f(xv[u].v[i]);
          // exactly bn.hip relu_mask_from_x: the y > 0 test on the stored bf16 y
          const float yy = fmaxf(bn_pre(xx, msc[ii], msh[ii]), 0.f);
          const bool keep = bf2f(f2bf(yy)) > 0.f;
          dv[u].v[i] = keep ? dv[u].v[i] : (u16)0;   // dy -> dz in place
          const float g = bf2f(dv[u].v[i]);
          s1[i] += g;
          s2[i] += g * (xx - mean[ii]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = u * 8 + (lane >> 3);
      *reinterpret_cast<bf16x8*>(im + toff<128>(row, c0)) = dv[u];          // 8 cols stay in one granule
      *reinterpret_cast<bf16x8*>(im + toff<128>(row, 64 + c0)) = xv[u];
    }
    bf16x8 xf[2];
    xf[0] = xn[0];
    xf[1] = xn[1];
    if (st + 1 < a.groups) load_step(st + 1, dv, xv, xn);
    // G3: this lane's patch values are pixels 8kg + i of taps 16t + col
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 8; ++i) g3[t] += bf2f(xf[t].v[i]);
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS image writes landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h)           // h = 0: dz -> G1, h = 1: x0 -> G2
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int li = lane & 15, qq = li >> 2, pp = li & 3;
        const int row = 8 * kg + qq, cc = 64 * h + 16 * j + 4 * pp;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)(im + toff<128>(row, cc)));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4_t*)(im + toff<128>(row + 4, cc)));
        const bf16x8 af = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        if (h == 0) {
          acc1[j][0] = mfma16(af, xf[0], acc1[j][0]);
          acc1[j][1] = mfma16(af, xf[1], acc1[j][1]);
        } else {
          acc2[j][0] = mfma16(af, xf[0], acc2[j][0]);
          acc2[j][1] = mfma16(af, xf[1], acc2[j][1]);
        }
      }
    __builtin_amdgcn_wave_barrier();
  }
  // S1 / S2: fold the 8 lanes (lane >> 3) that share a channel octet, then the waves
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s2[i] *= a.stats[64 + c0 + i];        // xhat = (x0 - mean) * invstd
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      s1[i] += __shfl_xor(s1[i], o, 64);
      s2[i] += __shfl_xor(s2[i], o, 64);
    }
  }
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[wid][0][c0 + i] = s1[i];
      red[wid][1][c0 + i] = s2[i];
    }
  }
  // G3: fold the four pixel octets kg
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    g3[t] += __shfl_xor(g3[t], 16, 64);
    g3[t] += __shfl_xor(g3[t], 32, 64);
  }
  __syncthreads();                        // every wave is done with its image
  float (*t1)[33] = reinterpret_cast<float (*)[33]>(&img[0][0]);
  float (*t2)[33] = t1 + 64;
  float* t3 = &t2[64][0];
  // sum the 4 waves' tiles.  D: lane holds rows co = 16j + 4kg + r, column k = 16t + col
  for (int w = 0; w < 4; ++w) {
    if (wid == w) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float& d1 = t1[16 * j + 4 * kg + r][16 * t + col];
            float& d2 = t2[16 * j + 4 * kg + r][16 * t + col];
            d1 = (w == 0 ? 0.f : d1) + acc1[j][t][r];
            d2 = (w == 0 ? 0.f : d2) + acc2[j][t][r];
          }
      if (kg == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) t3[16 * t + col] = (w == 0 ? 0.f : t3[16 * t + col]) + g3[t];
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < 64 * kS3KP; e += 256) {
    const int co = e / kS3KP, k = e % kS3KP;
    if (k < a.K) {
      atomicAdd(a.scratch + kS3G1 + e, t1[co][k]);
      atomicAdd(a.scratch + kS3G2 + e, t2[co][k]);
    }
  }
  if (tid < a.K) atomicAdd(a.scratch + kS3G3 + tid, t3[tid]);
  if (tid >= 64 && tid < 192) {
    const int h = (tid - 64) >> 6, c = tid & 63;
    atomicAdd(a.scratch + (h == 0 ? kS3S1 : kS3S2) + c,
              red[0][h][c] + red[1][h][c] + red[2][h][c] + red[3][h][c]);
  }
}

// One block, launched right after stem3_bn_bwd_kernel (the kernel boundary makes
// its atomics visible): the coefficients with fold_bwd_coefs' arithmetic, dgamma /
// dbeta, dW += k1 G1 + Cc G2 + Bc G3; re-zeroes the scratch for the next call and
// the layer's forward slot sums (as the backward apply's slice_zero does).  A null
// dw / dgamma / dbeta is a frozen parameter: skipped.
__global__ void __launch_bounds__(1024) stem3_bn_bwd_finalize_kernel(
    float* __restrict__ scratch, const float* __restrict__ gamma, const float* __restrict__ stats,
    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dw,
    float* __restrict__ zero_buf, long long M, int K) {
  __shared__ float lk1[64], lbc[64], lcc[64], lg3[kS3KP];
  const int t = threadIdx.x;
  if (t < 64) {
    const float db = scratch[kS3S1 + t];   // sum dz
    const float dg = scratch[kS3S2 + t];   // sum dz * xhat
    if (dgamma) dgamma[t] += dg;
    if (dbeta) dbeta[t] += db;
    const float mean = stats[t], inv = stats[64 + t];
    const float k1 = (gamma ? gamma[t] : 1.f) * inv;
    const float invM = 1.f / (float)M;
    const float Cc = -k1 * inv * dg * invM;
    lk1[t] = k1;
    lbc[t] = -k1 * db * invM - Cc * mean;
    lcc[t] = Cc;
  } else if (t < 64 + kS3KP) {
    lg3[t - 64] = scratch[kS3G3 + t - 64];
  }
  __syncthreads();
  // (1024 threads, every load of the two trips issued up front: the kernel is one
  // dependent chain of latencies on the step's critical path)
#pragma unroll
  for (int e = t; e < 64 * kS3KP; e += 1024) {
    const int co = e / kS3KP, k = e % kS3KP;
    const float g1 = scratch[kS3G1 + e], g2 = scratch[kS3G2 + e];
    if (dw != nullptr && k < K) dw[co * K + k] += lk1[co] * g1 + lcc[co] * g2 + lbc[co] * lg3[k];
    scratch[kS3G1 + e] = 0.f;
    scratch[kS3G2 + e] = 0.f;
  }
  if (t < kS3Scratch - kS3G3) scratch[kS3G3 + t] = 0.f;   // G3, S1, S2 (read before the barrier)
  if (zero_buf != nullptr)
    for (int i = t; i < 2 * kBnSlots * 64; i += 1024) zero_buf[i] = 0.f;
}

bool stem3_supported(int CI, int R, int S, int CO, int stride, int pad, int W) {
  return CI >= 1 && CI <= 3 && R == 3 && S == 3 && CO == 64 && stride == 1 && pad == 1 &&
         W % 8 == 0;
}

void launch_stem3_fwd(const u16* x, int xbytes, int sb, int sh, int sw, int sc, const u16* w,
                      u16* y, float* part, int B, int H, int W, int CI, hipStream_t s) {
  Stem3Args a{};
  a.x = x; a.w = w; a.y = y; a.part = part;
  a.sb = sb; a.sh = sh; a.sw = sw; a.sc = sc; a.xbytes = xbytes;
  a.H = H; a.W = W; a.CI = CI; a.K = 9 * CI;
  a.P = (long long)B * H * W;
  // 16 groups of 16 pixels per wave (1024 pixels per block) unless that leaves
  // fewer than ~2 blocks per CU
  static const int gmax = [] {
    const char* e = getenv("DMP_STEM3_GROUPS");   // A/B knob: max groups per wave
    return e ? atoi(e) : 16;
  }();
  int groups = gmax > 0 ? gmax : 16;
  while (groups > 1 && (a.P + 64LL * groups - 1) / (64LL * groups) < 512) groups >>= 1;
  a.groups = groups;
  const long long nb = (a.P + 64LL * groups - 1) / (64LL * groups);
  hipLaunchKernelGGL(stem3_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
}

void launch_stem3_wgrad(const u16* dy, const u16* x, int xbytes, int sb, int sh, int sw, int sc,
                        float* dw, int B, int H, int W, int CI, hipStream_t s) {
  Stem3Args a{};
  a.x = x; a.dy = dy; a.dw = dw;
  a.sb = sb; a.sh = sh; a.sw = sw; a.sc = sc; a.xbytes = xbytes;
  a.H = H; a.W = W; a.CI = CI; a.K = 9 * CI;
  a.P = (long long)B * H * W;
  // ~512 blocks: 128-pixel steps per block
  static const long long target = [] {
    const char* e = getenv("DMP_STEM3_WG_BLOCKS");   // A/B knob: target block count
    const long long v = e ? atoll(e) : 512;
    return v > 0 ? v : 512;
  }();
  const long long steps = (a.P + 127) / 128;
  long long per = (steps + target - 1) / target;
  // >= 4 steps per block: at the reference batch (512 steps) 128 blocks beat 512 --
  // a quarter of the per-block atomic flushes (ResNet-18 bs64 -0.75 %,
  // profiles/stem3_wgrad_grid_r6.txt); batches >= 256 already run >= 4 per block
  if (per < 4) per = 4;
  a.groups = (int)per;
  const long long nb = (steps + per - 1) / per;
  hipLaunchKernelGGL(stem3_wgrad_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
}

int stem3_bn_bwd_scratch_floats() { return kS3Scratch; }

// 128-pixel steps per block of stem3_bn_bwd_kernel: launch_stem3_wgrad's rule
// (about `target` blocks, default 512; >= 4 steps per block so the per-block
// atomic flush stays a small part of the block's work)
int stem3_bn_bwd_steps(long long P, int target) {
  if (P <= 0 || P >= (1LL << 31)) return 0;   // pixels are indexed in 32 bits
  const long long tg = target > 0 ? target : 512;
  const long long steps = (P + 127) / 128;
  long long per = (steps + tg - 1) / tg;
  if (per < 4) per = 4;
  return per > 0x7fffffff ? 0 : (int)per;
}

long long stem3_bn_bwd_blocks(long long P, int target) {
  const int per = stem3_bn_bwd_steps(P, target);
  return per > 0 ? ((P + 127) / 128 + per - 1) / per : 0;
}

void launch_stem3_bn_bwd(const u16* dy, const u16* x0, const u16* x, int xbytes, int sb, int sh,
                         int sw, int sc, const float* stats, const float* gamma, float* dgamma,
                         float* dbeta, float* dw, float* scratch, float* zero_buf, int B, int H,
                         int W, int CI, int blocks, hipStream_t s) {
  Stem3BnArgs a{};
  a.x = x; a.x0 = x0; a.dy = dy; a.stats = stats; a.scratch = scratch;
  a.sb = sb; a.sh = sh; a.sw = sw; a.sc = sc; a.xbytes = xbytes;
  a.H = H; a.W = W; a.CI = CI; a.K = 9 * CI;
  a.P = (long long)B * H * W;
  a.groups = stem3_bn_bwd_steps(a.P, blocks);
  const long long nb = stem3_bn_bwd_blocks(a.P, blocks);
  hipLaunchKernelGGL(stem3_bn_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(stem3_bn_bwd_finalize_kernel, dim3(1), dim3(1024), 0, s, scratch, gamma, stats,
                     dgamma, dbeta, dw, zero_buf, a.P, a.K);
}

}  // namespace dmp
