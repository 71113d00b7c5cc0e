// Layer-wise adaptive optimizers over the flat arena: LAMB and LARS
// (specification: parallel/fused_optim.py; layout constants: optim_trust.h).
//
// The trust ratio of tensor i needs ||p_i|| and the norm of THIS step's update
// before any element of p_i may be written, so a step is three launches on one
// stream, all driven by one chunk table that is a function of the arena layout
// alone:
//   stage 1  one workgroup per chunk (<= kTrustChunk elements of one tensor):
//            LAMB updates m and v in place and forms u in registers, LARS only
//            reads p and g; per-lane fp32 sums of p^2 and u^2 (g'^2), a fixed
//            cross-lane / cross-wave order, ONE float2 into partials[chunk];
//   reduce   one wave per tensor adds its partials in fp64 in a fixed order and
//            writes the tensor's scalar and both norms;
//   stage 2  the same chunks again: LAMB re-reads m, v, p and recomputes u with
//            the identical expression (lamb_u), LARS reads g, p, mom; then acc,
//            the bf16 shadow and the EMA as the AdamW kernel does them.
// No atomics, nothing to zero (every partial and trust word that is read was
// written by the same step's launches), no host value: the sequence records
// into a step graph once.  Partial k always covers the same elements, whatever
// the grid, so every norm is a pure function of the data.
//
// Pad elements (the tail of a tensor's last 64-element block, the arena's tail)
// are never summed and never written with anything but what they held: the last
// float4 of a chunk is masked by the element count.
//
// A malformed table must not fault the device: every row is checked against the
// arena length again here and a bad one is skipped (its partial reads as 0).
#include "common.h"
#include "launchers.h"
#include "optim_trust.h"

#include <algorithm>

namespace dmp {
namespace {

// words of the hyper block that these kernels read (optim.hip enum HyperWord)
constexpr int kHLr = 1, kHGscale = 2, kHBc1 = 3, kHBc2 = 4, kHBeta1 = 11, kHBeta2 = 12,
              kHOmb1 = 15, kHOmb2 = 16, kHEmaD = 17, kHEmaO = 18;

__device__ __forceinline__ float hyper_load(const float* hyper, int w) {
  return __hip_atomic_load(hyper + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_bf16x4(bf16x4* __restrict__ dst, long long i,
                                             const float4& v) {
  bf16x4 o;
  o.v[0] = f2bf(v.x); o.v[1] = f2bf(v.y); o.v[2] = f2bf(v.z); o.v[3] = f2bf(v.w);
  dst[i] = o;
}

// e = D e + O p, three roundings: the model EMA of optim.hip (ema_lane)
__device__ __forceinline__ float ema_lane(float e, float p, float D, float O) {
#pragma clang fp contract(off)
  const float a = D * e;
  const float b = O * p;
  return a + b;
}

__device__ __forceinline__ void ema_update4(float4* __restrict__ e, long long i, const float4& p,
                                            float D, float O) {
  float4 ev = e[i];
  ev.x = ema_lane(ev.x, p.x, D, O); ev.y = ema_lane(ev.y, p.y, D, O);
  ev.z = ema_lane(ev.z, p.z, D, O); ev.w = ema_lane(ev.w, p.w, D, O);
  e[i] = ev;
}

// ---- the chunk table ----------------------------------------------------------
struct Chunk {
  int tensor;        // row of the tensor table
  long long first4;  // first float4 of the chunk
  int count;         // real elements (the last float4 may hold fewer than four)
  bool ok;
};

__device__ __forceinline__ Chunk load_chunk(const int* __restrict__ chunks, int c, int ntens,
                                            long long n) {
  const int* row = chunks + kTrustRow * (long long)c;
  Chunk k;
  k.tensor = row[0];
  const int start = row[1];
  k.count = row[2];
  k.first4 = start >> 2;
  k.ok = k.tensor >= 0 && k.tensor < ntens && start >= 0 && (start & 63) == 0 && k.count >= 1 &&
         k.count <= kTrustChunk && (long long)start + k.count <= n;
  return k;
}

// ---- sums in a fixed order ----------------------------------------------------
// Sum over the wave: xor 1 and xor 2 inside the quad, row_half_mirror and
// row_mirror give every lane the sum of its row of 16 (both partners of a step
// add the same two values, so they agree bit for bit), then one lane of each
// row is read and the four are added as (r0 + r1) + (r2 + r3).  All 64 lanes
// must be active.
__device__ __forceinline__ float wave_sum_fixed(float x) {
#define DMP_DPP_ADD(ctrl) \
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xF, 0xF, true))
  DMP_DPP_ADD(0xB1);
  DMP_DPP_ADD(0x4E);
  DMP_DPP_ADD(0x141);
  DMP_DPP_ADD(0x140);
#undef DMP_DPP_ADD
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
  const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 32));
  const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 48));
  return (a + b) + (c + d);
}

// The chunk's two sums: wave sums, then the four waves through LDS as
// (w0 + w1) + (w2 + w3); thread 0 stores the one float2 this chunk owns.
__device__ __forceinline__ void store_partial(float sa, float sb, float2* red,
                                              float2* __restrict__ partials, int c) {
  sa = wave_sum_fixed(sa);
  sb = wave_sum_fixed(sb);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(sa, sb);
  __syncthreads();
  if (threadIdx.x == 0)
    partials[c] = make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x),
                              (red[0].y + red[1].y) + (red[2].y + red[3].y));
  __syncthreads();      // red is free for the block's next chunk
}

// ---- LAMB arithmetic ------------------------------------------------------------
struct LambCoef {
  float gscale, b1, b2, omb1, omb2, bc1, sbc2, eps;
};

__device__ __forceinline__ LambCoef lamb_coef(const float* hyper, float eps) {
  LambCoef k;
  k.gscale = hyper_load(hyper, kHGscale);
  k.b1 = hyper_load(hyper, kHBeta1); k.b2 = hyper_load(hyper, kHBeta2);
  k.omb1 = hyper_load(hyper, kHOmb1); k.omb2 = hyper_load(hyper, kHOmb2);
  k.bc1 = hyper_load(hyper, kHBc1);
  k.sbc2 = sqrtf(hyper_load(hyper, kHBc2));
  k.eps = eps;
  return k;
}

// AdamW's moments, its expressions (adamw_fused_step_kernel)
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambCoef& k) {
  const float gs = k.gscale * g;
  m = k.b1 * m + k.omb1 * gs;
  v = k.b2 * v + k.omb2 * (gs * gs);
}

// u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wdd p, every operation rounded on
// its own (contraction off; division and square root are the correctly rounded
// ones).  THE expression of both stages: stage 2 reads back the m and v that
// stage 1 stored and the p that nothing has written since, so it forms the very
// bits whose squares went into the norm.
__device__ __forceinline__ float lamb_u(float m, float v, float p, const LambCoef& k, float wdd) {
#pragma clang fp contract(off)
  const float a = m / k.bc1;
  const float r = sqrtf(v) / k.sbc2;
  const float d = r + k.eps;
  const float q = a / d;
  const float w = wdd * p;
  return q + w;
}

// p - s u with s = fl(lr_t * trust_i): two roundings
__device__ __forceinline__ float axpy_neg(float p, float s, float u) {
#pragma clang fp contract(off)
  const float t = s * u;
  return p - t;
}

// ---- LARS arithmetic ------------------------------------------------------------
// g' = gscale g;  d = local (g' + wdd p);  mom = momentum mom + d, each rounded
// on its own
__device__ __forceinline__ float lars_mom(float g, float p, float mom, float gscale, float wdd,
                                          float local, float momentum) {
#pragma clang fp contract(off)
  const float gs = gscale * g;
  const float w = wdd * p;
  const float s = gs + w;
  const float d = local * s;
  const float a = momentum * mom;
  return a + d;
}

__device__ __forceinline__ float sq_scaled(float gscale, float g) {
#pragma clang fp contract(off)
  const float gs = gscale * g;
  return gs * gs;
}

}  // namespace

// ---- stage 1 ----------------------------------------------------------------------
// NORMS_ONLY = false (LAMB): g, p, m, v in; m, v out; partial = (sum p^2, sum u^2).
// NORMS_ONLY = true  (LARS): g, p in;              partial = (sum p^2, sum g'^2).
// 16-B loads; lanes past the element count in the last float4 neither add to a
// sum nor change m / v.
template <bool NORMS_ONLY>
__global__ void __launch_bounds__(256) lamb_stage1_kernel(
    const int* __restrict__ chunks, int nchunks, const int* __restrict__ tens, int ntens,
    long long n, const float4* __restrict__ g, const float4* __restrict__ p,
    float4* __restrict__ m, float4* __restrict__ v, float2* __restrict__ partials,
    const float* __restrict__ hyper, float weight_decay, float eps) {
  __shared__ float2 red[4];
  const LambCoef k = lamb_coef(hyper, eps);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, ntens, n);       // block-uniform
    float sp = 0.f, su = 0.f;
    if (ch.ok) {
      const float wdd = tens[kTrustRow * ch.tensor + 2] ? weight_decay : 0.f;
      const int n4 = (ch.count + 3) >> 2;
      for (int i = threadIdx.x; i < n4; i += 256) {
        const long long at = ch.first4 + i;
        const int rem = ch.count - 4 * i;                   // >= 1
        const float4 gv = g[at];
        const float4 pv = p[at];
        if constexpr (NORMS_ONLY) {
#define DMP_LARS_NORM_LANE(c, j)                   \
          if (j < rem) {                           \
            sp += pv.c * pv.c;                     \
            su += sq_scaled(k.gscale, gv.c);       \
          }
          DMP_LARS_NORM_LANE(x, 0) DMP_LARS_NORM_LANE(y, 1)
          DMP_LARS_NORM_LANE(z, 2) DMP_LARS_NORM_LANE(w, 3)
#undef DMP_LARS_NORM_LANE
        } else {
          float4 mv = m[at], vv = v[at];
#define DMP_LAMB_NORM_LANE(c, j)                                 \
          if (j < rem) {                                         \
            lamb_moments(gv.c, mv.c, vv.c, k);                   \
            const float u = lamb_u(mv.c, vv.c, pv.c, k, wdd);    \
            sp += pv.c * pv.c;                                   \
            su += u * u;                                         \
          }
          DMP_LAMB_NORM_LANE(x, 0) DMP_LAMB_NORM_LANE(y, 1)
          DMP_LAMB_NORM_LANE(z, 2) DMP_LAMB_NORM_LANE(w, 3)
#undef DMP_LAMB_NORM_LANE
          m[at] = mv;
          v[at] = vv;
        }
      }
    }
    store_partial(sp, su, red, partials, c);
  }
}

// ---- reduce -----------------------------------------------------------------------
// One wave per tensor: lane l adds partials l, l + 64, ... of the tensor's chunks
// in fp64, then a xor butterfly in fp64 (both partners add the same two values);
// a fixed order for a fixed layout.  out[tensor] = (scalar, ||p||, ||u|| or
// ||g'||, 0) with
//   LAMB  scalar = ||p|| / ||u||
//   LARS  scalar = trust_coef ||p|| / (||g'|| + wd ||p|| + lars_eps)
// when the tensor is in the adapt set and both norms are > 0, else 1 (a NaN norm
// is not > 0).  The division runs in fp64 and is rounded to fp32 once.
__global__ void __launch_bounds__(256) trust_reduce_kernel(
    const int* __restrict__ tens, int ntens, int nchunks, const float2* __restrict__ partials,
    float* __restrict__ out, int lars, float weight_decay, float trust_coef, float lars_eps) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= ntens) return;                                   // the whole wave
  const int first = tens[kTrustRow * t], cnt = tens[kTrustRow * t + 1];
  const int adapt = tens[kTrustRow * t + 2];
  const bool ok = first >= 0 && cnt >= 0 && first <= nchunks && cnt <= nchunks - first;
  double a = 0.0, b = 0.0;
  if (ok)
    for (int j = lane; j < cnt; j += 64) {
      const float2 q = partials[first + j];
      a += (double)q.x;
      b += (double)q.y;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (lane != 0) return;
  const double pn = sqrt(a), un = sqrt(b);
  double r = 1.0;
  if (ok && adapt && pn > 0.0 && un > 0.0)
    r = lars ? (double)trust_coef * pn / (un + (double)weight_decay * pn + (double)lars_eps)
             : pn / un;
  float* o = out + kTrustOut * (long long)t;
  o[0] = (float)r; o[1] = (float)pn; o[2] = (float)un; o[3] = 0.f;
}

// ---- stage 2 ----------------------------------------------------------------------
// What follows the new p of one float4, as in adamw_fused_step_kernel
template <bool EMA, typename... E>
__device__ __forceinline__ void finish4(long long at, const float4& p0, const float4& pn,
                                        float4* __restrict__ p, float4* __restrict__ acc,
                                        bf16x4* __restrict__ w16, float emaD, float emaO,
                                        E... ema) {
  p[at] = pn;
  if (acc) {
    float4 a = acc[at];
    a.x += pn.x - p0.x; a.y += pn.y - p0.y; a.z += pn.z - p0.z; a.w += pn.w - p0.w;
    acc[at] = a;
  }
  if (w16) store_bf16x4(w16, at, pn);
  if constexpr (EMA) {
    if (emaO != 0.f) ema_update4(ema..., at, pn, emaD, emaO);
  }
}

// LAMB: p = p - fl(lr_t trust_i) u with u recomputed from the stored m, v and
// the old p.  g is not read.
template <bool EMA, typename... E>
__global__ void __launch_bounds__(256) lamb_stage2_kernel(
    const int* __restrict__ chunks, int nchunks, const int* __restrict__ tens, int ntens,
    long long n, const float* __restrict__ trust, float4* __restrict__ p,
    float4* __restrict__ acc, const float4* __restrict__ m, const float4* __restrict__ v,
    bf16x4* __restrict__ w16, const float* __restrict__ hyper, float weight_decay, float eps,
    E... ema) {
  static_assert(sizeof...(E) == (EMA ? 1 : 0), "EMA: exactly one float4* ema");
  float emaD = 1.f, emaO = 0.f;
  if constexpr (EMA) {
    emaD = hyper_load(hyper, kHEmaD);
    emaO = hyper_load(hyper, kHEmaO);
  }
  const float lr = hyper_load(hyper, kHLr);
  const LambCoef k = lamb_coef(hyper, eps);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, ntens, n);
    if (!ch.ok) continue;
    const float s = lr * trust[kTrustOut * ch.tensor];      // once per workgroup
    const float wdd = tens[kTrustRow * ch.tensor + 2] ? weight_decay : 0.f;
    const int n4 = (ch.count + 3) >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const long long at = ch.first4 + i;
      const int rem = ch.count - 4 * i;
      const float4 p0 = p[at], mv = m[at], vv = v[at];
      float4 pn = p0;
#define DMP_LAMB_APPLY_LANE(c, j) \
      if (j < rem) pn.c = axpy_neg(p0.c, s, lamb_u(mv.c, vv.c, p0.c, k, wdd));
      DMP_LAMB_APPLY_LANE(x, 0) DMP_LAMB_APPLY_LANE(y, 1)
      DMP_LAMB_APPLY_LANE(z, 2) DMP_LAMB_APPLY_LANE(w, 3)
#undef DMP_LAMB_APPLY_LANE
      finish4<EMA>(at, p0, pn, p, acc, w16, emaD, emaO, ema...);
    }
  }
}

// LARS: mom = momentum mom + local_i (g' + wdd p);  p = p - fl(lr_t mom)
template <bool EMA, typename... E>
__global__ void __launch_bounds__(256) lars_stage2_kernel(
    const int* __restrict__ chunks, int nchunks, const int* __restrict__ tens, int ntens,
    long long n, const float* __restrict__ trust, const float4* __restrict__ g,
    float4* __restrict__ p, float4* __restrict__ acc, float4* __restrict__ mom,
    bf16x4* __restrict__ w16, const float* __restrict__ hyper, float weight_decay,
    float momentum, E... ema) {
  static_assert(sizeof...(E) == (EMA ? 1 : 0), "EMA: exactly one float4* ema");
  float emaD = 1.f, emaO = 0.f;
  if constexpr (EMA) {
    emaD = hyper_load(hyper, kHEmaD);
    emaO = hyper_load(hyper, kHEmaO);
  }
  const float lr = hyper_load(hyper, kHLr);
  const float gscale = hyper_load(hyper, kHGscale);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const Chunk ch = load_chunk(chunks, c, ntens, n);
    if (!ch.ok) continue;
    const float local = trust[kTrustOut * ch.tensor];
    const float wdd = tens[kTrustRow * ch.tensor + 2] ? weight_decay : 0.f;
    const int n4 = (ch.count + 3) >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const long long at = ch.first4 + i;
      const int rem = ch.count - 4 * i;
      const float4 gv = g[at], p0 = p[at];
      float4 mo = mom[at];
      float4 pn = p0;
#define DMP_LARS_APPLY_LANE(c, j)                                            \
      if (j < rem) {                                                         \
        mo.c = lars_mom(gv.c, p0.c, mo.c, gscale, wdd, local, momentum);     \
        pn.c = axpy_neg(p0.c, lr, mo.c);                                     \
      }
      DMP_LARS_APPLY_LANE(x, 0) DMP_LARS_APPLY_LANE(y, 1)
      DMP_LARS_APPLY_LANE(z, 2) DMP_LARS_APPLY_LANE(w, 3)
#undef DMP_LARS_APPLY_LANE
      mom[at] = mo;
      finish4<EMA>(at, p0, pn, p, acc, w16, emaD, emaO, ema...);
    }
  }
}

// ---------------------------------------------------------------- launchers
int trust_chunk() { return kTrustChunk; }

static int trust_grid(int nchunks, int grid_cap) {
  const int cap = grid_cap > 0 ? std::min(grid_cap, kTrustGridCap) : kTrustGridCap;
  return std::max(1, std::min(nchunks, cap));
}

void launch_lamb_step(const float* g, float* p, float* acc, float* m, float* v, uint16_t* w16,
                      const TrustTables& t, long long n, const float* hyper, float wd, float eps,
                      int grid_cap, hipStream_t s, float* ema) {
  if (t.nchunks <= 0 || t.ntens <= 0) return;
  const dim3 grid(trust_grid(t.nchunks, grid_cap)), block(256);
  float2* partials = reinterpret_cast<float2*>(t.partials);
  hipLaunchKernelGGL(lamb_stage1_kernel<false>, grid, block, 0, s, t.chunks, t.nchunks, t.tens,
                     t.ntens, n, (const float4*)g, (const float4*)p, (float4*)m, (float4*)v,
                     partials, hyper, wd, eps);
  hipLaunchKernelGGL(trust_reduce_kernel, dim3((t.ntens + 3) / 4), block, 0, s, t.tens, t.ntens,
                     t.nchunks, (const float2*)partials, t.trust, 0, wd, 0.f, 0.f);
  if (ema)
    hipLaunchKernelGGL((lamb_stage2_kernel<true, float4*>), grid, block, 0, s, t.chunks,
                       t.nchunks, t.tens, t.ntens, n, (const float*)t.trust, (float4*)p,
                       (float4*)acc, (const float4*)m, (const float4*)v, (bf16x4*)w16, hyper, wd,
                       eps, (float4*)ema);
  else
    hipLaunchKernelGGL(lamb_stage2_kernel<false>, grid, block, 0, s, t.chunks, t.nchunks, t.tens,
                       t.ntens, n, (const float*)t.trust, (float4*)p, (float4*)acc,
                       (const float4*)m, (const float4*)v, (bf16x4*)w16, hyper, wd, eps);
}

void launch_lars_step(const float* g, float* p, float* acc, float* mom, uint16_t* w16,
                      const TrustTables& t, long long n, const float* hyper, float wd,
                      float momentum, float trust_coef, float lars_eps, int grid_cap,
                      hipStream_t s, float* ema) {
  if (t.nchunks <= 0 || t.ntens <= 0) return;
  const dim3 grid(trust_grid(t.nchunks, grid_cap)), block(256);
  float2* partials = reinterpret_cast<float2*>(t.partials);
  hipLaunchKernelGGL(lamb_stage1_kernel<true>, grid, block, 0, s, t.chunks, t.nchunks, t.tens,
                     t.ntens, n, (const float4*)g, (const float4*)p, (float4*)nullptr,
                     (float4*)nullptr, partials, hyper, wd, 0.f);
  hipLaunchKernelGGL(trust_reduce_kernel, dim3((t.ntens + 3) / 4), block, 0, s, t.tens, t.ntens,
                     t.nchunks, (const float2*)partials, t.trust, 1, wd, trust_coef, lars_eps);
  if (ema)
    hipLaunchKernelGGL((lars_stage2_kernel<true, float4*>), grid, block, 0, s, t.chunks,
                       t.nchunks, t.tens, t.ntens, n, (const float*)t.trust, (const float4*)g,
                       (float4*)p, (float4*)acc, (float4*)mom, (bf16x4*)w16, hyper, wd, momentum,
                       (float4*)ema);
  else
    hipLaunchKernelGGL(lars_stage2_kernel<false>, grid, block, 0, s, t.chunks, t.nchunks, t.tens,
                       t.ntens, n, (const float*)t.trust, (const float4*)g, (float4*)p,
                       (float4*)acc, (float4*)mom, (bf16x4*)w16, hyper, wd, momentum);
}

}  // namespace dmp
