// Flat-arena optimizer / parameter-server kernels (memory-bound, 16 B per lane).
//
// Reference behaviour being re-implemented (not translated):
//   * worker step  /root/reference/asgd/optim/Asynchronous.py:54-68
//       acc += -lr * g          (accumulated_gradients.add_(-lr, gradients))
//       p   += -lr * g          (per-tensor local SGD)
//     here: ONE pass over the flat fp32 arena that also refreshes the bf16
//     compute shadow, instead of a per-step torch.cat ravel + 2 axpys + N
//     per-tensor adds.
//   * PS apply  (missing asgd/server.py, contract in SURVEY.md C7)
//       shard += delta          (delta already carries -lr)
//
// All buffers are padded by the arena to a multiple of 64 elements and are
// 256-B aligned, so n % 4 == 0 always holds (asserted on the host side).
#include "common.h"
#include "launchers.h"

#include <algorithm>

namespace dmp {

// dst[i] = bf16(v): four round-to-nearest-even casts, one 8-B store
__device__ __forceinline__ void store_bf16x4(bf16x4* __restrict__ dst, long long i,
                                             const float4& v) {
  bf16x4 o;
  o.v[0] = f2bf(v.x); o.v[1] = f2bf(v.y); o.v[2] = f2bf(v.z); o.v[3] = f2bf(v.w);
  dst[i] = o;
}

// Model EMA of one element: e = D e + O p with the two products and the sum each
// rounded on its own, the bits of torch's e.mul(D).add(p.mul(O)) on the CPU
// (parallel/fused_optim.py).  Plain operators with contraction off for these
// statements, as in mx8_axpy: the __fmul_rn / __fadd_rn intrinsics inline as
// operations that still carry the header's contract flag, and the backend
// fuses them into one multiply-add (seen in the assembly).
// timm's form: about an ulp of rounding noise per update, and no stalling once
// O |p - e| drops below an ulp of e.
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

// One grid-stride pass of the SGD update, shared by the two kernels below.
// `gscale` (device-hyper variant only, SCALE = true) multiplies the gradient
// before weight decay and momentum see it.  That product is rounded on its own:
// below it is only ever an addend or a factor of the next operation, never a
// product that feeds a sum, so there is no multiply-add to contract it into (the
// __fmul_rn spelling alone would not prevent one, see ema_lane).  gscale == 1
// therefore leaves every later rounding where the by-value kernel has it
// (bitwise-equal results, pinned by a test).
// EMA (device-hyper variant only): `ema` is updated from the new p under the
// grid-uniform branch O != 0, so a step between two EMA updates moves none of
// its bytes.  Without EMA the three trailing arguments do not exist in the code.
template <bool SCALE, bool EMA = false>
__device__ __forceinline__ void asgd_fused_step_body(
    const float4* __restrict__ g, float4* __restrict__ p, float4* __restrict__ acc,
    float4* __restrict__ mom, bf16x4* __restrict__ w16, long long n4, float lr, float gscale,
    float weight_decay, float momentum, float dampening, int nesterov, long long first,
    long long stride, float4* __restrict__ ema = nullptr, float D = 1.f, float O = 0.f) {
  for (long long i = first; i < n4; i += stride) {
    float4 gv = g[i];
    float4 pv = p[i];
    if (SCALE) {
      gv.x = __fmul_rn(gscale, gv.x); gv.y = __fmul_rn(gscale, gv.y);
      gv.z = __fmul_rn(gscale, gv.z); gv.w = __fmul_rn(gscale, gv.w);
    }
    if (weight_decay != 0.f) {
      gv.x += weight_decay * pv.x; gv.y += weight_decay * pv.y;
      gv.z += weight_decay * pv.z; gv.w += weight_decay * pv.w;
    }
    if (mom) {
      float4 m = mom[i];
      const float d = 1.f - dampening;
      m.x = momentum * m.x + d * gv.x; m.y = momentum * m.y + d * gv.y;
      m.z = momentum * m.z + d * gv.z; m.w = momentum * m.w + d * gv.w;
      mom[i] = m;
      if (nesterov) {
        gv.x += momentum * m.x; gv.y += momentum * m.y;
        gv.z += momentum * m.z; gv.w += momentum * m.w;
      } else {
        gv = m;
      }
    }
    const float4 d = make_float4(-lr * gv.x, -lr * gv.y, -lr * gv.z, -lr * gv.w);
    if (acc) {
      float4 a = acc[i];
      a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w;
      acc[i] = a;
    }
    pv.x += d.x; pv.y += d.y; pv.z += d.z; pv.w += d.w;
    p[i] = pv;
    if (w16) store_bf16x4(w16, i, pv);
    if constexpr (EMA) {
      if (O != 0.f) ema_update4(ema, i, pv, D, O);
    }
  }
}

// g      : fp32 gradient (flat)         [n]
// p      : fp32 worker parameters       [n]   (in/out)
// acc    : fp32 push accumulator        [n]   (in/out, may be null)
// mom    : fp32 momentum buffer         [n]   (in/out, may be null)
// w16    : bf16 compute shadow of p     [n]   (out, may be null)
__global__ void __launch_bounds__(256) asgd_fused_step_kernel(
    const float4* __restrict__ g, float4* __restrict__ p, float4* __restrict__ acc,
    float4* __restrict__ mom, bf16x4* __restrict__ w16, long long n4, float lr,
    float weight_decay, float momentum, float dampening, int nesterov) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  asgd_fused_step_body<false>(g, p, acc, mom, w16, n4, lr, 1.f, weight_decay, momentum,
                              dampening, nesterov,
                              (long long)blockIdx.x * blockDim.x + threadIdx.x, stride);
}

// ---- device-resident optimizer state ("hyper block") ------------------------
// One small fp32 / int32 buffer per optimizer holds everything about a step
// that changes from step to step, so a captured step graph bakes none of it
// in (the pattern of dropout.hip's device-side Philox offset).  Words:
enum HyperWord {
  kHStep = 0,       // int32  t: updates applied so far
  kHLr = 1,         // lr_t of the current step
  kHGscale = 2,     // grad_scale * clip coefficient
  kHBc1 = 3,        // 1 - beta1^t
  kHBc2 = 4,        // 1 - beta2^t
  kHNorm = 5,       // grad_scale * ||g||  (0 with clipping off)
  kHKind = 6,       // int32  0 constant, 1 warmup_cosine
  kHBaseLr = 7,
  kHLrMin = 8,
  kHWarmup = 9,     // int32
  kHTotal = 10,     // int32
  kHBeta1 = 11,
  kHBeta2 = 12,
  kHMaxNorm = 13,   // <= 0: clipping off
  kHGradScale = 14,
  kHOmb1 = 15,      // 1 - beta1, rounded from the host's double (as torch passes it)
  kHOmb2 = 16,      // 1 - beta2
  // model EMA (parallel/ema.py): e = D e + O p on the steps with t % K == 0
  kHEmaD = 17,      // fp32(d_u) of this step; 1 on a step without an EMA update
  kHEmaO = 18,      // fp32(1 - d_u), the difference taken in fp64; 0 = EMA untouched
  kHEmaU = 19,      // int32  u = t / K: EMA updates applied so far
  kHEmaDecay = 20,  // base decay
  kHEmaEvery = 21,  // int32  K; 0: EMA off, none of 17..19 is written
  kHEmaWarm = 22,   // int32  1: d_u = min(decay, (1 + u) / (10 + u))
  kHyperWords = 24,
};

__device__ __forceinline__ float hyper_load(const float* hyper, int w) {
  return __hip_atomic_load(hyper + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One block, once per step, on the step's stream BEFORE the update kernel.
//   1. clipping on (nparts > 0): reduce the per-block partials that
//      sumsq_partial_kernel just wrote, in a fixed order (thread t takes
//      partials t, t+256, ...; then a fixed LDS tree), so the norm is a pure
//      function of the gradient;  norm = grad_scale * sqrt(sum)
//   2. clip = min(1, max_norm / (norm + 1e-6))  (torch clip_grad_norm_; a NaN
//      norm stays NaN, an infinite one gives 0 and 0 * inf = NaN downstream)
//   3. t += 1, lr_t from the schedule, bias corrections.
// The scalar part runs on one thread in fp64 (cos / pow once per step): the
// published fp32 values are then correctly rounded up to the fp32 inputs.
__global__ void __launch_bounds__(256) optim_hyper_kernel(float* __restrict__ hyper,
                                                          const float* __restrict__ partial,
                                                          int nparts) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  if (nparts > 0) {
    double s = 0.0;
    for (int i = tid; i < nparts; i += 256) s += (double)partial[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
  }
  if (tid != 0) return;
  int* hi = reinterpret_cast<int*>(hyper);
  const float gs = hyper[kHGradScale];
  const float max_norm = hyper[kHMaxNorm];
  float norm = 0.f, clip = 1.f;
  if (nparts > 0 && max_norm > 0.f) {
    norm = gs * sqrtf((float)red[0]);
    const float c = max_norm / (norm + 1e-6f);
    clip = c < 1.f ? c : (c != c ? c : 1.f);
  }
  const int t = hi[kHStep] + 1;
  const double base = (double)hyper[kHBaseLr], lmin = (double)hyper[kHLrMin];
  const int warm = hi[kHWarmup], total = hi[kHTotal];
  // read with the other inputs, before any store: one round trip for all of them
  const int every = hi[kHEmaEvery], ema_warm = hi[kHEmaWarm];
  const float ema_decay = hyper[kHEmaDecay];
  double lr = base;
  if (hi[kHKind] == 1) {
    if (t <= warm) lr = base * (double)t / (double)warm;
    else if (t >= total) lr = lmin;
    else lr = lmin + 0.5 * (base - lmin) *
                  (1.0 + cos(3.14159265358979323846 * (double)(t - warm) / (double)(total - warm)));
  }
  const double b1 = 1.0 - (double)hyper[kHOmb1], b2 = 1.0 - (double)hyper[kHOmb2];
  hi[kHStep] = t;
  hyper[kHLr] = (float)lr;
  hyper[kHGscale] = gs * clip;
  hyper[kHBc1] = (float)(1.0 - pow(b1, (double)t));
  hyper[kHBc2] = (float)(1.0 - pow(b2, (double)t));
  hyper[kHNorm] = norm;
  // model EMA: every K-th step is EMA update u = t / K with decay d_u; the steps
  // between publish D = 1, O = 0, which the step kernels read as "leave e alone"
  if (every > 0) {
    const int u = t / every;
    float D = 1.f, O = 0.f;
    if (t % every == 0) {
      double d = (double)ema_decay;
      if (ema_warm) {
        const double w = (1.0 + (double)u) / (10.0 + (double)u);
        d = d < w ? d : w;
      }
      D = (float)d;
      O = (float)(1.0 - d);
    }
    hyper[kHEmaD] = D;
    hyper[kHEmaO] = O;
    hi[kHEmaU] = u;
  }
}

// SGD with lr and the gradient scale read from the hyper block (schedules and
// clipping for the SGD paths); otherwise asgd_fused_step_kernel.
// EMA: one trailing argument, the fp32 moving average of p [n]; the <false>
// instantiation has neither the argument nor a trace of it in its code.
template <bool EMA, typename... E>
__global__ void __launch_bounds__(256) asgd_fused_step_dev_kernel(
    const float4* __restrict__ g, float4* __restrict__ p, float4* __restrict__ acc,
    float4* __restrict__ mom, bf16x4* __restrict__ w16, long long n4,
    const float* __restrict__ hyper, float weight_decay, float momentum, float dampening,
    int nesterov, E... ema) {
  static_assert(sizeof...(E) == (EMA ? 1 : 0), "EMA: exactly one float4* ema");
  const float lr = hyper_load(hyper, kHLr);
  const float gscale = hyper_load(hyper, kHGscale);
  const long long stride = (long long)gridDim.x * blockDim.x;
  if constexpr (EMA) {
    const float D = hyper_load(hyper, kHEmaD), O = hyper_load(hyper, kHEmaO);
    asgd_fused_step_body<true, true>(g, p, acc, mom, w16, n4, lr, gscale, weight_decay, momentum,
                                     dampening, nesterov,
                                     (long long)blockIdx.x * blockDim.x + threadIdx.x, stride,
                                     ema..., D, O);
  } else {
    asgd_fused_step_body<true>(g, p, acc, mom, w16, n4, lr, gscale, weight_decay, momentum,
                               dampening, nesterov,
                               (long long)blockIdx.x * blockDim.x + threadIdx.x, stride);
  }
}

// AdamW (torch.optim.AdamW's form) in one pass over the flat arena:
//   g' = gscale * g;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2
//   p  = p (1 - lr wd decay) - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//   acc += p_new - p_old   (the Downpour push carries the applied update,
//                           weight decay included)
// decay : one uint8 per 64-element arena block (every parameter starts on a
//         64-element boundary, so a float4 never straddles two blocks);
//         null = decay everything.
// Division and square root are the correctly rounded ones: the pass moves
// ~38 B per element and has the VALU time to spare.
// EMA: as asgd_fused_step_dev_kernel, 8 B per element more on an EMA step.
template <bool EMA, typename... E>
__global__ void __launch_bounds__(256) adamw_fused_step_kernel(
    const float4* __restrict__ g, float4* __restrict__ p, float4* __restrict__ acc,
    float4* __restrict__ m, float4* __restrict__ v, bf16x4* __restrict__ w16,
    const u8* __restrict__ decay, long long n4, const float* __restrict__ hyper,
    float weight_decay, float eps, E... ema) {
  static_assert(sizeof...(E) == (EMA ? 1 : 0), "EMA: exactly one float4* ema");
  float emaD = 1.f, emaO = 0.f;
  if constexpr (EMA) {
    emaD = hyper_load(hyper, kHEmaD);
    emaO = hyper_load(hyper, kHEmaO);
  }
  const float lr = hyper_load(hyper, kHLr);
  const float gscale = hyper_load(hyper, kHGscale);
  const float b1 = hyper_load(hyper, kHBeta1), b2 = hyper_load(hyper, kHBeta2);
  const float omb1 = hyper_load(hyper, kHOmb1), omb2 = hyper_load(hyper, kHOmb2);
  const float step = lr / hyper_load(hyper, kHBc1);
  const float sbc2 = sqrtf(hyper_load(hyper, kHBc2));
  // once per thread, in fp64: 1 - lr wd sits next to 1, where an fp32 product
  // would cost an ulp of p on every step
  const float keep = (float)(1.0 - (double)lr * (double)weight_decay);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 gv = g[i];
    const float4 p0 = p[i];
    float4 mv = m[i], vv = v[i];
    const float k = (!decay || decay[i >> 4]) ? keep : 1.f;
    float4 pn;
#define DMP_ADAMW_LANE(c)                                        \
    {                                                            \
      const float gs = gscale * gv.c;                            \
      mv.c = b1 * mv.c + omb1 * gs;                              \
      vv.c = b2 * vv.c + omb2 * (gs * gs);                       \
      pn.c = p0.c * k - step * (mv.c / (sqrtf(vv.c) / sbc2 + eps)); \
    }
    DMP_ADAMW_LANE(x) DMP_ADAMW_LANE(y) DMP_ADAMW_LANE(z) DMP_ADAMW_LANE(w)
#undef DMP_ADAMW_LANE
    m[i] = mv;
    v[i] = vv;
    p[i] = pn;
    if (acc) {
      float4 a = acc[i];
      a.x += pn.x - p0.x; a.y += pn.y - p0.y; a.z += pn.z - p0.z; a.w += pn.w - p0.w;
      acc[i] = a;
    }
    if (w16) store_bf16x4(w16, i, pn);
    if constexpr (EMA) {
      if (emaO != 0.f) ema_update4(ema..., i, pn, emaD, emaO);
    }
  }
}

// ---- model EMA outside the step kernels (parallel/ema.py) -------------------
// In-place exchange p <-> e with w16 = bf16(new p) in the same pass: evaluation
// on the averaged weights swaps them in and, by a second application, out again
// (bit for bit: the exchange moves values, the cast is a function of p).
__global__ void __launch_bounds__(256) arena_swap_kernel(float4* __restrict__ p,
                                                         float4* __restrict__ e,
                                                         bf16x4* __restrict__ w16, long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 pv = p[i], ev = e[i];
    p[i] = ev;
    e[i] = pv;
    if (w16) store_bf16x4(w16, i, ev);
  }
}

// The model's floating-point buffers (BatchNorm running statistics), which are
// no part of the arena: one block per row of `table`, int64 (live pointer,
// element offset into `flat`, numel).  Scalar accesses: a running-stat tensor
// promises no 16-byte multiple.  mode 0: flat = D flat + O live with D / O of
// the hyper block and the step kernels' skip; mode 1: exchange live <-> flat.
// A row that does not lie inside flat[0, flat_numel) is skipped.
__global__ void __launch_bounds__(256) ema_buffers_kernel(const long long* __restrict__ table,
                                                          float* __restrict__ flat,
                                                          long long flat_numel,
                                                          const float* __restrict__ hyper,
                                                          int mode) {
  const long long* row = table + 3 * (long long)blockIdx.x;
  float* live = reinterpret_cast<float*>(row[0]);
  const long long off = row[1], n = row[2];
  if (live == nullptr || off < 0 || n < 0 || off > flat_numel || n > flat_numel - off) return;
  float* e = flat + off;
  if (mode == 0) {
    const float D = hyper_load(hyper, kHEmaD), O = hyper_load(hyper, kHEmaO);
    if (O == 0.f) return;
    for (long long i = threadIdx.x; i < n; i += blockDim.x)
      e[i] = ema_lane(e[i], live[i], D, O);
  } else {
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
      const float a = live[i], b = e[i];
      live[i] = b;
      e[i] = a;
    }
  }
}

// Applied-count of a PS shard: the version a reply is stamped with
// (parallel/server.py, parallel/async_sharded.py; SURVEY §7.3(3) "a version
// counter is the basis for staleness-bounded pulls").  ps_count runs on the
// applying stream right after the apply kernel, so the count only moves once an
// apply has wholly landed; ps_stamp runs on the replying stream BEFORE the
// snapshot copy, so a stamp counts only applies the snapshot fully contains
// (applies still in flight on other link streams may show up in some elements,
// never in the count).  Both are agent-scope atomics: the counting and reading
// streams may run on any XCD (MI355X_MICROARCH.md "Workgroup dispatch").
__global__ void __launch_bounds__(64) ps_count_kernel(int* __restrict__ cnt, int add, int set) {
  if (threadIdx.x == 0) {
    if (set) __hip_atomic_exchange(cnt, add, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_add(cnt, add, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(64) ps_stamp_kernel(int* __restrict__ cnt,
                                                      float* __restrict__ dst) {
  if (threadIdx.x == 0) {
    const int v = __hip_atomic_fetch_add(cnt, 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    dst[0] = (float)v;
  }
}

// Staleness factor of ONE apply (policy "damp").  Runs on the applying stream
// immediately before the apply kernel: reads the applied count (agent-scope
// acquire, as ps_stamp does), forms tau = max(0, count - base) where `base` is
// the version the pushed delta was computed from (its header), and publishes
//   f(tau) = 1 for tau <= bound,  1 / (1 + tau - bound) above
// as {factor, tau} in the stream's own 2-float slot: the next apply on the same
// stream is ordered behind this one, so one slot per stream is enough.  One
// factor per apply, complete before the apply starts, on purpose: blocks of the
// apply never read the counter themselves (it can move mid-kernel, which would
// scale different elements differently) and no block waits for another.
// tau is the staleness when THIS kernel ran: a lower bound on the staleness
// when the apply lands (other streams' applies may land in between), the same
// lower-bound semantics as the reply stamps.  `cap` is the host's enqueue count
// when the push's header was handled: the count is clamped to it, so tau never
// exceeds the staleness the host logged for the same push.  A faster link's
// LATER pushes may have landed by now (completion-ordered applies); the server
// ordered them behind this push and they do not count against it.
// log (int32, kStaleLogHead + 2 * kStaleLogRing): [0] applies seen, [1] max tau,
// [2] damped applies (tau > bound), then a wrapping ring of (tau, factor bits)
// indexed by the apply's number.  All agent-scope atomics: factor kernels of
// different link streams run concurrently on any XCD; the host reads the log
// after a sync (stats, tests).
constexpr int kStaleLogHead = 4;
constexpr int kStaleLogRing = 1024;

__global__ void __launch_bounds__(64) ps_stale_factor_kernel(int* __restrict__ cnt, int base,
                                                             int bound, int cap,
                                                             float* __restrict__ slot,
                                                             int* __restrict__ log) {
  if (threadIdx.x == 0) {
    int v = __hip_atomic_fetch_add(cnt, 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    v = v < cap ? v : cap;
    const int tau = v > base ? v - base : 0;
    const float f = tau <= bound ? 1.f : 1.f / (float)(1 + tau - bound);
    __hip_atomic_store(slot, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(slot + 1, (float)tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int idx = __hip_atomic_fetch_add(log, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(log + 1, tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tau > bound)
      __hip_atomic_fetch_add(log + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int* e = log + kStaleLogHead + 2 * (int)((unsigned)idx % (unsigned)kStaleLogRing);
    __hip_atomic_store(e, tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(e + 1, __float_as_int(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Push hand-off: out = acc (fp32 or bf16 wire), acc = 0. One pass replaces the
// reference's "send(acc); acc.zero_()" (Asynchronous.py:58-60) and makes the
// send buffer a private snapshot so the next step may keep accumulating.
__global__ void __launch_bounds__(256) push_handoff_kernel(
    float4* __restrict__ acc, float4* __restrict__ out32, bf16x4* __restrict__ out16,
    long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 a = acc[i];
    if (out32) out32[i] = a;
    if (out16) store_bf16x4(out16, i, a);
    acc[i] = z;
  }
}

// ---- block-scaled 8-bit push wire (OCP MXFP8; specification: parallel/wire8.py)
// Payload of n elements: n E4M3 code bytes, then (at the next multiple of 16)
// ceil(n / 32) E8M0 scale bytes, the total padded to a multiple of 4.  The one
// host-side definition; -1 for a length the kernels do not take.
long long mx8_layout(long long n, long long* scales_off) {
  if (n < 0 || n > (1LL << 40)) return -1;
  const long long so = (n + 15) / 16 * 16;
  if (scales_off) *scales_off = so;
  return (so + (n + 31) / 32 + 3) / 4 * 4;
}

// gfx950's FP8 conversions are the OCP ones (e4m3fn), round to nearest even.
// Two floats -> two code bytes in the low half of the result.
__device__ __forceinline__ u32 mx8_encode2(float a, float b, int down) {
  a = fminf(fmaxf(ldexpf(a, down), -448.f), 448.f);
  b = fminf(fmaxf(ldexpf(b, down), -448.f), 448.f);
  return (u32)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

// code byte `sel` of `codes` times 2^up; NaN for a block sent as E8M0 NaN
__device__ __forceinline__ float mx8_decode(u32 codes, int sel, int up, bool nan) {
  float f;
  switch (sel) {
    case 0: f = __builtin_amdgcn_cvt_f32_fp8((int)codes, 0); break;
    case 1: f = __builtin_amdgcn_cvt_f32_fp8((int)codes, 1); break;
    case 2: f = __builtin_amdgcn_cvt_f32_fp8((int)codes, 2); break;
    default: f = __builtin_amdgcn_cvt_f32_fp8((int)codes, 3); break;
  }
  return nan ? __uint_as_float(0x7fc00000u) : ldexpf(f, up);
}

// s + scale * d with the product and the sum rounded separately (contraction
// off for this statement): the same value as the atomic form and as the fp32
// expression of the CPU path.  A fused multiply-add rounds once, and against a
// twice-rounded reference that is many ulps of a result that cancels.
__device__ __forceinline__ float mx8_axpy(float s, float scale, float d) {
#pragma clang fp contract(off)
  const float p = scale * d;
  return s + p;
}

// (f32x4, the native vector type: the hand-off's 16-B loads and stores stay whole)
__device__ __forceinline__ u32 mx8_mag(f32x4 v) {
  const u32 a = __float_as_uint(v[0]) & 0x7fffffffu, b = __float_as_uint(v[1]) & 0x7fffffffu;
  const u32 c = __float_as_uint(v[2]) & 0x7fffffffu, d = __float_as_uint(v[3]) & 0x7fffffffu;
  return max(max(a, b), max(c, d));
}

// Four elements: codes into one dword, v <- residual (x - dequant, exact in fp32)
__device__ __forceinline__ u32 mx8_quant4(f32x4& v, int down) {
  const u32 lo = mx8_encode2(v[0], v[1], down), hi = mx8_encode2(v[2], v[3], down);
  const u32 c = lo | (hi << 16);
  v[0] -= mx8_decode(c, 0, -down, false); v[1] -= mx8_decode(c, 1, -down, false);
  v[2] -= mx8_decode(c, 2, -down, false); v[3] -= mx8_decode(c, 3, -down, false);
  return c;
}

// Push hand-off on the MX8 wire: payload = quantise(acc), acc = residual, one
// pass (the residual is the error feedback: the next push carries it).
// A lane owns one float4 (16-B load and store, 4 code bytes as one dword: every
// wave-instruction is contiguous), 8 lanes own a block of 32: the block amax
// is three cross-lane DPP steps on the magnitude bits (unsigned order =
// magnitude order, and an exponent field of 255 marks a non-finite block) --
// no LDS, no atomics.  The loop bound is the block's first float4, so all
// eight lanes of a block are active for the cross-lane steps; a lane past the
// end (n % 32 != 0) counts as zeros and stores nothing.
__global__ void __launch_bounds__(256) push_handoff_mx8_kernel(
    f32x4* __restrict__ acc, u8* __restrict__ payload, long long n4, long long scales_off) {
  const long long stride = (long long)gridDim.x * blockDim.x;     // a multiple of 8
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  u32* __restrict__ codes = reinterpret_cast<u32*>(payload);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; (i & ~7LL) < n4;
       i += stride) {
    const bool v = i < n4;
    f32x4 a = z;
    if (v) a = acc[i];
    u32 m = mx8_mag(a);
    // lane ^ 1 and lane ^ 2 (quad permutes [1,0,3,2], [2,3,0,1]), then the other
    // quad of the 8 (row_half_mirror: lane i <-> 7 - i, both hold their quad's max)
    m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true));
    m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true));
    m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, true));
    const int e = (int)(m >> 23);
    const bool bad = e == 255;
    const int sb = bad ? 255 : max(e - 8, 0);       // e <= 254: never above 246
    u32 c = 0;
    if (bad) a = z;
    else c = mx8_quant4(a, 127 - sb);
    if (v) {
      codes[i] = c;
      acc[i] = a;
      if ((i & 7) == 0) payload[scales_off + (i >> 3)] = (u8)sb;
    }
  }
}

// ---- wire readers: how a payload on the wire becomes fp32 ----------------------
// One per format.  A reader knows
//   load4(i)  float4 item i, the plain 16-B-per-lane shape;
//   load1(i)  element i, the atomic one-element-per-lane shape;
//   axpy      how s + scale * d is formed in the plain apply.  This is where the
//             bit-for-bit claims of a wire live.  fp32 and bf16: the plain
//             expression, which the compiler contracts into one fused
//             multiply-add (one rounding).  MX8: mx8_axpy, contraction off, the
//             product and the sum rounded separately -- the value the atomic
//             form and the CPU path (parallel/wire8.py) give.
// The atomic apply rounds scale * d on its own and adds it in memory: two
// roundings on every wire.
struct WireF32 {
  const float* __restrict__ p;
  __device__ __forceinline__ float4 load4(long long i) const {
    return reinterpret_cast<const float4*>(p)[i];
  }
  __device__ __forceinline__ float load1(long long i) const { return p[i]; }
  static __device__ __forceinline__ float axpy(float s, float scale, float d) {
    return s + scale * d;
  }
};

struct WireBF16 {
  const u16* __restrict__ p;
  __device__ __forceinline__ float4 load4(long long i) const {
    const bf16x4 d = reinterpret_cast<const bf16x4*>(p)[i];
    return make_float4(bf2f(d.v[0]), bf2f(d.v[1]), bf2f(d.v[2]), bf2f(d.v[3]));
  }
  __device__ __forceinline__ float load1(long long i) const { return bf2f(p[i]); }
  static __device__ __forceinline__ float axpy(float s, float scale, float d) {
    return s + scale * d;
  }
};

// 4 code bytes as one dword and the block's scale byte (8 float4 items, 32
// elements per block)
struct WireMX8 {
  const u8* __restrict__ p;
  long long scales_off;
  __device__ __forceinline__ float4 load4(long long i) const {
    const u32 c = reinterpret_cast<const u32*>(p)[i];
    const int sb = p[scales_off + (i >> 3)];
    const bool nan = sb == 255;
    return make_float4(mx8_decode(c, 0, sb - 127, nan), mx8_decode(c, 1, sb - 127, nan),
                       mx8_decode(c, 2, sb - 127, nan), mx8_decode(c, 3, sb - 127, nan));
  }
  __device__ __forceinline__ float load1(long long i) const {
    const int sb = p[scales_off + (i >> 5)];
    return mx8_decode(p[i], 0, sb - 127, sb == 255);
  }
  static __device__ __forceinline__ float axpy(float s, float scale, float d) {
    return mx8_axpy(s, scale, d);
  }
};

// Staleness damping (parallel/staleness.py, policy "damp"): an apply may take a
// pointer to ONE fp32 factor that ps_stale_factor_kernel (above) published on
// the same stream before this kernel started.  Every thread loads it once (an
// agent-scope load: served by L2, the same word for the whole grid) and uses
// scale * factor; a null pointer is the undamped apply.
__device__ __forceinline__ float ps_scale(float scale, const float* factor) {
  return factor ? scale * __hip_atomic_load(factor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : scale;
}

// shard += scale * delta      -- PS GradientUpdate apply
// optional: mirror the new shard into bf16 for low-precision pulls.
template <typename W>
__global__ void __launch_bounds__(256) ps_apply_kernel(float4* __restrict__ shard, const W delta,
                                                       bf16x4* __restrict__ mirror, long long n4,
                                                       float scale, const float* factor) {
  scale = ps_scale(scale, factor);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 s = shard[i];
    const float4 d = delta.load4(i);
    s.x = W::axpy(s.x, scale, d.x); s.y = W::axpy(s.y, scale, d.y);
    s.z = W::axpy(s.z, scale, d.z); s.w = W::axpy(s.w, scale, d.w);
    shard[i] = s;
    if (mirror) store_bf16x4(mirror, i, s);
  }
}

// shard += scale * delta with fp32 global atomics (no-return
// global_atomic_add_f32): the completion-ordered PS applies each worker's delta
// on that worker's own link stream, so applies of different workers may run at
// the same time on one shard ("or use fp32 atomics").  Lane i
// of a wave adds element base + i: every wave-instruction covers 256 contiguous
// bytes, the full-rate shape of MI355X_MICROARCH.md §Global float atomics.
template <typename W>
__global__ void __launch_bounds__(256) ps_apply_atomic_kernel(float* __restrict__ shard,
                                                              const W delta, long long n,
                                                              float scale, const float* factor) {
  scale = ps_scale(scale, factor);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    unsafeAtomicAdd(shard + i, scale * delta.load1(i));
}

// ---- delay compensation (DC-ASGD; specification: parallel/wire.py dc_delta) ----
// The PS keeps `bak`, the parameters it last sent the pushing worker, and
// corrects the delta to first order for how far the shard has moved since:
//   e = d - c * d*d * (s - bak),   s' = s + sc * e
// Seven fp32 operations, each rounded on its own, in this order (contraction
// off, as in mx8_axpy): the torch expressions of the CPU path give the same
// bits on every wire.  dc_term is sc * e, what the atomic form adds in memory.
__device__ __forceinline__ float dc_term(float s, float d, float b, float c, float sc) {
#pragma clang fp contract(off)
  const float t = s - b;
  const float q = d * d;
  const float r = q * t;
  const float u = c * r;
  const float e = d - u;
  return sc * e;
}

__device__ __forceinline__ float dc_axpy(float s, float d, float b, float c, float sc) {
#pragma clang fp contract(off)
  const float p = dc_term(s, d, b, c, sc);
  return s + p;
}

// shard += scale * e(delta, shard, bak): the plain apply with a third stream
// (16 B per parameter on the fp32 wire against 12), same launch shape.
template <typename W>
__global__ void __launch_bounds__(256) ps_apply_dc_kernel(
    float4* __restrict__ shard, const W delta, const float4* __restrict__ bak,
    bf16x4* __restrict__ mirror, long long n4, float scale, float c, const float* factor) {
  scale = ps_scale(scale, factor);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 s = shard[i];
    const float4 b = bak[i];
    const float4 d = delta.load4(i);
    s.x = dc_axpy(s.x, d.x, b.x, c, scale); s.y = dc_axpy(s.y, d.y, b.y, c, scale);
    s.z = dc_axpy(s.z, d.z, b.z, c, scale); s.w = dc_axpy(s.w, d.w, b.w, c, scale);
    shard[i] = s;
    if (mirror) store_bf16x4(mirror, i, s);
  }
}

// The atomic form (the shape of ps_apply_atomic_kernel): shard[i] is read with a
// plain load for s - bak, then scale * e is added in memory.  An apply running
// on another link stream at the same time may or may not show in that load:
// the correction is first order in s - bak either way, and no add is lost.
template <typename W>
__global__ void __launch_bounds__(256) ps_apply_dc_atomic_kernel(
    float* __restrict__ shard, const W delta, const float* __restrict__ bak, long long n,
    float scale, float c, const float* factor) {
  scale = ps_scale(scale, factor);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    unsafeAtomicAdd(shard + i, dc_term(shard[i], delta.load1(i), bak[i], c, scale));
}

// ---- sparse block top-k push wire (specification: parallel/wire_topk.py) --------
// Payload of n elements at K: ceil(n / 256) * K int32 words, K slots per block
// of 256 elements; a word is (bf16 bits << 16) | offset in the block.  The one
// host-side definition; -1 for a K or a length the kernels do not take (the
// applies divide a 32-bit word index by K).
long long topk_words(long long n, int k) {
  if (k < 1 || k > kTopkMaxK || n < 0 || n > (1LL << 33)) return -1;
  return (n + kTopkBlock - 1) / kTopkBlock * k;
}

// torch's fp32 -> bf16 on the bits (round to nearest even as integer arithmetic,
// every NaN to 0x7fc0): no dependence on the conversion instruction's NaN
// payload or denormal handling.  Only a round's one winning lane runs it.
__device__ __forceinline__ u32 topk_bf16(u32 bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16;
}

// max over the wave of a per-lane value, wave-uniform: xor 1, xor 2 inside the
// quad, row_half_mirror and row_mirror give every lane its row's max (16
// lanes), then one lane of each row is read.  All 64 lanes must be active.
__device__ __forceinline__ u32 topk_wave_max(u32 m) {
  m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, true));
  m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, true));
  m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, true));
  m = max(m, (u32)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, true));
  const u32 a = (u32)__builtin_amdgcn_readlane((int)m, 0), b = (u32)__builtin_amdgcn_readlane((int)m, 16);
  const u32 c = (u32)__builtin_amdgcn_readlane((int)m, 32), d = (u32)__builtin_amdgcn_readlane((int)m, 48);
  return max(max(a, b), max(c, d));
}

// Push hand-off on the top-k wire: payload = sparsify(acc), acc = residual, one
// pass.  One wave owns one block of 256: lane l holds the float4 at block * 64
// + l (a 16-B load per lane, contiguous across the wave), so element offset
// idx = 4 * lane + component.  The wave loops over blocks with a wave-uniform
// bound: all 64 lanes are active in every cross-lane step; a lane past the end
// holds zeros (never selected) and stores nothing.
// One round: every lane offers the largest magnitude key among its components
// not yet taken, the wave takes the max, __ballot finds the lanes that hold it,
// the lowest such lane and in it the lowest such component win (the lowest
// index).  The winner writes slot r, replaces its component with the residual
// and marks it in its 4-bit `taken` mask, which also zeroes the component's key:
// a residual is non-zero and would otherwise be selected again.  No LDS, no
// atomics.  A block stops when the wave max is 0 and zero-fills the remaining
// slots.  Only lanes that took something store their float4 back: the pass
// reads 4 B per parameter and writes next to nothing.
__global__ void __launch_bounds__(256) push_handoff_topk_kernel(
    f32x4* __restrict__ acc, u32* __restrict__ payload, long long n4, long long nblk, int k) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long nwaves = (long long)gridDim.x * 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += nwaves) {
    const long long i = b * 64 + lane;
    const bool v = i < n4;
    f32x4 a = z;
    if (v) a = acc[i];
    u32 k0 = __float_as_uint(a[0]) & 0x7fffffffu, k1 = __float_as_uint(a[1]) & 0x7fffffffu;
    u32 k2 = __float_as_uint(a[2]) & 0x7fffffffu, k3 = __float_as_uint(a[3]) & 0x7fffffffu;
    u32 m = max(max(k0, k1), max(k2, k3));
    u32 taken = 0;
    u32* __restrict__ out = payload + b * k;
    int r = 0;
    for (; r < k; ++r) {
      const u32 top = topk_wave_max(m);
      if (top == 0) break;                                  // wave-uniform
      const unsigned long long holders = __ballot(m == top);
      if (lane == __ffsll((long long)holders) - 1) {
        const int c = k0 == top ? 0 : k1 == top ? 1 : k2 == top ? 2 : 3;
        const float x = c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3];
        const u32 h = topk_bf16(__float_as_uint(x));
        out[r] = (h << 16) | (u32)(4 * lane + c);
        const float left = top >= 0x7f800000u ? 0.f : x - __uint_as_float(h << 16);
        if (c == 0) { a[0] = left; k0 = 0; }
        else if (c == 1) { a[1] = left; k1 = 0; }
        else if (c == 2) { a[2] = left; k2 = 0; }
        else { a[3] = left; k3 = 0; }
        taken |= 1u << c;
        m = max(max(k0, k1), max(k2, k3));
      }
    }
    if (lane >= r && lane < k) out[lane] = 0;               // empty slots (k <= 32 lanes)
    if (taken) acc[i] = a;                                  // taken: a real element, i < n4
  }
}

// Sparse applies: one thread per payload word, shard[block * 256 + idx] +=
// scale * value, in the forms the dense wires have (plain with an optional bf16
// mirror store of the touched elements, fp32-atomic, either with the damping
// factor, either delay-compensated against bak[addr]).  A scatter, not a fourth
// wire reader.  Every form skips a word whose value is +-0 (an empty slot, or a
// value that rounded to zero) and a word whose address is >= n (a malformed
// payload must not write outside the shard).  The plain form rounds scale * v
// and the sum separately (mx8_axpy, dc_axpy): plain, atomic and the CPU
// expression give the same bits.  Addresses within one well-formed payload are
// distinct, so the plain form needs no atomics; a payload with duplicate
// addresses is malformed and is defined only for the atomic form.
template <bool ATOMIC, bool DC>
__global__ void __launch_bounds__(256) ps_apply_topk_kernel(
    float* __restrict__ shard, const u32* __restrict__ payload, const float* __restrict__ bak,
    u16* __restrict__ mirror, u32 nwords, long long n, u32 k, float scale, float c,
    const float* factor) {
  scale = ps_scale(scale, factor);
  const u32 stride = gridDim.x * blockDim.x;                // nwords <= 2^30: no wrap below
  for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += stride) {
    const u32 w = payload[j];
    if ((w & 0x7fff0000u) == 0) continue;
    const long long at = (long long)(j / k) * kTopkBlock + (w & 0xffu);
    if (at >= n) continue;
    const float d = __uint_as_float(w & 0xffff0000u);
    if constexpr (ATOMIC) {
      if constexpr (DC) unsafeAtomicAdd(shard + at, dc_term(shard[at], d, bak[at], c, scale));
      else unsafeAtomicAdd(shard + at, scale * d);
    } else {
      float s = shard[at];
      if constexpr (DC) s = dc_axpy(s, d, bak[at], c, scale);
      else s = mx8_axpy(s, scale, d);
      shard[at] = s;
      if (mirror) mirror[at] = f2bf(s);
    }
  }
}

// Reply snapshot: ONE read of the shard feeds the fp32 payload, the bf16
// payload and the worker's backup (any of them null), so the backup is the very
// values that were sent even while other link streams add to the shard.
__global__ void __launch_bounds__(256) ps_snapshot_kernel(
    const float4* __restrict__ shard, float4* __restrict__ out32, bf16x4* __restrict__ out16,
    float4* __restrict__ bak, long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 s = shard[i];
    if (out32) out32[i] = s;
    if (out16) store_bf16x4(out16, i, s);
    if (bak) bak[i] = s;
  }
}

// Pull landing: p = src (fp32 or bf16 wire), w16 = bf16(p). Optionally the
// delta the worker accumulated since the snapshot is re-applied on top
// (keep_local: p = src + acc), which keeps not-yet-pushed local progress
// instead of discarding it (the reference overwrote it).
template <typename W>
__global__ void __launch_bounds__(256) pull_land_kernel(float4* __restrict__ p, const W src,
                                                        const float4* __restrict__ acc,
                                                        bf16x4* __restrict__ w16, long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = src.load4(i);
    if (acc) {
      const float4 a = acc[i];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
    p[i] = v;
    if (w16) store_bf16x4(w16, i, v);
  }
}

// fp32 -> bf16 cast (flat), used to initialise the compute shadow.
__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(
    const float4* __restrict__ src, bf16x4* __restrict__ dst, long long n4) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    store_bf16x4(dst, i, src[i]);
  }
}

// Sum of squares of a flat fp32 buffer (grad-norm / divergence watchdog).
// Writes one partial per block; the host side sums <=2048 partials.
__global__ void __launch_bounds__(256) sumsq_partial_kernel(
    const float4* __restrict__ x, float* __restrict__ partial, long long n4) {
  __shared__ float red[4];
  float s = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 a = x[i];
    s += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Zero fill of a dense buffer, 16 B per lane (the grad arena at every step
// start).  A kernel, not hipMemsetAsync: a memset node captured into the step's
// hipGraph was NOT ordered behind the previous replay's kernels on this stack
// (ROCm 7.x): back-to-back replays without a host sync zeroed the arena while
// the previous step's weight-gradient atomics / fused update still used it, and
// training went non-finite within tens of steps (scripts/nan_hunt.py A/B:
// 3 of 3 memset runs diverged at least once, 0 of 6 with a kernel).
__global__ void __launch_bounds__(256) zero_fill_kernel(float4* __restrict__ x, long long n4,
                                                         float* __restrict__ tail, int ntail) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float4 z = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) x[i] = z;
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0.f;
}

// ---------------------------------------------------------------- launchers
void launch_zero_fill(void* p, long long bytes, hipStream_t s) {
  // bytes % 4 == 0 and 16-B aligned base (torch allocations); the < 16-B tail
  // is handled by block 0
  const long long n4 = bytes / 16;
  const int ntail = (int)((bytes - n4 * 16) / 4);
  hipLaunchKernelGGL(zero_fill_kernel, dim3(stream_grid(n4 > 0 ? n4 : 1, 256)), dim3(256), 0, s,
                     (float4*)p, n4, (float*)p + n4 * 4, ntail);
}

void launch_asgd_fused_step(const float* g, float* p, float* acc, float* mom, u16* w16,
                            long long n, float lr, float wd, float momentum, float dampening,
                            bool nesterov, hipStream_t s) {
  const long long n4 = n / 4;
  hipLaunchKernelGGL(asgd_fused_step_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                     (const float4*)g, (float4*)p, (float4*)acc, (float4*)mom, (bf16x4*)w16, n4,
                     lr, wd, momentum, dampening, nesterov ? 1 : 0);
}

int launch_sumsq_partial(const float* x, float* partial, long long n, hipStream_t s);

int optim_hyper_words() { return kHyperWords; }

// `partial` non-null: clipping on -- the norm pass over g, then the hyper kernel
// reduces its partials; null: no norm launch (gscale = grad_scale exactly)
void launch_optim_hyper(float* hyper, const float* g, float* partial, long long n, hipStream_t s) {
  int nparts = 0;
  if (partial) nparts = launch_sumsq_partial(g, partial, n, s);
  hipLaunchKernelGGL(optim_hyper_kernel, dim3(1), dim3(256), 0, s, hyper, partial, nparts);
}

void launch_asgd_fused_step_dev(const float* g, float* p, float* acc, float* mom, u16* w16,
                                long long n, const float* hyper, float wd, float momentum,
                                float dampening, bool nesterov, hipStream_t s, float* ema) {
  const long long n4 = n / 4;
  const dim3 grid(stream_grid(n4, 256));
  if (ema)
    hipLaunchKernelGGL((asgd_fused_step_dev_kernel<true, float4*>), grid, dim3(256), 0, s,
                       (const float4*)g, (float4*)p, (float4*)acc, (float4*)mom, (bf16x4*)w16, n4,
                       hyper, wd, momentum, dampening, nesterov ? 1 : 0, (float4*)ema);
  else
    hipLaunchKernelGGL(asgd_fused_step_dev_kernel<false>, grid, dim3(256), 0, s,
                       (const float4*)g, (float4*)p, (float4*)acc, (float4*)mom, (bf16x4*)w16, n4,
                       hyper, wd, momentum, dampening, nesterov ? 1 : 0);
}

void launch_adamw_fused_step(const float* g, float* p, float* acc, float* m, float* v, u16* w16,
                             const u8* decay, long long n, const float* hyper, float wd,
                             float eps, hipStream_t s, float* ema) {
  const long long n4 = n / 4;
  const dim3 grid(stream_grid(n4, 256));
  if (ema)
    hipLaunchKernelGGL((adamw_fused_step_kernel<true, float4*>), grid, dim3(256), 0, s,
                       (const float4*)g, (float4*)p, (float4*)acc, (float4*)m, (float4*)v,
                       (bf16x4*)w16, decay, n4, hyper, wd, eps, (float4*)ema);
  else
    hipLaunchKernelGGL(adamw_fused_step_kernel<false>, grid, dim3(256), 0, s,
                       (const float4*)g, (float4*)p, (float4*)acc, (float4*)m, (float4*)v,
                       (bf16x4*)w16, decay, n4, hyper, wd, eps);
}

void launch_arena_swap(float* p, float* e, u16* w16, long long n, hipStream_t s) {
  if (n <= 0) return;
  const long long n4 = n / 4;
  hipLaunchKernelGGL(arena_swap_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s, (float4*)p,
                     (float4*)e, (bf16x4*)w16, n4);
}

void launch_ema_buffers(const long long* table, int rows, float* flat, long long flat_numel,
                        const float* hyper, int mode, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(ema_buffers_kernel, dim3(rows), dim3(256), 0, s, table, flat, flat_numel,
                     hyper, mode);
}

// One launch shape per form: the plain apply takes 16 B per lane (stream_grid),
// the atomic one an element per lane on at most 4096 blocks.
template <typename W>
static void ps_apply_as(float* shard, W delta, u16* mirror, long long n, float scale, bool atomic,
                        hipStream_t s, const float* factor) {
  if (atomic) {
    const int grid = (int)std::min<long long>((n + 255) / 256, 256LL * 16);
    hipLaunchKernelGGL(ps_apply_atomic_kernel<W>, dim3(grid), dim3(256), 0, s, shard, delta, n,
                       scale, factor);
  } else {
    const long long n4 = n / 4;
    hipLaunchKernelGGL(ps_apply_kernel<W>, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                       (float4*)shard, delta, (bf16x4*)mirror, n4, scale, factor);
  }
}

void launch_ps_apply(float* shard, Wire delta, u16* mirror, long long n, float scale, bool atomic,
                     hipStream_t s, const float* factor) {
  // an empty shard: nothing to add (a 0-block grid is invalid; MX8 has no layout)
  if (n <= 0 && (atomic || delta.kind == Wire::kMX8)) return;
  long long so = 0;
  switch (delta.kind) {
    case Wire::kF32:
      return ps_apply_as(shard, WireF32{(const float*)delta.data}, mirror, n, scale, atomic, s,
                         factor);
    case Wire::kBF16:
      return ps_apply_as(shard, WireBF16{(const u16*)delta.data}, mirror, n, scale, atomic, s,
                         factor);
    case Wire::kMX8:
      mx8_layout(n, &so);
      return ps_apply_as(shard, WireMX8{(const u8*)delta.data, so}, mirror, n, scale, atomic, s,
                         factor);
  }
}

// The launch shapes of ps_apply_as, with the backup as third operand.
template <typename W>
static void ps_apply_dc_as(float* shard, W delta, const float* bak, u16* mirror, long long n,
                           float scale, float c, bool atomic, hipStream_t s,
                           const float* factor) {
  if (atomic) {
    const int grid = (int)std::min<long long>((n + 255) / 256, 256LL * 16);
    hipLaunchKernelGGL(ps_apply_dc_atomic_kernel<W>, dim3(grid), dim3(256), 0, s, shard, delta,
                       bak, n, scale, c, factor);
  } else {
    const long long n4 = n / 4;
    hipLaunchKernelGGL(ps_apply_dc_kernel<W>, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                       (float4*)shard, delta, (const float4*)bak, (bf16x4*)mirror, n4, scale, c,
                       factor);
  }
}

void launch_ps_apply_dc(float* shard, Wire delta, const float* bak, u16* mirror, long long n,
                        float scale, float c, bool atomic, hipStream_t s, const float* factor) {
  if (n <= 0) return;
  long long so = 0;
  switch (delta.kind) {
    case Wire::kF32:
      return ps_apply_dc_as(shard, WireF32{(const float*)delta.data}, bak, mirror, n, scale, c,
                            atomic, s, factor);
    case Wire::kBF16:
      return ps_apply_dc_as(shard, WireBF16{(const u16*)delta.data}, bak, mirror, n, scale, c,
                            atomic, s, factor);
    case Wire::kMX8:
      mx8_layout(n, &so);
      return ps_apply_dc_as(shard, WireMX8{(const u8*)delta.data, so}, bak, mirror, n, scale, c,
                            atomic, s, factor);
  }
}

void launch_ps_snapshot(const float* shard, float* out32, u16* out16, float* bak, long long n,
                        hipStream_t s) {
  if (n <= 0) return;
  const long long n4 = n / 4;
  hipLaunchKernelGGL(ps_snapshot_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                     (const float4*)shard, (float4*)out32, (bf16x4*)out16, (float4*)bak, n4);
}

void launch_ps_count(int* cnt, int add, bool set, hipStream_t s) {
  hipLaunchKernelGGL(ps_count_kernel, dim3(1), dim3(64), 0, s, cnt, add, set ? 1 : 0);
}

void launch_ps_stamp(int* cnt, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(ps_stamp_kernel, dim3(1), dim3(64), 0, s, cnt, dst);
}

int stale_log_numel() { return kStaleLogHead + 2 * kStaleLogRing; }

void launch_ps_stale_factor(int* cnt, int base, int bound, int cap, float* slot, int* log,
                            hipStream_t s) {
  hipLaunchKernelGGL(ps_stale_factor_kernel, dim3(1), dim3(64), 0, s, cnt, base, bound, cap,
                     slot, log);
}

// src: fp32 or bf16 (parameters never travel as MX8)
void launch_pull_land(float* p, Wire src, const float* acc, u16* w16, long long n, hipStream_t s) {
  const long long n4 = n / 4;
  const dim3 grid(stream_grid(n4, 256));
  if (src.kind == Wire::kF32)
    hipLaunchKernelGGL(pull_land_kernel<WireF32>, grid, dim3(256), 0, s, (float4*)p,
                       WireF32{(const float*)src.data}, (const float4*)acc, (bf16x4*)w16, n4);
  else
    hipLaunchKernelGGL(pull_land_kernel<WireBF16>, grid, dim3(256), 0, s, (float4*)p,
                       WireBF16{(const u16*)src.data}, (const float4*)acc, (bf16x4*)w16, n4);
}

void launch_push_handoff(float* acc, float* out32, u16* out16, long long n, hipStream_t s) {
  const long long n4 = n / 4;
  hipLaunchKernelGGL(push_handoff_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                     (float4*)acc, (float4*)out32, (bf16x4*)out16, n4);
}

// payload: mx8_layout(n) bytes, 16-B aligned; n % 4 == 0 (checked by the binding)
void launch_push_handoff_mx8(float* acc, u8* payload, long long n, hipStream_t s) {
  if (n <= 0) return;
  long long so = 0;
  mx8_layout(n, &so);
  const long long n4 = n / 4;
  hipLaunchKernelGGL(push_handoff_mx8_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                     (f32x4*)acc, payload, n4, so);
}

// payload: topk_words(n, k) int32 words; n % 4 == 0 (both checked by the binding)
void launch_push_handoff_topk(float* acc, u32* payload, long long n, int k, hipStream_t s) {
  if (n <= 0) return;
  const long long nblk = (n + kTopkBlock - 1) / kTopkBlock;
  hipLaunchKernelGGL(push_handoff_topk_kernel, dim3(stream_grid(nblk * 64, 256)), dim3(256), 0, s,
                     (f32x4*)acc, payload, n / 4, nblk, k);
}

// bak null: the plain apply; else the delay-compensated one with coefficient c
void launch_ps_apply_topk(float* shard, const u32* payload, const float* bak, u16* mirror,
                          long long n, int k, float scale, float c, bool atomic, hipStream_t s,
                          const float* factor) {
  const long long nwords = topk_words(n, k);
  if (nwords <= 0) return;
  const dim3 grid((unsigned)std::min<long long>((nwords + 255) / 256, 256LL * 16)), block(256);
  const u32 nw = (u32)nwords, ku = (u32)k;
  if (bak) {
    if (atomic)
      hipLaunchKernelGGL((ps_apply_topk_kernel<true, true>), grid, block, 0, s, shard, payload,
                         bak, mirror, nw, n, ku, scale, c, factor);
    else
      hipLaunchKernelGGL((ps_apply_topk_kernel<false, true>), grid, block, 0, s, shard, payload,
                         bak, mirror, nw, n, ku, scale, c, factor);
  } else {
    if (atomic)
      hipLaunchKernelGGL((ps_apply_topk_kernel<true, false>), grid, block, 0, s, shard, payload,
                         bak, mirror, nw, n, ku, scale, c, factor);
    else
      hipLaunchKernelGGL((ps_apply_topk_kernel<false, false>), grid, block, 0, s, shard, payload,
                         bak, mirror, nw, n, ku, scale, c, factor);
  }
}

void launch_cast_f32_bf16(const float* src, u16* dst, long long n, hipStream_t s) {
  const long long n4 = n / 4;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s,
                     (const float4*)src, (bf16x4*)dst, n4);
}

int launch_sumsq_partial(const float* x, float* partial, long long n, hipStream_t s) {
  const long long n4 = n / 4;
  int grid = stream_grid(n4, 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, s, (const float4*)x,
                     partial, n4);
  return grid;
}

}  // namespace dmp
