// GroupNorm (+ residual) (+ ReLU) over channels-last bf16 activations [N][H*W][C]:
//   y = relu?( ((x - mean) * rstd) * gamma[c] + beta[c] [+ residual] )
// with torch's statistics (biased variance over the H*W*cpg elements of a
// (sample, group)), mean and rstd saved as fp32 [N, G], and the backward
//   dz = dy * [y > 0] (ReLU fused), dbeta[c] = sum dz, dgamma[c] = sum dz * xhat,
//   dx = rstd * (dz*gamma - mean_g(dz*gamma) - xhat * mean_g(dz*gamma*xhat)), dres = dz.
// Geometry, routes, LDS image and grids come from group_norm_plan.h; the kernels
// trust only what plan_group_norm accepted.
//
// Work split.  A workgroup owns one sample x one channel slice of SV 16-byte
// vectors (whole groups) x one pixel part.  Lane = (pixel row, vector of the
// slice): lane t reads vector t % SV of pixels t / SV, t / SV + PR, ... (PR = 256 /
// SV; when SV does not divide 256 the last 256 - PR * SV lanes only take part in
// the barriers).  A lane's channels never change, so gamma, beta, mean and rstd of
// its 8 channels sit in registers.
//
// Resident route.  A lane keeps what it loaded in LDS, at [i][lane]: consecutive
// lanes, consecutive 16-byte slots, so every ds_read / ds_write_b128 is free of
// bank conflicts, and as no lane ever reads another lane's slot the passes over
// the staged slice need no barrier.  Forward: load + sum, group mean, centred sum
// of squares from LDS, then normalise from LDS and store y once: the exact
// two-pass variance at one pass of memory traffic.  Backward: x and dz are staged
// (dz is dy or 0, so bf16 holds it exactly; y is read once for the mask and dres
// is written in that pass), one reduction, then dx from LDS.
//
// Streaming route.  Forward: a statistics launch runs the first two resident
// passes over each pixel part (a part is sized to fit LDS, so its M2 is centred
// too) and writes (count, mean, M2) per (sample, part, group); the apply launch
// merges its groups' partials in part order with Chan's formula in its prologue
// and streams x once more.  Backward: a reduce launch writes the two group sums
// per (sample, part, group), the apply launch adds them in part order.  Variance
// is never E[x^2] - mean^2 on either route.
//
// Reductions.  Lane sums are fp32 (a lane adds a few dozen values); every step
// across lanes is fp64 and in a fixed order: lanes store their 8 (or 16) sums to
// LDS, one thread per channel adds the PR pixel rows in index order, one thread
// per group adds its cpg channels.  This deviates from the DPP + cross-wave
// sketch of the design note: a group spans 1/8 of a lane (cpg 1) up to 256 lanes
// (G = 1), and columns through LDS serve all of them with one code path and one
// summation order; at 4-64 slice channels the column pass is a few hundred LDS
// reads per workgroup, far below the cost of the loads it follows.  fp64 makes
// mean and rstd correctly rounded to within an ulp whatever |mean| / sigma is.
//
// Parameter gradients.  A backward workgroup walks the samples n = z, z + NR, ...
// and keeps the running per-channel sums of its slice (fp64, LDS); at the end it
// overwrites its own row of the layer's slab [rows][2][C].  gn_param_reduce adds
// the rows in index order into the arena gradient: no atomics, nothing to zero,
// bitwise reproducible, graph-safe.  The slab's size depends on C alone.
#include "common.h"
#include "group_norm_plan.h"
#include "launchers.h"

namespace dmp {

struct GnArgs {
  const u16* x;
  const u16* res;      // forward: residual (null: none)
  u16* y;
  const float* gamma;
  const float* beta;
  float* mean;         // [N][G]
  float* rstd;
  double* part;        // streaming partials, [N][parts][G][3] forward, [..][2] backward
  const u16* dy;
  const u16* yin;      // backward: the forward's output (ReLU mask), null without ReLU
  u16* dx;
  u16* dres;           // null: not wanted
  float* slab;         // null: no parameter gradient wanted
  int N, C, CV, G, cpg, HW;
  int SV, PR, T, IT, GS, parts, PP;
  float eps;
  int relu;
};

__device__ __forceinline__ void gn_widen(const bf16x8& v, float (&f)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = bf2f(v.v[k]);
}

// Block reduction of NV x 8 lane sums to per-channel columns (chan) and per-group
// sums (grp), fp64, fixed order.  w (null: ones) weights the channels of the group
// sums; tot (null: none) accumulates the columns.  All 256 threads call it.
template <int NV>
__device__ __forceinline__ void gn_reduce(const float (&v)[NV][8], bool live, int cvl, int prow,
                                          const GnArgs& a, float* red, double* chan, double* grp,
                                          const float* w, double* tot) {
  const int SC = a.SV * 8;
  // one sum at a time through red [PR][SC]: 8 KB whatever NV is
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    if (live) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[prow * SC + cvl * 8 + k] = v[q][k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < SC; c += kGnThreads) {
      double s = 0.0;
      for (int r = 0; r < a.PR; ++r) s += (double)red[r * SC + c];
      chan[q * SC + c] = s;
      if (tot) tot[q * SC + c] += s;
    }
    __syncthreads();
  }
  for (int g = threadIdx.x; g < a.GS; g += kGnThreads) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      double s = 0.0;
      for (int c = g * a.cpg; c < (g + 1) * a.cpg; ++c)
        s += chan[q * SC + c] * (w ? (double)w[c] : 1.0);
      grp[q * a.GS + g] = s;
    }
  }
  __syncthreads();
}

// MODE 0: resident forward.  1: statistics of a pixel part (streaming).  2:
// streaming apply.
template <int MODE>
__global__ void __launch_bounds__(kGnThreads) gn_fwd_kernel(const GnArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const int tid = threadIdx.x, SC = a.SV * 8;
  const bool live = tid < a.T;
  const int cvl = tid % a.SV, prow = tid / a.SV;
  const int slice = blockIdx.x, part = blockIdx.y, n = blockIdx.z;
  const GnLds L = gn_lds(a.T, MODE == 2 ? 0 : a.IT, SC, a.GS, MODE == 2 ? 0 : 1, 1);
  bf16x8* xs = reinterpret_cast<bf16x8*>(gn_smem + L.x);
  double* chan = reinterpret_cast<double*>(gn_smem + L.chan);
  double* grp = reinterpret_cast<double*>(gn_smem + L.grp);
  float* red = reinterpret_cast<float*>(gn_smem + L.red);
  float* gstat = reinterpret_cast<float*>(gn_smem + L.gstat);

  const int p0 = part * a.PP, p1 = p0 + a.PP < a.HW ? p0 + a.PP : a.HW;
  const long long base = (long long)n * a.HW * a.CV + slice * a.SV + cvl;   // in vectors
  const bf16x8* xg = reinterpret_cast<const bf16x8*>(a.x) + base;
  const int g0 = slice * a.GS;
  int gl[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) gl[k] = (cvl * 8 + k) / a.cpg;
  float mu[8], rs[8];

  if constexpr (MODE != 2) {
    const double cnt = (double)(p1 - p0) * a.cpg;
    float s[1][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[0][k] = 0.f;
    if (live) {
      for (int i = 0, p = p0 + prow; p < p1; ++i, p += a.PR) {
        const bf16x8 v = xg[(long long)p * a.CV];
        xs[i * a.T + tid] = v;
#pragma unroll
        for (int k = 0; k < 8; ++k) s[0][k] += bf2f(v.v[k]);
      }
    }
    gn_reduce<1>(s, live, cvl, prow, a, red, chan, grp, nullptr, nullptr);
    for (int g = tid; g < a.GS; g += kGnThreads) gstat[g] = (float)(grp[g] / cnt);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      mu[k] = gstat[gl[k]];
      s[0][k] = 0.f;
    }
    if (live) {
      for (int i = 0, p = p0 + prow; p < p1; ++i, p += a.PR) {
        float f[8];
        gn_widen(xs[i * a.T + tid], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = f[k] - mu[k];
          s[0][k] += d * d;
        }
      }
    }
    gn_reduce<1>(s, live, cvl, prow, a, red, chan, grp, nullptr, nullptr);
    if constexpr (MODE == 1) {
      for (int g = tid; g < a.GS; g += kGnThreads) {
        double* o = a.part + (((long long)n * a.parts + part) * a.G + g0 + g) * 3;
        o[0] = cnt;
        o[1] = (double)gstat[g];
        o[2] = grp[g];
      }
      return;
    } else {
      for (int g = tid; g < a.GS; g += kGnThreads) {
        const float r = (float)(1.0 / sqrt(grp[g] / cnt + (double)a.eps));
        gstat[a.GS + g] = r;
        a.mean[(long long)n * a.G + g0 + g] = gstat[g];
        a.rstd[(long long)n * a.G + g0 + g] = r;
      }
    }
  } else {
    // merge the parts' (count, mean, M2) in part order (Chan et al.)
    for (int g = tid; g < a.GS; g += kGnThreads) {
      double na = 0.0, ma = 0.0, M2 = 0.0;
      for (int q = 0; q < a.parts; ++q) {
        const double* o = a.part + (((long long)n * a.parts + q) * a.G + g0 + g) * 3;
        const double nb = o[0], d = o[1] - ma, nn = na + nb;
        ma += d * nb / nn;
        M2 += o[2] + d * d * na * nb / nn;
        na = nn;
      }
      const float m = (float)ma, r = (float)(1.0 / sqrt(M2 / na + (double)a.eps));
      gstat[g] = m;
      gstat[a.GS + g] = r;
      if (part == 0) {
        a.mean[(long long)n * a.G + g0 + g] = m;
        a.rstd[(long long)n * a.G + g0 + g] = r;
      }
    }
  }
  __syncthreads();
  if (!live) return;

  float ga[8], be[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mu[k] = gstat[gl[k]];
    rs[k] = gstat[a.GS + gl[k]];
    ga[k] = a.gamma[slice * SC + cvl * 8 + k];
    be[k] = a.beta[slice * SC + cvl * 8 + k];
  }
  const bf16x8* rg = a.res ? reinterpret_cast<const bf16x8*>(a.res) + base : nullptr;
  bf16x8* yg = reinterpret_cast<bf16x8*>(a.y) + base;
  for (int i = 0, p = p0 + prow; p < p1; ++i, p += a.PR) {
#pragma clang fp contract(off)
    float f[8], r[8];
    if constexpr (MODE == 0) gn_widen(xs[i * a.T + tid], f);
    else gn_widen(xg[(long long)p * a.CV], f);
    if (rg) gn_widen(rg[(long long)p * a.CV], r);
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = ((f[k] - mu[k]) * rs[k]) * ga[k] + be[k];
      if (rg) t = t + r[k];
      if (a.relu) t = fmaxf(t, 0.f);
      o.v[k] = f2bf(t);
    }
    yg[(long long)p * a.CV] = o;
  }
}

// MODE 0: resident backward.  1: streaming reduce (group sums per part, slab row).
// 2: streaming apply.
template <int MODE>
__global__ void __launch_bounds__(kGnThreads) gn_bwd_kernel(const GnArgs a) {
  extern __shared__ __align__(16) unsigned char gn_smem[];
  const int tid = threadIdx.x, SC = a.SV * 8;
  const bool live = tid < a.T;
  const int cvl = tid % a.SV, prow = tid / a.SV;
  const int slice = blockIdx.x, part = blockIdx.y;
  const GnLds L = gn_lds(a.T, MODE == 0 ? a.IT : 0, SC, a.GS, MODE == 0 ? 2 : 0, 2);
  bf16x8* xs = reinterpret_cast<bf16x8*>(gn_smem + L.x);
  bf16x8* zs = reinterpret_cast<bf16x8*>(gn_smem + L.dz);
  double* chan = reinterpret_cast<double*>(gn_smem + L.chan);
  double* grp = reinterpret_cast<double*>(gn_smem + L.grp);
  double* tot = MODE != 2 && a.slab ? reinterpret_cast<double*>(gn_smem + L.tot) : nullptr;
  float* red = reinterpret_cast<float*>(gn_smem + L.red);
  float* gstat = reinterpret_cast<float*>(gn_smem + L.gstat);

  const int p0 = part * a.PP, p1 = p0 + a.PP < a.HW ? p0 + a.PP : a.HW;
  const int g0 = slice * a.GS;
  const double cnt = (double)a.HW * a.cpg;
  const float* gslice = a.gamma + slice * SC;
  int gl[8];
  float ga[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gl[k] = (cvl * 8 + k) / a.cpg;
    ga[k] = gslice[cvl * 8 + k];
  }
  // zeroed here, before the first reduction's barriers; from then on a column's
  // running sum is touched by the one thread that owns the column
  if (tot)
    for (int c = tid; c < 2 * SC; c += kGnThreads) tot[c] = 0.0;

  for (int n = blockIdx.z; n < a.N; n += gridDim.z) {
    const long long base = (long long)n * a.HW * a.CV + slice * a.SV + cvl;
    const bf16x8* xg = reinterpret_cast<const bf16x8*>(a.x) + base;
    const bf16x8* dyg = reinterpret_cast<const bf16x8*>(a.dy) + base;
    const bf16x8* yg = a.relu ? reinterpret_cast<const bf16x8*>(a.yin) + base : nullptr;
    bf16x8* dresg = a.dres ? reinterpret_cast<bf16x8*>(a.dres) + base : nullptr;
    bf16x8* dxg = reinterpret_cast<bf16x8*>(a.dx) + base;
    float mu[8], rs[8], am[8], bm[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      mu[k] = a.mean[(long long)n * a.G + g0 + gl[k]];
      rs[k] = a.rstd[(long long)n * a.G + g0 + gl[k]];
    }

    if constexpr (MODE != 2) {
      float s[2][8];
#pragma unroll
      for (int k = 0; k < 8; ++k) s[0][k] = s[1][k] = 0.f;
      if (live) {
        for (int i = 0, p = p0 + prow; p < p1; ++i, p += a.PR) {
          const long long v = (long long)p * a.CV;
          const bf16x8 xv = xg[v];
          bf16x8 dz = dyg[v];
          if (yg) {
            const bf16x8 yv = yg[v];
#pragma unroll
            for (int k = 0; k < 8; ++k) dz.v[k] = bf2f(yv.v[k]) > 0.f ? dz.v[k] : (u16)0;
          }
          if constexpr (MODE == 0) {
            xs[i * a.T + tid] = xv;
            zs[i * a.T + tid] = dz;
            if (dresg) dresg[v] = dz;
          }
          float xf[8], zf[8];
          gn_widen(xv, xf);
          gn_widen(dz, zf);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            s[0][k] += zf[k];
            s[1][k] += zf[k] * ((xf[k] - mu[k]) * rs[k]);
          }
        }
      }
      gn_reduce<2>(s, live, cvl, prow, a, red, chan, grp, gslice, tot);
      if constexpr (MODE == 1) {
        for (int g = tid; g < a.GS; g += kGnThreads) {
          double* o = a.part + (((long long)n * a.parts + part) * a.G + g0 + g) * 2;
          o[0] = grp[g];
          o[1] = grp[a.GS + g];
        }
        continue;
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          am[k] = (float)(grp[gl[k]] / cnt);
          bm[k] = (float)(grp[a.GS + gl[k]] / cnt);
        }
      }
    } else {
      __syncthreads();
      for (int g = tid; g < a.GS; g += kGnThreads) {
        double A = 0.0, B = 0.0;
        for (int q = 0; q < a.parts; ++q) {
          const double* o = a.part + (((long long)n * a.parts + q) * a.G + g0 + g) * 2;
          A += o[0];
          B += o[1];
        }
        gstat[g] = (float)(A / cnt);
        gstat[a.GS + g] = (float)(B / cnt);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        am[k] = gstat[gl[k]];
        bm[k] = gstat[a.GS + gl[k]];
      }
    }

    if (live) {
      for (int i = 0, p = p0 + prow; p < p1; ++i, p += a.PR) {
        const long long v = (long long)p * a.CV;
        bf16x8 xv, dz;
        if constexpr (MODE == 0) {
          xv = xs[i * a.T + tid];
          dz = zs[i * a.T + tid];
        } else {
          xv = xg[v];
          dz = dyg[v];
          if (yg) {
            const bf16x8 yv = yg[v];
#pragma unroll
            for (int k = 0; k < 8; ++k) dz.v[k] = bf2f(yv.v[k]) > 0.f ? dz.v[k] : (u16)0;
          }
          if (dresg) dresg[v] = dz;
        }
        float xf[8], zf[8];
        gn_widen(xv, xf);
        gn_widen(dz, zf);
        bf16x8 o;
        {
          // no contraction: dz * gamma must round as the group mean of a
          // one-element group did, so that a zero-variance group gives dx = 0
#pragma clang fp contract(off)
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float xh = (xf[k] - mu[k]) * rs[k];
            o.v[k] = f2bf(rs[k] * (zf[k] * ga[k] - am[k] - xh * bm[k]));
          }
        }
        dxg[v] = o;
      }
    }
  }

  if (tot) {
    // tot was last written by this thread's own columns (gn_reduce), same stride
    const long long row = (long long)blockIdx.z * a.parts + part;
    for (int c = tid; c < SC; c += kGnThreads) {
      a.slab[(row * 2 + 0) * a.C + slice * SC + c] = (float)tot[c];
      a.slab[(row * 2 + 1) * a.C + slice * SC + c] = (float)tot[SC + c];
    }
  }
}

// dbeta[c] += sum of slab rows [r][0][c], dgamma[c] += rows [r][1][c], index order
__global__ void __launch_bounds__(256) gn_param_reduce_kernel(const float* __restrict__ slab,
                                                              int rows, int C,
                                                              float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  float* out = which ? dgamma : dbeta;
  if (out == nullptr) return;
  float v = 0.f;
  for (int r = 0; r < rows; ++r) v += slab[((long long)r * 2 + which) * C + c];
  out[c] += v;
}

static GnArgs gn_args(const GnPlan& p, int N, int C, int HW, int G) {
  GnArgs a{};
  a.N = N, a.C = C, a.CV = p.CV, a.G = G, a.cpg = p.cpg, a.HW = HW;
  a.SV = p.SV, a.PR = p.PR, a.T = p.T, a.IT = p.IT, a.GS = p.GS, a.parts = p.parts, a.PP = p.PP;
  return a;
}

template <auto Kernel>
static void gn_launch(const GnArgs& a, dim3 grid, int lds, hipStream_t s) {
  allow_max_dynamic_lds<Kernel>();
  hipLaunchKernelGGL(Kernel, grid, dim3(kGnThreads), (size_t)lds, s, a);
}

void launch_gn_fwd(const GnPlan& p, const uint16_t* x, const uint16_t* res, const float* gamma,
                   const float* beta, uint16_t* y, float* mean, float* rstd, double* part, int N,
                   int C, int HW, int G, float eps, bool relu, hipStream_t s) {
  GnArgs a = gn_args(p, N, C, HW, G);
  a.x = x, a.res = res, a.y = y, a.gamma = gamma, a.beta = beta, a.mean = mean, a.rstd = rstd;
  a.part = part, a.eps = eps, a.relu = relu;
  const dim3 grid(p.grid[0], p.grid[1], N);
  if (p.route == 0) {
    gn_launch<gn_fwd_kernel<0>>(a, grid, p.lds_bytes, s);
  } else {
    gn_launch<gn_fwd_kernel<1>>(a, grid, p.lds_bytes, s);
    gn_launch<gn_fwd_kernel<2>>(a, grid, p.lds_apply, s);
  }
}

void launch_gn_bwd(const GnPlan& p, const uint16_t* x, const uint16_t* dy, const uint16_t* y,
                   const float* gamma, const float* mean, const float* rstd, uint16_t* dx,
                   uint16_t* dres, float* dgamma, float* dbeta, float* slab, double* part, int N,
                   int C, int HW, int G, bool relu, hipStream_t s) {
  GnArgs a = gn_args(p, N, C, HW, G);
  a.x = x, a.dy = dy, a.yin = relu ? y : nullptr, a.gamma = gamma;
  a.mean = const_cast<float*>(mean), a.rstd = const_cast<float*>(rstd);
  a.dx = dx, a.dres = dres, a.part = part, a.relu = relu;
  a.slab = dgamma || dbeta ? slab : nullptr;
  const dim3 grid(p.grid[0], p.grid[1], p.NR);
  if (p.route == 0) {
    gn_launch<gn_bwd_kernel<0>>(a, grid, p.lds_bytes, s);
  } else {
    gn_launch<gn_bwd_kernel<1>>(a, grid, p.lds_bytes, s);
    gn_launch<gn_bwd_kernel<2>>(a, dim3(p.grid[0], p.grid[1], N), p.lds_apply, s);
  }
  if (a.slab)
    hipLaunchKernelGGL(gn_param_reduce_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, s, slab,
                       p.slab_rows, C, dgamma, dbeta);
}

}  // namespace dmp
