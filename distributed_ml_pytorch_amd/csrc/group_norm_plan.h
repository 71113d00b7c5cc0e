// Host-side plan of the GroupNorm kernels (group_norm.hip): route, channel slice,
// pixel parts, LDS image, grids and slab rows of an (N, C, H*W, G) geometry.
// Plain C++ (no torch, no HIP) in the manner of dwconv_plan.h / attn_plan.h: the
// launchers, the bindings and group_norm_plan_check.cpp read the same function;
// the kernels trust only what it accepted.  gn_lds() alone is also compiled for
// the device, so that kernel and planner cannot disagree about the LDS image.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define DMP_GN_HD __host__ __device__
#else
#define DMP_GN_HD
#endif

namespace dmp {

constexpr int kGnThreads = 256;
constexpr int kGnVec = 8;                    // channels of a lane's 16-byte vector
constexpr int kGnMaxC = 2048;
constexpr int kGnLdsMax = 160 * 1024;        // gfx950: LDS of a CU
constexpr int kGnLdsPrefer = 80 * 1024;      // two workgroups per CU
constexpr int kGnFillWgs = 512;              // two workgroups on each of 256 CUs
constexpr int kGnStreamItems = 8;            // vectors a lane stages per pixel part
constexpr int kGnMaxParts = 64;              // most pixel parts of the streaming route
constexpr int kGnSlabFloats = 1 << 18;       // budget of a layer's dgamma / dbeta slab
constexpr int kGnMaxSlabRows = 256;
constexpr int kGnMaxBatch = 65535;           // samples ride gridDim.z

inline bool gn_cpg_ok(int cpg) {
  return cpg == 1 || cpg == 2 || cpg == 4 || (cpg > 0 && cpg % kGnVec == 0);
}

// rows [2][C] of a layer's slab: a function of C alone (64 .. 256 rows).  It must
// not grow with the batch or the map: a captured step holds the slab's address,
// and an evaluation at another batch size runs the same layer.
inline int gn_slab_rows(int C) {
  const int r = kGnSlabFloats / (2 * C);
  return r < kGnMaxSlabRows ? r : kGnMaxSlabRows;
}
inline long long gn_slab_floats(int C) { return (long long)gn_slab_rows(C) * 2 * C; }

// LDS image of a workgroup, byte offsets.  T live lanes, IT staged vectors per
// lane and tensor, SC slice channels, GS slice groups, NV sums per channel (1
// forward, 2 backward); `tensors` staged activations (0: a launch that streams).
struct GnLds {
  int x, dz;        // staged vectors [IT][T] x 16 B, lane-private
  int chan;         // column sums [NV][SC] fp64
  int grp;          // group sums [NV][GS] fp64
  int tot;          // backward: running dbeta / dgamma of the slice [2][SC] fp64
  int red;          // lane sums [PR][SC] fp32, one of the NV sums at a time
  int gstat;        // per-group pair [2][GS] fp32 (mean, rstd | the two group means)
  int bytes;
};

DMP_GN_HD inline GnLds gn_lds(int T, int IT, int SC, int GS, int tensors, int NV) {
  GnLds l{};
  int o = 0;
  l.x = o;
  o += tensors > 0 ? IT * T * 16 : 0;
  l.dz = o;
  o += tensors > 1 ? IT * T * 16 : 0;
  l.chan = o;
  o += NV * SC * 8;
  l.grp = o;
  o += NV * GS * 8;
  l.tot = o;
  o += NV > 1 ? 2 * SC * 8 : 0;
  l.red = o;
  o += T * kGnVec * 4;
  l.gstat = o;
  o += 2 * GS * 4;
  l.bytes = o;
  return l;
}

struct GnPlan {
  bool ok;
  int route;                   // 0 resident, 1 streaming
  int CV, SV, slices;          // 16-byte vectors of a pixel, of a slice; slices of C
  int cpg, GS;                 // channels per group; whole groups per slice
  int PR, T;                   // pixel rows of a workgroup (256 / SV), live lanes PR * SV
  int parts, PP, IT;           // pixel parts, pixels per part, vectors per lane and part
  int NR;                      // backward: sample rows of the grid (each walks N by NR)
  int slab_rows;               // backward: slab rows written and reduced, NR * parts
  int lds_bytes;               // the staging launch (resident, or streaming statistics)
  int lds_apply;               // the streaming apply launch
  int grid[3];                 // slices, parts, samples (forward) or NR (backward reduce)
};

namespace gn_detail {

inline void shape(GnPlan& p, int SV, long long pixels) {
  p.SV = SV;
  p.slices = p.CV / SV;
  p.GS = SV * kGnVec / p.cpg;
  p.PR = kGnThreads / SV;
  p.T = p.PR * SV;
  p.IT = (int)((pixels + p.PR - 1) / p.PR);
}

inline bool sv_ok(const GnPlan& p, int SV, int gv) { return p.CV % SV == 0 && SV % gv == 0; }

}  // namespace gn_detail

// route: -1 automatic, 0 resident, 1 streaming (a forced route that cannot be
// honoured is refused, never replaced).
//
// Resident: the slice candidates are the divisors SV of C / 8 that hold whole
// groups.  One that keeps the workgroup within kGnLdsPrefer, is at least 64 bytes
// wide per pixel (or all of C) and still gives kGnFillWgs workgroups wins, the
// widest first; then the narrowest of those that do not fill the CUs (most
// workgroups); then the widest narrow one within kGnLdsPrefer; then anything
// within the CU's LDS.  The backward stages two tensors, so the same rule lands
// on half the slice.
// Streaming: the narrowest slice of at least 64 bytes, kGnStreamItems vectors a
// lane and part; more than kGnMaxParts parts grow the part instead.
inline GnPlan plan_group_norm(long long N, int C, long long HW, int G, int route, bool backward) {
  using namespace gn_detail;
  GnPlan p{};
  if (N < 1 || N > kGnMaxBatch || C < kGnVec || C % kGnVec || C > kGnMaxC || HW < 1 ||
      HW > (1ll << 30) || G < 1 || C % G || route < -1 || route > 1)
    return p;
  p.cpg = C / G;
  if (!gn_cpg_ok(p.cpg)) return p;
  if (N * HW * C * 2 >= (1ll << 31)) return p;          // 32-bit offsets within a tensor
  p.CV = C / kGnVec;
  const int gv = p.cpg >= kGnVec ? p.cpg / kGnVec : 1;  // vectors of a group
  if (gv > kGnThreads) return p;
  const int tensors = backward ? 2 : 1, NV = backward ? 2 : 1;
  const int top = p.CV < kGnThreads ? p.CV : kGnThreads;

  int best = 0, best_cls = 0;
  if (route != 1) {
    for (int SV = top; SV >= 1; --SV) {
      if (!sv_ok(p, SV, gv)) continue;
      shape(p, SV, HW);
      if ((long long)p.IT * p.T * 16 * tensors > kGnLdsMax) continue;
      const int lds = gn_lds(p.T, p.IT, SV * kGnVec, p.GS, tensors, NV).bytes;
      if (lds > kGnLdsMax) continue;
      const bool wide = SV >= 4 || SV == p.CV, pref = lds <= kGnLdsPrefer;
      const bool fills = N * p.slices >= kGnFillWgs;
      const int cls = pref && wide ? (fills ? 5 : 4) : pref ? 3 : wide ? 2 : 1;
      if (cls > best_cls || (cls == best_cls && cls == 4)) best = SV, best_cls = cls;
    }
  }
  if (best) {
    p.route = 0;
    shape(p, best, HW);
    p.parts = 1;
    p.PP = (int)HW;
    p.lds_bytes = gn_lds(p.T, p.IT, best * kGnVec, p.GS, tensors, NV).bytes;
    p.lds_apply = 0;
  } else {
    if (route == 0) return p;
    p.route = 1;
    // wide candidates from the narrowest up, then the narrow ones from the widest down
    int pick = 0;
    for (int pass = 0; pass < 2 && !pick; ++pass) {
      for (int i = 1; i <= top && !pick; ++i) {
        const int SV = pass == 0 ? i : top + 1 - i;
        const bool wide = SV >= 4 || SV == p.CV;
        if (!sv_ok(p, SV, gv) || wide != (pass == 0)) continue;
        const int PR = kGnThreads / SV;
        long long PP = (long long)PR * kGnStreamItems;
        if ((HW + PP - 1) / PP > kGnMaxParts)
          PP = ((HW + kGnMaxParts - 1) / kGnMaxParts + PR - 1) / PR * PR;
        shape(p, SV, PP);
        if ((long long)p.IT * p.T * 16 > kGnLdsMax) continue;
        const int lds = gn_lds(p.T, backward ? 0 : p.IT, SV * kGnVec, p.GS, backward ? 0 : 1, NV).bytes;
        if (lds > kGnLdsMax) continue;
        pick = SV;
        p.PP = (int)PP;
        p.parts = (int)((HW + PP - 1) / PP);
        p.lds_bytes = lds;
      }
    }
    if (!pick) return p;
    p.lds_apply = gn_lds(p.T, 0, p.SV * kGnVec, p.GS, 0, NV).bytes;
  }
  const int rows = gn_slab_rows(C);
  if (p.parts > rows) return p;
  p.NR = backward ? (int)(N < rows / p.parts ? N : rows / p.parts) : 0;
  p.slab_rows = p.NR * p.parts;
  p.grid[0] = p.slices;
  p.grid[1] = p.parts;
  p.grid[2] = backward ? p.NR : (int)N;
  p.ok = true;
  return p;
}

}  // namespace dmp
