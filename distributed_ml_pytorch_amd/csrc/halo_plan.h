// Host-side tile plans of the four 3x3 halo-tile kernel families: forward and
// stride-1 dgrad (conv_halo_kernel), persistent 64-channel (conv_halo64p_kernel),
// stride-2 dgrad (conv_dgrad_s2_kernel) and the halo weight gradient
// (conv_wgrad_halo_kernel).  A planner turns (cfg id, shape) into the geometry
// struct its kernel takes by value, the decoded config and the LDS bytes, or
// says that the config does not apply.  Plain C++ (no torch, no HIP), so the
// sanitizer driver (host_check.cpp, `make asan`) can compute, print and check
// every plan on a CPU; conv.hip and conv_wgrad.hip keep only the dispatch from a
// plan to a template instantiation.
#pragma once

#include <cstddef>

#include "halo_pm.h"

namespace dmp {

// dynamic LDS a block may ask for (of the CU's 160 KiB)
constexpr int kMaxDynamicLds = 160 * 1024;

// ------------------------------------------------------------ kernel arguments
// (passed by value to the kernels: field order and types are part of their ABI;
// TH, TB, MV: halo_tiling below)
struct HaloGeom {
  int TH, TB, HROWS, A_INS, MV;
  // conv_halo_kernel staging: staged row width W2 (W + 2, or W + 4 with PSW),
  // rows per image block PI ((TH + 2) * W2 [+ pad]), PSW: swizzle keyed on the
  // pixel-like index (see conv_halo_kernel)
  int W2, PI, PSW;
};

struct HaloPGeom {
  int TH, TB, HROWS, APW, AINS, ntiles;   // APW: pieces per wave (>= AINS / NW), AINS: exact
  // DIAGNOSTIC (DMP_HALO64P_XFORM=1, forward only): the cost of applying a
  // per-channel BatchNorm scale / shift + clamp to the staged input tile in LDS
  // ("apply-in-consumer"): every wave rewrites its own landed halo pieces,
  // x -> max(x * xs + xh, xlo), before the tile's barrier.  Run with the
  // identity (xs 1, xh 0, xlo -inf: outputs unchanged, the work is not
  // foldable: runtime values) to price the transform against the BN apply
  // pass it would replace (profiles/bn_consumer_fusion_r3.txt).
  int xform;
  float xs, xh, xlo;
  // 8-wave blocks: waves 4-7 (the SIMD partners of waves 0-3) run each tile as
  // compute(k) -> epilogue(k) instead of epilogue(k-1) -> compute(k), so one
  // wave's epilogue VALU and stores overlap its partner's MFMAs instead of both
  // waves of a SIMD storing at once after the tile barrier (MI355X_MICROARCH.md,
  // "Two waves per SIMD" item 9: split roles by wave number >= 4)
  int stagger;
};

struct WgradHaloGeom {
  int TH, TB, THX, XROWS, XPW, ntiles, tiles_per_split, MV;
};

constexpr int kHaloAPW = 8;   // max halo DMA instructions per wave per stage
constexpr int kHpAPW = 12;    // max halo DMA pieces per wave per tile
// 8-wave blocks need at most 8 (BM 256 on 32 x 32 / 64 x 64 maps: 6 / 7): the
// smaller bound frees 8 VGPRs of slot offsets in the register-capped kernel
constexpr int hp_apw_max(int nw) { return nw == 8 ? 8 : kHpAPW; }
constexpr int kWhXPW = 12;    // max X-row DMA instructions per wave per stage

// ------------------------------------------------------------ the tiling rule
// How a BM-pixel tile divides an H x W map: whole rows of one image (TB = 1,
// TH rows) or whole images (TH = H, TB images), MV = TB * TH * W pixels of the
// tile in use.  Row tiles take the most whole rows that fit BM and tile the
// image.  Padded tiles (MV < BM; ImageNet 28x28: 7 rows = 196 pixels in 224,
// 56x56: 4 rows in 256, 14x14 / 7x7: whole images) may leave at most 1/8 of
// the tile's rows idle: forward / dgrad rows past MV read a valid staged row
// and the epilogue drops them, wgrad dY rows past MV stage zeros.  A strict
// caller takes exact tiles only.
struct HaloTiling {
  bool ok;
  int TH, TB, MV;
};

inline HaloTiling halo_tiling(int bm, int H, int W, bool padded) {
  HaloTiling t{};
  const int img = H * W;
  if (H <= 0 || W <= 0) return t;
  if (bm <= img) {
    t.TB = 1;
    t.TH = bm / W;
    while (t.TH > 0 && img % (t.TH * W) != 0) --t.TH;
    if (t.TH == 0) return t;
  } else {
    t.TH = H;
    t.TB = bm / img;
  }
  t.MV = t.TB * t.TH * W;
  t.ok = padded ? 8 * (bm - t.MV) <= bm : t.MV == bm;
  return t;
}

// --------------------------------------------- forward / stride-1 dgrad tiles
// Halo-tile configurations (BM, BN, BK, WM, WN, NS), cfg ids kHaloBase + i; only
// for 3x3 / stride 1 / pad 1 and block tiles of whole rows or whole images.
#define DMP_HALO_CONFIGS(X)   \
  X(0, 256, 64, 32, 4, 2, 2)  \
  X(1, 128, 64, 32, 2, 2, 2)  \
  X(2, 64, 64, 32, 2, 2, 2)   \
  X(3, 128, 64, 32, 4, 2, 2)  \
  X(4, 256, 64, 32, 2, 2, 2)  \
  X(5, 128, 64, 32, 2, 2, 1)  \
  X(6, 256, 64, 32, 4, 2, 1)  \
  X(7, 64, 64, 32, 2, 2, 1)   \
  X(8, 128, 64, 32, 4, 2, 1)   \
  X(9, 256, 64, 32, 4, 1, 1)   \
  X(10, 256, 64, 32, 4, 1, 2)  \
  X(11, 128, 64, 32, 2, 1, 1)  \
  X(12, 128, 128, 32, 2, 2, 1) \
  X(13, 256, 128, 32, 4, 2, 1) \
  X(14, 512, 64, 32, 8, 1, 1)  \
  X(18, 224, 64, 32, 2, 2, 1)  \
  X(19, 224, 64, 32, 2, 1, 1)  \
  X(20, 112, 64, 32, 1, 2, 1)  \
  X(21, 112, 128, 32, 1, 4, 1) \
  X(22, 112, 128, 32, 1, 2, 1) \
  X(23, 448, 64, 32, 4, 2, 1)  \
  X(24, 224, 64, 32, 2, 2, 2)  \
  X(25, 112, 128, 32, 1, 4, 2)
// 18-25: whole-row tiles of 7 x 16 pixels for the ImageNet ResNet widths (56-
// and 28-pixel rows: 4 / 2 / 8 rows of 56, 4 rows of 28), where none of the
// power-of-two tiles above is a whole number of rows.  Ids 15-17 are the
// persistent kernels below (kept: ids are cached by the tuner).

constexpr int kHaloBase = 100, kNumHaloConfigs = 26;   // ids kHaloBase + [0, 26)
// persistent 64-channel halo kernels (conv_halo64p_kernel): ids 115-117
constexpr int kHaloPBase = kHaloBase + 15, kNumHaloPConfigs = 3;
constexpr bool is_halop(int cfg) {
  return cfg >= kHaloPBase && cfg < kHaloPBase + kNumHaloPConfigs;
}

struct HaloCfg {
  bool ok;
  int bm, bn, bk, nw, ns;
};

inline HaloCfg halo_cfg(int cfg) {
  switch (cfg - kHaloBase) {
#define X(i, BM, BN, BK, WM, WN, NS) \
  case i: return {true, BM, BN, BK, WM * WN, NS};
    DMP_HALO_CONFIGS(X)
#undef X
  }
  return {};
}

struct HaloPlan {
  bool ok;
  HaloGeom g;
  HaloCfg c;
  size_t lds;
};

// plan of a halo config on an (H, W, C) input; !ok when it does not apply.
// psw: allow the W + 4-wide staging (on unless DMP_HALO_PSW=0)
inline HaloPlan plan_halo(int cfg, int H, int W, int C, int R, int S, int stride, int pad,
                          bool psw) {
  HaloPlan p{};
  p.c = halo_cfg(cfg);
  if (!p.c.ok) return p;
  const int bm = p.c.bm, bn = p.c.bn, bk = p.c.bk;
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C % bk != 0) return p;
  const HaloTiling t = halo_tiling(bm, H, W, true);
  if (!t.ok) return p;
  HaloGeom& h = p.g;
  h.TH = t.TH;
  h.TB = t.TB;
  h.MV = t.MV;
  const int rpi = 64 / (bk / 8);
  // fragments wrapping image rows (W not a multiple of 16, not the <= 8 widths the
  // row-parity key covers): the W + 4-wide staging of conv_halo_kernel (PSW)
  h.PSW = psw && bk == 32 && W % 16 != 0 && !(W <= 8 && 16 % W == 0);
  h.W2 = h.PSW ? W + 4 : W + 2;
  h.PI = (h.TH + 2) * h.W2;
  if (h.PSW) h.PI += (((h.TH * W - h.PI) % 4) + 4) % 4;   // PI == TH * W (mod 4)
  h.HROWS = h.TB * h.PI;
  h.A_INS = (h.HROWS + rpi - 1) / rpi;
  if (h.A_INS > kHaloAPW * p.c.nw) return p;
  const size_t stage = (size_t)h.A_INS * rpi * bk + (size_t)9 * bn * bk;
  p.lds = (size_t)p.c.ns * stage * 2;
  if (p.lds < (size_t)bm * (bn + 8) * 2) p.lds = (size_t)bm * (bn + 8) * 2;   // row epilogue tile
  p.ok = p.lds <= (size_t)kMaxDynamicLds;
  return p;
}

// Position-major plan (halo_pm.h) of a halo config: 4 x 4 maps in whole-image
// tiles of 16 images, one fragment = one pixel position across them, padding
// taps not issued.  Taken by launch_halo instead of plan_halo's dense plan under
// the same cfg id; !ok: the config keeps the dense kernel.  Covers the 256 x 64
// two-stage tile of 4 x 2 waves (id kHaloBase), the pick of ResNet-18's stage 4.
constexpr bool halo_pm_cfg(int cfg) { return cfg == kHaloBase; }

inline HaloPlan plan_halo_pm(int cfg, int H, int W, int C, int R, int S, int stride, int pad) {
  HaloPlan p{};
  if (!halo_pm_cfg(cfg)) return p;
  p.c = halo_cfg(cfg);
  if (!p.c.ok || p.c.bm != pm::kBM || p.c.bk != 32) return p;
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C % p.c.bk != 0) return p;
  if (H != pm::kH || W != pm::kW) return p;
  const HaloTiling t = halo_tiling(p.c.bm, H, W, false);
  if (!t.ok || t.TH != H || t.TB != pm::kTB) return p;
  HaloGeom& h = p.g;
  h.TH = t.TH;
  h.TB = t.TB;
  h.MV = t.MV;
  h.PSW = 0;
  h.W2 = W;          // no halo columns
  h.PI = pm::kPI;
  h.HROWS = pm::kRows;
  h.A_INS = pm::kPieces;
  if (h.A_INS > kHaloAPW * p.c.nw) return p;
  const size_t stage = (size_t)pm::kRows * p.c.bk + (size_t)9 * p.c.bn * p.c.bk;
  p.lds = (size_t)p.c.ns * stage * 2;
  const size_t epi = (size_t)pm::epi_elems(p.c.bn) * 2;   // row epilogue tile
  if (p.lds < epi) p.lds = epi;
  p.ok = p.lds <= (size_t)kMaxDynamicLds;
  return p;
}

// ------------------------------------------------ persistent 64-channel tiles
// ids kHaloPBase + i -> (BM, NS, waves)
constexpr int kHaloP[kNumHaloPConfigs][3] = {{256, 2, 4}, {128, 3, 4}, {256, 2, 8}};

struct HaloPPlan {
  bool ok;
  HaloPGeom g;   // xform .. stagger are the launcher's to fill
  int bm, ns, nw;
  size_t lds;
};

inline HaloPPlan plan_halop(int cfg, int B, int H, int W, int C, int R, int S, int stride,
                            int pad) {
  HaloPPlan p{};
  if (!is_halop(cfg)) return p;
  const int* row = kHaloP[cfg - kHaloPBase];
  const int bm = p.bm = row[0], ns = p.ns = row[1], nw = p.nw = row[2];
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C != 64) return p;
  const HaloTiling t = halo_tiling(bm, H, W, false);
  if (!t.ok) return p;
  HaloPGeom& h = p.g;
  h.TH = t.TH;
  h.TB = t.TB;
  h.HROWS = h.TB * (h.TH + 2) * (W + 2);
  h.AINS = (h.HROWS + 7) / 8;
  h.APW = (h.AINS + nw - 1) / nw;
  if (h.APW > hp_apw_max(nw) || (ns - 2) * h.APW > 24) return p;
  const long long P = (long long)B * H * W;
  if (2LL * P * 64 >= (1LL << 31)) return p;
  h.ntiles = (int)((P + bm - 1) / bm);
  const size_t pieces = ns == 2 ? (size_t)h.AINS : (size_t)h.APW * nw;
  p.lds = 2 * ((size_t)9 * 64 * 64 + (size_t)ns * pieces * 8 * 64);
  p.ok = p.lds <= (size_t)kMaxDynamicLds;
  return p;
}

// ------------------------------------------------------- stride-2 dgrad tiles
// (conv_dgrad_s2_kernel): id, BM, BN, WM, WN, NS; ids kS2Base + i
// (wave tiles of 32 pixels x 64 channels or 64 x 32 per class: 4 classes x 8
// accumulator tiles = 128 registers)
#define DMP_S2_CONFIGS(X)      \
  X(0, 128, 64, 4, 1, 1)       \
  X(1, 256, 64, 8, 1, 1)       \
  X(2, 128, 128, 4, 2, 1)      \
  X(3, 256, 32, 4, 1, 1)       \
  X(4, 64, 64, 2, 1, 1)        \
  X(5, 112, 64, 7, 1, 1)       \
  X(6, 256, 64, 8, 1, 2)       \
  X(7, 128, 128, 4, 2, 2)      \
  X(8, 128, 64, 8, 1, 2)       \
  X(9, 112, 64, 7, 1, 2)
constexpr int kS2Base = 200, kNumS2Configs = 10;

struct S2Plan {
  bool ok;
  HaloGeom g;   // tiles of the class grid (= dY geometry): TH, TB, HROWS, A_INS, MV
  int bm, bn, nw, ns;
  size_t lds;
};

// plan of a stride-2 halo dgrad config: dY (OH x OW, K channels) -> dX (H x W, N channels)
inline S2Plan plan_s2(int cfg, int H, int W, int OH, int OW, int K, int N, int R, int S,
                      int stride, int pad) {
  S2Plan p{};
  switch (cfg - kS2Base) {
#define X(i, BM, BN, WM, WN, NS) \
  case i: p.bm = BM; p.bn = BN; p.nw = WM * WN; p.ns = NS; break;
    DMP_S2_CONFIGS(X)
#undef X
    default: return p;
  }
  if (R != 3 || S != 3 || stride != 2 || pad != 1 || H != 2 * OH || W != 2 * OW) return p;
  if (K % 32 != 0 || N % p.bn != 0) return p;
  const HaloTiling t = halo_tiling(p.bm, OH, OW, false);
  if (!t.ok) return p;
  HaloGeom& h = p.g;
  h.TH = t.TH;
  h.TB = t.TB;
  h.MV = t.MV;
  h.HROWS = h.TB * (h.TH + 1) * (OW + 1);
  h.A_INS = (h.HROWS + 15) / 16;
  if (h.A_INS > kHaloAPW * p.nw) return p;
  p.lds = (size_t)p.ns * 2 * ((size_t)h.A_INS * 512 + (size_t)9 * p.bn * 32);
  p.ok = p.lds <= (size_t)kMaxDynamicLds;
  return p;
}

// ------------------------------------------------------ halo weight gradient
// cfg ids: kWhBase + variant * 12 + bm_sel * 4 + spl; BM = 64 << bm_sel, target
// block count 128 << spl; variant -> (NS, TR, PG) below (ids 1000..1011 are the
// round-1 kernel's configs: NS 2, one tap row per block)
constexpr int kWhBase = 1000;
// variants 6-7: BM fixed at 224 = 4 rows of 56 (ImageNet ResNet stage 1, where no
// power-of-two tile is a whole number of rows); only bm_sel 0 is valid there
constexpr int kWhVariants = 8;
constexpr int kWhNS[kWhVariants] = {2, 3, 4, 2, 3, 2, 2, 3};
constexpr int kWhTR[kWhVariants] = {1, 1, 1, 3, 3, 1, 1, 1};
constexpr int kWhPG[kWhVariants] = {1, 1, 1, 1, 1, 2, 1, 1};   // pixel groups (8 waves when 2)
constexpr int kWhBM[kWhVariants] = {0, 0, 0, 0, 0, 0, 224, 224};   // 0: 64 << bm_sel
constexpr int kNumWhConfigs = 12 * kWhVariants;

// slab mode (ids kWhSlabBase + i = halo config kWhBase + i): the split-K partials
// go to a [splits][dW] fp32 slab with plain stores (~6 TB/s chip-wide) and one
// streaming pass adds them into dW, instead of fp32 atomics (~1.3 TB/s of added
// bytes, ~25 % of the 64-channel wgrad: profiles/conv_kernels_r2.txt); offered
// for the NS-2 one-tap-row variants when the geometry splits K
constexpr int kWhSlabBase = 3000;
constexpr bool wh_slab_variant(int var) { return var == 0 || var == 5 || var == 6; }

struct WgradHaloPlan {
  bool ok;   // the tiles apply (a slab id is offered only when slab_elems > 0 as well)
  WgradHaloGeom g;
  int bm, ns, tr, pg, splits;
  size_t lds;
  long long slab_elems;   // fp32 elements of the slab a slab id needs (0: not offered)
};

inline WgradHaloPlan plan_wgrad_halo(int cfg, int B, int H, int W, int CI, int CO, int R, int S,
                                     int stride, int pad) {
  WgradHaloPlan p{};
  const bool slab = cfg >= kWhSlabBase;
  const int id = cfg - (slab ? kWhSlabBase : kWhBase);
  if (id < 0 || id >= kNumWhConfigs) return p;
  const int var = id / 12, rest = id % 12;
  if (kWhBM[var] != 0 && rest / 4 != 0) return p;
  const int bm = p.bm = kWhBM[var] != 0 ? kWhBM[var] : 64 << (rest / 4);
  const int target = 128 << (rest % 4);
  const int ns = p.ns = kWhNS[var], tr = p.tr = kWhTR[var], pg = p.pg = kWhPG[var];
  if (pg == 2 && bm < 128) return p;
  if (R != 3 || S != 3 || pad != 1 || CI % 64 || CO % 64) return p;
  const bool s2 = stride == 2;
  if (stride != 1 && !(s2 && tr == 1 && H % 2 == 0 && W % 2 == 0 && ns <= 3 && kWhBM[var] == 0))
    return p;
  if (tr == 3 && bm > 128) return p;   // 36 accumulator tiles + hoisted addresses spill
  const int XW = W;                    // staged X row width - 2 (input columns)
  if (s2) { H /= 2; W /= 2; }          // tiles run over the dY (output) geometry
  const HaloTiling t = halo_tiling(bm, H, W, true);
  if (!t.ok) return p;
  WgradHaloGeom& h = p.g;
  h.TH = t.TH;
  h.TB = t.TB;
  h.MV = t.MV;
  h.THX = h.TH + tr - 1;
  h.XROWS = h.TB * h.THX * (XW + 2);
  h.XPW = ((h.XROWS + 7) / 8 + 4 * pg - 1) / (4 * pg);
  if (h.XPW > kWhXPW || h.THX + 1 > 127 || h.TB > 0x7fff) return p;
  if ((ns - 2) * (bm / 32 + h.XPW) > 40) return p;
  const long long M = (long long)B * H * W;
  if (2LL * M * (CO > CI ? CO : CI) * (s2 ? 4 : 1) >= (1LL << 31)) return p;
  h.ntiles = (int)((M + h.MV - 1) / h.MV);
  const int per = (CI / 64) * (CO / 64) * (3 / tr);
  int sp = target / per;
  if (sp < 1) sp = 1;
  if (sp > h.ntiles) sp = h.ntiles;
  h.tiles_per_split = (h.ntiles + sp - 1) / sp;
  p.splits = (h.ntiles + h.tiles_per_split - 1) / h.tiles_per_split;
  const size_t stage = (size_t)bm * 64 + (size_t)h.XPW * 4 * pg * 512;
  p.lds = (size_t)ns * stage * 2;
  p.ok = p.lds <= (size_t)kMaxDynamicLds;
  if (p.ok && slab && p.splits > 1 && wh_slab_variant(var))
    p.slab_elems = (long long)p.splits * CO * R * S * CI;
  return p;
}

}  // namespace dmp
