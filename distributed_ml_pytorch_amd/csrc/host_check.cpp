// Sanitizer driver for the host-side C++ of the extension (`make asan`, SURVEY
// §5.2; tests/test_asan_cpu.py).  Built host-only (hipcc --cuda-host-only: the
// kernels' device code is not compiled, nothing is launched, no GPU needed) with
// -fsanitize=address,undefined, it drives every piece of host logic that turns a
// tensor shape into kernel geometry -- tile / config selection, LDS sizing,
// split-K counts, slab sizes, the 32-bit offset guards -- over the shape sets of
// every model the framework ships (ResNet-18 CIFAR at the reference's batch 64
// and the bench's 512, ResNet-50 ImageNet bs128, ViT-B/16 bs64, AlexNet, LeNet)
// plus oversize batches that must be REJECTED, not wrapped.  Any signed overflow,
// out-of-range shift or bad access in that arithmetic aborts the run (UBSan /
// ASan, -fno-sanitize-recover).  Exit status 0 and a summary line on success.
// Every accepted tile plan of the four 3x3 halo-tile families (halo_plan.h) is
// checked against the tile invariants on the way; `host_check --plans` prints
// the plans of a fixed shape list instead (one line each, every field).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "geom_guard.h"
#include "attn_plan.h"
#include "halo_plan.h"
#include "launchers.h"

namespace {

int g_fail = 0;
long long g_checks = 0;

#define EXPECT(cond, ...)                                           \
  do {                                                              \
    ++g_checks;                                                     \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                            \
      std::fprintf(stderr, "\n");                                   \
      ++g_fail;                                                     \
    }                                                               \
  } while (0)

struct Conv {
  const char* model;
  int B, CI, H, W, CO, R, S, stride, pad;
};

int out_dim(int in, int pad, int k, int st) { return (int)dmp::guard::conv_out(in, pad, k, st); }

// every conv of a ResNet (BasicBlock / Bottleneck) at batch B
void resnet_convs(std::vector<Conv>& v, const char* name, int B, bool bottleneck, bool cifar) {
  int H = cifar ? 32 : 56, cin = 64;
  if (cifar) v.push_back({name, B, 3, 32, 32, 64, 3, 3, 1, 1});
  else v.push_back({name, B, 3, 224, 224, 64, 7, 7, 2, 3});
  const int blocks[4] = {2, 2, 2, 2}, blocks50[4] = {3, 4, 6, 3};
  for (int st = 0; st < 4; ++st) {
    const int planes = 64 << st;
    const int n = bottleneck ? blocks50[st] : blocks[st];
    for (int j = 0; j < n; ++j) {
      const int stride = (st > 0 && j == 0) ? 2 : 1;
      const int OH = out_dim(H, 1, 3, stride);
      if (bottleneck) {
        const int out = planes * 4;
        v.push_back({name, B, cin, H, H, planes, 1, 1, 1, 0});
        v.push_back({name, B, planes, H, H, planes, 3, 3, stride, 1});
        v.push_back({name, B, planes, OH, OH, out, 1, 1, 1, 0});
        if (stride != 1 || cin != out) {
          v.push_back({name, B, cin, H, H, out, 1, 1, stride, 0});
          v.push_back({name, B, cin, OH, OH, out, 1, 1, 1, 0});   // subsampled-alias form
        }
        cin = out;
      } else {
        v.push_back({name, B, cin, H, H, planes, 3, 3, stride, 1});
        v.push_back({name, B, planes, OH, OH, planes, 3, 3, 1, 1});
        if (stride != 1 || cin != planes) {
          v.push_back({name, B, cin, H, H, planes, 1, 1, stride, 0});
          v.push_back({name, B, cin, OH, OH, planes, 1, 1, 1, 0});
        }
        cin = planes;
      }
      H = OH;
    }
  }
}

// what every tile of the halo families must satisfy: bm rows, MV of them in use,
// TB images x TH rows of a gh x gw map (the class grid for stride 2)
void check_tile(int cfg, int bm, int TH, int TB, int MV, int gh, int gw, size_t lds) {
  EXPECT(MV == TB * TH * gw, "cfg %d: MV %d != %d x %d x %d", cfg, MV, TB, TH, gw);
  EXPECT(MV <= bm && 8 * (bm - MV) <= bm, "cfg %d: %d of %d rows in use", cfg, MV, bm);
  EXPECT(TB == 1 ? TH > 0 && (gh * gw) % (TH * gw) == 0 : TH == gh,
         "cfg %d: TB %d TH %d on %d x %d", cfg, TB, TH, gh, gw);
  EXPECT(lds <= (size_t)dmp::kMaxDynamicLds, "cfg %d: %zu B of LDS", cfg, lds);
}

// Every id of the four halo-tile families on one conv: the public predicates
// agree with the planners, every accepted plan holds the tile invariants, and
// (out != nullptr: --plans) after a `shape` line each accepted plan is written
// with all its fields, in the order of kPlanLegend, then the rejected ids
// counted per family.  The planners get DMP_HALO_PSW's
// default (on).  Returns how many stride-1 forward ids conv_halo_ok accepts.
const char kPlanLegend[] =
    "# halo cfg bm bn bk nw ns TH TB MV HROWS A_INS W2 PI PSW lds\n"
    "# halop cfg bm ns nw TH TB HROWS APW AINS ntiles lds\n"
    "# s2 cfg bm bn nw ns TH TB MV HROWS A_INS lds\n"
    "# wgrad cfg bm ns tr pg TH TB THX XROWS XPW ntiles tiles_per_split MV lds splits"
    " [slab_elems]\n";

int check_plans(const Conv& c, std::FILE* out) {
  const int OH = out_dim(c.H, c.pad, c.R, c.stride), OW = out_dim(c.W, c.pad, c.S, c.stride);
  char tag[96];
  std::snprintf(tag, sizeof tag, "B%d C%d %dx%d K%d %dx%d s%d p%d", c.B, c.CI, c.H, c.W, c.CO,
                c.R, c.S, c.stride, c.pad);
  if (out) std::fprintf(out, "shape %s\n", tag);
  auto rejected = [&](const char* family, int n, int of) {
    if (out) std::fprintf(out, "%s rejected %d of %d\n", family, n, of);
  };
  int nfwd = 0, nhalop = 0, rej = 0;
  for (int i = 0; i < dmp::conv_num_halo_configs(); ++i) {
    const int cfg = dmp::conv_halo_base() + i;
    const bool ok = dmp::conv_halo_ok(cfg, c.H, c.W, c.CI, c.R, c.S, c.stride, c.pad);
    nfwd += ok;
    if (dmp::is_halop(cfg)) {
      const dmp::HaloPPlan p =
          dmp::plan_halop(cfg, c.B, c.H, c.W, c.CI, c.R, c.S, c.stride, c.pad);
      // the predicate plans for batch 1: only the 2 GiB guard can differ
      EXPECT(!p.ok || ok, "cfg %d: plan ok, predicate not", cfg);
      nhalop += p.ok;
      if (!p.ok) continue;
      const dmp::HaloPGeom& g = p.g;
      check_tile(cfg, p.bm, g.TH, g.TB, p.bm, c.H, c.W, p.lds);
      EXPECT(g.APW <= dmp::hp_apw_max(p.nw) && g.APW * p.nw >= g.AINS, "cfg %d: APW %d AINS %d",
             cfg, g.APW, g.AINS);
      EXPECT((long long)g.ntiles * p.bm >= (long long)c.B * c.H * c.W, "cfg %d: %d tiles", cfg,
             g.ntiles);
      if (out)
        std::fprintf(out, "halop %d %d %d %d %d %d %d %d %d %d %zu\n", cfg, p.bm, p.ns, p.nw, g.TH,
                     g.TB, g.HROWS, g.APW, g.AINS, g.ntiles, p.lds);
      continue;
    }
    const dmp::HaloPlan p =
        dmp::plan_halo(cfg, c.H, c.W, c.CI, c.R, c.S, c.stride, c.pad, true);
    EXPECT(p.ok == ok, "cfg %d: plan %d predicate %d", cfg, p.ok, ok);
    rej += !p.ok;
    if (!p.ok) continue;
    const dmp::HaloGeom& g = p.g;
    check_tile(cfg, p.c.bm, g.TH, g.TB, g.MV, c.H, c.W, p.lds);
    EXPECT(g.A_INS <= dmp::kHaloAPW * p.c.nw, "cfg %d: A_INS %d", cfg, g.A_INS);
    if (out)
      std::fprintf(out, "halo %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu\n", cfg, p.c.bm,
                   p.c.bn, p.c.bk, p.c.nw, p.c.ns, g.TH, g.TB, g.MV, g.HROWS, g.A_INS, g.W2, g.PI,
                   g.PSW, p.lds);
  }
  rejected("halo", rej, dmp::kNumHaloConfigs - dmp::kNumHaloPConfigs);
  rejected("halop", dmp::kNumHaloPConfigs - nhalop, dmp::kNumHaloPConfigs);
  // stride-2 halo data gradient: dY (OH x OW, CO) -> dX (H x W, CI)
  rej = 0;
  for (int i = 0; i < dmp::conv_dgrad_s2_num_configs(); ++i) {
    const int cfg = dmp::conv_dgrad_s2_base() + i;
    const dmp::S2Plan p =
        dmp::plan_s2(cfg, c.H, c.W, OH, OW, c.CO, c.CI, c.R, c.S, c.stride, c.pad);
    const bool ok = dmp::conv_dgrad_s2_ok(cfg, c.H, c.W, OH, OW, c.CO, c.CI, c.R, c.S, c.stride,
                                          c.pad);
    EXPECT(p.ok == ok, "cfg %d: plan %d predicate %d", cfg, p.ok, ok);
    rej += !p.ok;
    if (!p.ok) continue;
    const dmp::HaloGeom& g = p.g;
    check_tile(cfg, p.bm, g.TH, g.TB, g.MV, OH, OW, p.lds);
    EXPECT(g.MV == p.bm && g.A_INS <= dmp::kHaloAPW * p.nw, "cfg %d: MV %d A_INS %d", cfg, g.MV,
           g.A_INS);
    if (out)
      std::fprintf(out, "s2 %d %d %d %d %d %d %d %d %d %d %zu\n", cfg, p.bm, p.bn, p.nw, p.ns,
                   g.TH, g.TB, g.MV, g.HROWS, g.A_INS, p.lds);
  }
  rejected("s2", rej, dmp::conv_dgrad_s2_num_configs());
  // halo weight gradient, atomic and slab (split-K partials) forms
  rej = 0;
  const int nwh = dmp::conv_wgrad_num_halo_configs();
  for (int i = 0; i < 2 * nwh; ++i) {
    const bool slab = i >= nwh;
    const int cfg = slab ? dmp::conv_wgrad_halo_slab_base() + i - nwh
                         : dmp::conv_wgrad_halo_base() + i;
    const dmp::WgradHaloPlan p =
        dmp::plan_wgrad_halo(cfg, c.B, c.H, c.W, c.CI, c.CO, c.R, c.S, c.stride, c.pad);
    const bool ok = dmp::conv_wgrad_halo_ok(cfg, c.B, c.H, c.W, c.CI, c.CO, c.R, c.S, c.stride,
                                            c.pad);
    const long long se = dmp::conv_wgrad_halo_slab_elems(cfg, c.B, c.H, c.W, c.CI, c.CO, c.R, c.S,
                                                         c.stride, c.pad);
    EXPECT(ok == (p.ok && (!slab || se > 0)) && se == p.slab_elems && (slab || se == 0),
           "wgrad cfg %d: plan %d predicate %d slab %lld / %lld", cfg, p.ok, ok, se, p.slab_elems);
    if (se > 0)
      EXPECT(se == (long long)p.splits * c.CO * c.R * c.S * c.CI && p.splits > 1,
             "slab elems %lld", se);
    rej += !ok;
    if (!ok) continue;
    const dmp::WgradHaloGeom& g = p.g;
    const int gh = c.stride == 2 ? c.H / 2 : c.H, gw = c.stride == 2 ? c.W / 2 : c.W;
    check_tile(cfg, p.bm, g.TH, g.TB, g.MV, gh, gw, p.lds);
    EXPECT(g.XPW <= dmp::kWhXPW && g.XPW * 4 * p.pg * 8 >= g.XROWS, "cfg %d: XPW %d XROWS %d", cfg,
           g.XPW, g.XROWS);
    EXPECT((long long)g.ntiles * g.MV >= (long long)c.B * gh * gw, "cfg %d: %d tiles", cfg,
           g.ntiles);
    EXPECT((long long)p.splits * g.tiles_per_split >= g.ntiles &&
               g.ntiles > (long long)(p.splits - 1) * g.tiles_per_split,
           "cfg %d: %d splits of %d tiles over %d", cfg, p.splits, g.tiles_per_split, g.ntiles);
    if (out) {
      std::fprintf(out, "wgrad %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d", cfg, p.bm, p.ns,
                   p.tr, p.pg, g.TH, g.TB, g.THX, g.XROWS, g.XPW, g.ntiles, g.tiles_per_split,
                   g.MV, p.lds, p.splits);
      if (slab) std::fprintf(out, " %lld", se);
      std::fprintf(out, "\n");
    }
  }
  rejected("wgrad", rej, 2 * nwh);
  return nfwd;
}

void check_conv(const Conv& c) {
  const int OH = out_dim(c.H, c.pad, c.R, c.stride), OW = out_dim(c.W, c.pad, c.S, c.stride);
  EXPECT(OH > 0 && OW > 0, "%s empty output", c.model);
  const bool fits = dmp::guard::conv_offsets_ok(c.B, c.H, c.W, c.CI, OH, OW, c.CO, c.R, c.S);
  const long long M = (long long)c.B * OH * OW;
  if (c.CI >= 64 && fits) {
    // implicit-GEMM configs: tile info and M-block counts
    const int ncfg = dmp::conv_num_configs();
    EXPECT(ncfg > 0, "no conv configs");
    for (int cfg = 0; cfg < ncfg; ++cfg) {
      int info[8] = {0};
      dmp::conv_config_info(cfg, info);
      EXPECT(info[0] > 0 && info[1] > 0 && info[2] > 0 && info[3] > 0 && info[3] <= 1024,
             "cfg %d info %d %d %d %d", cfg, info[0], info[1], info[2], info[3]);
      const int mb = dmp::conv_fwd_num_mblocks(M, c.CO, cfg);
      EXPECT(mb > 0 && (long long)mb * info[0] >= M, "cfg %d M %lld -> %d blocks of %d", cfg, M,
             mb, info[0]);
    }
    const int dflt = dmp::conv_default_config(M, c.CO);
    EXPECT(dflt >= 0 && dflt < ncfg, "default cfg %d", dflt);
    // every plan of the four 3x3 halo-tile families
    const int nhalo = check_plans(c, nullptr);
    if (c.R == 3 && c.stride == 1 && c.pad == 1 && c.H >= 4)
      EXPECT(nhalo > 0, "%s: no halo config for %dx%dx%d", c.model, c.H, c.W, c.CI);
  } else if (c.CI < 64) {
    // stems: 3x3 MFMA stem, VALU small conv, ImageNet s2d stem
    if (dmp::stem3_supported(c.CI, c.R, c.S, c.CO, c.stride, c.pad, c.W) &&
        dmp::guard::small_conv_ok(c.B, OH, OW, 2 * c.CO, (long long)c.B * c.CI * c.H * c.W)) {
      // one-pass stem backward: the grid covers every 128-pixel step, >= 4 per block
      const long long P = (long long)c.B * OH * OW;
      for (int target : {0, 1, 64, 512, 4096, 1 << 20}) {
        const int per = dmp::stem3_bn_bwd_steps(P, target);
        const long long nb = dmp::stem3_bn_bwd_blocks(P, target);
        EXPECT(per >= 4 && nb > 0 && nb * per * 128 >= P && (nb - 1) * per * 128 < P,
               "stem3 bn bwd grid: P %lld target %d -> %lld blocks of %d steps", P, target, nb,
               per);
      }
    }
    if (c.R * c.S * c.CI <= dmp::conv_small_max_k() &&
        dmp::guard::small_conv_ok(c.B, OH, OW, c.CO, (long long)c.B * c.CI * c.H * c.W)) {
      const long long P = (long long)c.B * OH * OW;
      EXPECT(dmp::conv_small_fwd_blocks(P) > 0, "small fwd blocks");
      EXPECT(dmp::conv_small_wgrad_blocks(P, c.CO, c.R, c.S, c.CI) > 0, "small wgrad blocks");
    }
    if (c.R == 7) {
      EXPECT(dmp::stem_supported(c.H, c.W), "imagenet stem %dx%d", c.H, c.W);
      EXPECT(dmp::guard::stem_batch_ok(c.B, c.H, c.W), "stem batch %d", c.B);
    }
  }
}

void check_gemm(int M, int N, int K) {
  for (int cfg = 0; cfg < dmp::gemm_num_configs(); ++cfg) {
    int info[8] = {0};
    dmp::gemm_config_info(cfg, info);
    EXPECT(info[0] > 0 && info[1] > 0 && info[2] > 0 && info[2] <= 1024, "gemm cfg %d", cfg);
    for (int mode = 0; mode < 3; ++mode) dmp::gemm_config_ok(mode, cfg);
  }
  for (int sp : {1, 2, 4, 8, 16, 64}) {
    const int e = dmp::gemm_effective_splits(K, sp);
    EXPECT(e >= 1 && e <= sp && e <= K, "splits(%d, %d) = %d", K, sp, e);
  }
  EXPECT(dmp::guard::rows_bytes_ok(2, M, K) && dmp::guard::rows_bytes_ok(2, N, K) &&
             dmp::guard::rows_bytes_ok(2, M, N),
         "gemm %dx%dx%d rejected", M, N, K);
}

void check_guards() {
  using namespace dmp::guard;
  // conv outputs
  EXPECT(conv_out(32, 1, 3, 1) == 32 && conv_out(32, 1, 3, 2) == 16 && conv_out(224, 3, 7, 2) == 112,
         "conv_out");
  EXPECT(conv_out(2, 0, 3, 1) == 0 && conv_out(8, 0, 3, 0) == 0, "conv_out empty / bad stride");
  // the largest ResNet-18 CIFAR activation that fits: 2^30 elements of bf16 at 64 ch
  EXPECT(conv_offsets_ok(16383, 32, 32, 64, 32, 32, 64, 3, 3), "16383 x 64 x 32 x 32 fits");
  EXPECT(!conv_offsets_ok(16384, 32, 32, 64, 32, 32, 64, 3, 3), "exactly 2 GiB must be rejected");
  EXPECT(!conv_offsets_ok(int64_t(1) << 40, 32, 32, 64, 32, 32, 64, 3, 3), "2^40 batch");
  EXPECT(!conv_offsets_ok(int64_t(1) << 62, 1 << 20, 1 << 20, 64, 1 << 20, 1 << 20, 64, 3, 3),
         "product overflowing int64 must be rejected, not wrapped");
  EXPECT(!conv_offsets_ok(-1, 32, 32, 64, 32, 32, 64, 3, 3), "negative batch");
  EXPECT(!conv_offsets_ok(2, 32, 32, 64, 32, 32, 1 << 21, 3, 3), "weight over 2 GiB");
  EXPECT(bf16_bytes_ok(1, 1, 1, (int64_t(1) << 30) - 1) && !bf16_bytes_ok(1, 1, 1, int64_t(1) << 30),
         "bf16 2 GiB edge");
  EXPECT(small_conv_ok(512, 32, 32, 64, 512LL * 3 * 32 * 32), "small conv bs512");
  EXPECT(!small_conv_ok(int64_t(1) << 16, 32, 32, 1 << 10, 3), "small conv output over 2^31");
  EXPECT(!small_conv_ok(1, 32, 32, 64, int64_t(1) << 30), "small conv input over 2 GiB");
  EXPECT(dmp::stem3_bn_bwd_steps(0, 0) == 0 && dmp::stem3_bn_bwd_steps(-5, 512) == 0 &&
             dmp::stem3_bn_bwd_steps(INT64_MAX, 512) == 0 && dmp::stem3_bn_bwd_blocks(INT64_MAX, 0) == 0,
         "stem3 bn bwd grid must reject empty / oversize pixel counts, not wrap");
  EXPECT(dmp::stem3_bn_bwd_steps(8, 0) == 4 && dmp::stem3_bn_bwd_blocks(8, 0) == 1 &&
             dmp::stem3_bn_bwd_steps(512LL * 1024, 0) == 8 &&
             dmp::stem3_bn_bwd_blocks(512LL * 1024, 0) == 512 &&
             dmp::stem3_bn_bwd_blocks(1152, 0) == 3 && dmp::stem3_bn_bwd_scratch_floats() > 0,
         "stem3 bn bwd grid rule");
  EXPECT(stem_batch_ok(128, 224, 224) && !stem_batch_ok(int64_t(1) << 20, 224, 224), "stem");
  EXPECT(rows_bytes_ok(2, 12608, 3072) && !rows_bytes_ok(4, int64_t(1) << 20, 1 << 10),
         "rows 2 GiB");
  EXPECT(!rows_bytes_ok(2, int64_t(1) << 62, int64_t(1) << 62), "rows overflow");
  EXPECT(!rows_bytes_ok(0, 1, 1) && !rows_bytes_ok(2, -1, 4), "rows bad args");
  // the halo / wgrad geometry must REJECT (not overflow on) batches past 2 GiB
  const int hb = dmp::conv_halo_base();
  for (int i = 0; i < dmp::conv_num_halo_configs(); ++i)
    dmp::conv_halo_ok(hb + i, 32, 32, 64, 3, 3, 1, 1);
  for (int i = 0; i < dmp::conv_wgrad_num_halo_configs(); ++i) {
    const int cfg = dmp::conv_wgrad_halo_base() + i;
    EXPECT(!dmp::conv_wgrad_halo_ok(cfg, 1 << 20, 32, 32, 64, 64, 3, 3, 1, 1),
           "wgrad cfg %d accepted a 2^20 batch", cfg);
    EXPECT(dmp::conv_wgrad_halo_slab_elems(dmp::conv_wgrad_halo_slab_base() + i, 1 << 20, 32, 32,
                                           64, 64, 3, 3, 1, 1) == 0,
           "slab for a rejected shape");
  }
}

// MX8 push payload (optim.hip mx8_layout): codes, 16-B aligned scale bytes,
// total a multiple of 4, over the arena sizes and the edges of the range
void check_mx8_layout() {
  const long long sizes[] = {0, 4, 28, 32, 36, 64, 65540, 11173962 + 54, 86567656 + 24,
                             (1LL << 31) - 4, 1LL << 31, 1LL << 40};
  for (long long n : sizes) {
    long long so = -1;
    const long long nb = dmp::mx8_layout(n, &so);
    const long long nblk = (n + 31) / 32;
    EXPECT(nb >= 0 && so >= n && so - n < 16 && so % 16 == 0, "mx8 n %lld: scales at %lld", n, so);
    EXPECT(nb % 4 == 0 && nb >= so + nblk && nb - (so + nblk) < 4, "mx8 n %lld: %lld bytes", n,
           nb);
  }
  EXPECT(dmp::mx8_layout(4, nullptr) == 20 && dmp::mx8_layout(64, nullptr) == 68, "mx8 small");
  EXPECT(dmp::mx8_layout(-4, nullptr) == -1 && dmp::mx8_layout((1LL << 40) + 4, nullptr) == -1 &&
             dmp::mx8_layout(INT64_MAX, nullptr) == -1,
         "mx8 lengths out of range must be rejected, not wrapped");
}

// device-resident datasets (data.hip): the shipped sets fit, the 2 GiB / 2^31
// edges and bad channel counts are rejected without wrapping
void check_dataset_guard() {
  using namespace dmp::guard;
  EXPECT(dataset_ok(50000, 32, 32, 3) && dataset_ok(60000, 28, 28, 1) && dataset_ok(1, 1, 1, 4),
         "CIFAR-10 / MNIST / one-pixel datasets fit");
  EXPECT(dataset_ok(14263, 224, 224, 3) && !dataset_ok(14267, 224, 224, 3),
         "ImageNet-shaped images: the 2 GiB edge");
  EXPECT(dataset_ok((int64_t(1) << 31) - 1, 1, 1, 1) && !dataset_ok(int64_t(1) << 31, 1, 1, 1),
         "dataset 2 GiB edge");
  EXPECT(!dataset_ok(int64_t(1) << 31, 1, 1, 0) && !dataset_ok(4, 8, 8, 5) &&
             !dataset_ok(4, 8, 8, 0) && !dataset_ok(-1, 8, 8, 3) && !dataset_ok(4, 0, 8, 3),
         "dataset bad extents");
  EXPECT(!dataset_ok(int64_t(1) << 30, int64_t(1) << 30, int64_t(1) << 30, 4),
         "dataset product overflowing int64 must be rejected, not wrapped");
  EXPECT(assemble_ok(512, 32, 32, 3, 4) && assemble_ok(0, 32, 32, 3, 0) &&
             assemble_ok(128, 224, 224, 3, 16),
         "assembled batches fit");
  EXPECT(!assemble_ok(512, 32, 32, 3, 17) && !assemble_ok(512, 32, 32, 3, -1) &&
             !assemble_ok(int64_t(1) << 20, 32, 32, 3, 4) && !assemble_ok(-1, 32, 32, 3, 4),
         "assemble bad pad / oversize batch");
  // the mixing form: box inside the image (empty allowed), weights in [0, 1]
  const double nan = std::nan(""), inf = HUGE_VAL;
  EXPECT(mix_ok(32, 32, 0, 0, 0, 0, 1.0, 1.0) && mix_ok(32, 32, 0, 32, 0, 32, 1.0, 0.0) &&
             mix_ok(32, 32, 31, 32, 0, 1, 1.0, 0.999) && mix_ok(5, 7, 2, 2, 3, 7, 0.0, 0.0) &&
             mix_ok(224, 224, 0, 0, 0, 0, 0.3172, 0.3172) && mix_ok(1, 1, 0, 1, 0, 1, 1e-8, 0.5),
         "mix boxes and weights in range");
  EXPECT(!mix_ok(32, 32, 0, 33, 0, 32, 1.0, 1.0) && !mix_ok(32, 32, 0, 32, 0, 33, 1.0, 1.0) &&
             !mix_ok(32, 32, -1, 4, 0, 4, 1.0, 1.0) && !mix_ok(32, 32, 0, 4, -1, 4, 1.0, 1.0) &&
             !mix_ok(32, 32, 5, 4, 0, 4, 1.0, 1.0) && !mix_ok(32, 32, 0, 4, 9, 8, 1.0, 1.0) &&
             !mix_ok(32, 32, 0, int64_t(1) << 40, 0, 4, 1.0, 1.0) &&
             !mix_ok(32, 32, INT64_MIN, 4, 0, INT64_MAX, 1.0, 1.0),
         "mix box outside the image or reversed");
  EXPECT(!mix_ok(32, 32, 0, 0, 0, 0, 1.5, 1.0) && !mix_ok(32, 32, 0, 0, 0, 0, 1.0, 1.5) &&
             !mix_ok(32, 32, 0, 0, 0, 0, -1e-9, 1.0) && !mix_ok(32, 32, 0, 0, 0, 0, 1.0, -0.5) &&
             !mix_ok(32, 32, 0, 0, 0, 0, nan, 1.0) && !mix_ok(32, 32, 0, 0, 0, 0, 1.0, nan) &&
             !mix_ok(32, 32, 0, 0, 0, 0, inf, 1.0) && !mix_ok(32, 32, 0, 0, 0, 0, 1.0, -inf),
         "mix weights outside [0, 1], NaN or infinite");
}

// attention plans (attn_plan.h) over every token count either route takes, the
// edges that must be refused, and batch * heads products up to the grid limit
void check_attention_plans() {
  using namespace dmp;
  for (int N = 1; N <= kAttnStreamMax + 1; ++N) {
    for (int route = kAttnAuto; route <= kAttnStream; ++route) {
      const AttnPlan p = plan_attention(N, route, 16 * 12);
      const bool want = route == kAttnResident ? N <= kAttnResidentMax : N <= kAttnStreamMax;
      EXPECT(p.ok == want, "N %d route %d: ok %d", N, route, p.ok);
      if (!p.ok) continue;
      EXPECT(p.route == (route == kAttnAuto ? (N <= kAttnResidentMax ? kAttnResident : kAttnStream)
                                            : route),
             "N %d request %d -> route %d", N, route, p.route);
      // blocks x block size and tiles x tile size cover N, the last of each is not empty
      EXPECT((long long)p.q_blocks * p.q_block >= N && (long long)(p.q_blocks - 1) * p.q_block < N &&
                 (long long)p.k_blocks * p.k_block >= N && (long long)(p.k_blocks - 1) * p.k_block < N,
             "N %d: blocks %d x %d, %d x %d", N, p.q_blocks, p.q_block, p.k_blocks, p.k_block);
      EXPECT((long long)p.k_tiles * p.k_tile >= N && (long long)(p.k_tiles - 1) * p.k_tile < N &&
                 (long long)p.q_tiles * p.q_tile >= N && (long long)(p.q_tiles - 1) * p.q_tile < N,
             "N %d: tiles %d x %d, %d x %d", N, p.k_tiles, p.k_tile, p.q_tiles, p.q_tile);
      EXPECT(p.q_block == kAttnStrip * p.waves || p.route == kAttnResident, "N %d: strips", N);
      EXPECT(p.k_tile % 32 == 0 && p.q_tile % 32 == 0, "N %d: tiles of whole k-step pairs", N);
      const size_t stage = attn_image_pair_bytes(p.k_tile);
      EXPECT(p.lds_fwd == p.stages * stage && p.lds_dq == p.lds_fwd &&
                 p.lds_dkv == p.stages * (attn_image_pair_bytes(p.q_tile) + (size_t)8 * p.q_tile),
             "N %d: lds %zu %zu %zu", N, p.lds_fwd, p.lds_dq, p.lds_dkv);
      EXPECT(p.lds_fwd <= (size_t)kAttnLdsLimit && p.lds_dkv <= (size_t)kAttnLdsLimit,
             "N %d: %zu B of LDS", N, p.lds_dkv);
      // two workgroups per CU on the streaming route
      EXPECT(p.route == kAttnResident || 2 * p.lds_dkv <= (size_t)kAttnLdsLimit, "N %d", N);
      EXPECT(p.grid_fwd == 16LL * 12 * p.q_blocks && p.grid_dq == p.grid_fwd &&
                 p.grid_dkv == 16LL * 12 * p.k_blocks,
             "N %d: grids %lld %lld", N, p.grid_fwd, p.grid_dkv);
    }
  }
  for (int route = kAttnAuto; route <= kAttnStream; ++route) {
    EXPECT(!plan_attention(0, route).ok && !plan_attention(-1, route).ok &&
               !plan_attention(kAttnStreamMax + 1, route).ok &&
               !plan_attention(0x7fffffff, route).ok,
           "route %d: N out of range accepted", route);
    EXPECT(!plan_attention(197, route, 0).ok && !plan_attention(197, route, -3).ok &&
               !plan_attention(197, route, 1LL << 31).ok && !plan_attention(197, route, 1LL << 62).ok,
           "route %d: bad batch * heads accepted", route);
  }
  EXPECT(!plan_attention(197, 2).ok && !plan_attention(197, -2).ok, "unknown route accepted");
  EXPECT(!plan_attention(257, kAttnResident).ok && plan_attention(256, kAttnResident).ok,
         "resident route cap");
  // the grid limit: 32 blocks at 4096 tokens
  EXPECT(plan_attention(4096, kAttnStream, 0x7fffffffLL / 32).ok &&
             !plan_attention(4096, kAttnStream, 0x7fffffffLL / 32 + 1).ok &&
             plan_attention(256, kAttnAuto, 0x7fffffffLL).ok,
         "grid past 2^31 - 1 must be refused, not wrapped");
  EXPECT(attention_max_tokens() == kAttnStreamMax && attn_plan_max_tokens() == kAttnStreamMax,
         "attention cap");
  EXPECT(attention_bwd_workspace_floats(16, 577, 12, kAttnAuto) == 16LL * 12 * 577 &&
             attention_bwd_workspace_floats(16, 197, 12, kAttnAuto) == 0 &&
             attention_bwd_workspace_floats(16, 197, 12, kAttnStream) == 16LL * 12 * 197 &&
             attention_bwd_workspace_floats(16, 4097, 12, kAttnAuto) == 0,
         "attention backward workspace");
}

}  // namespace

// DMP_ASAN_SELFTEST=asan|ubsan: a deliberate heap overflow / signed overflow,
// so the test can see that the sanitizers are really in the build
int selftest(const char* kind) {
  volatile int n = 8;
  if (kind[0] == 'a') {
    int* p = new int[n];
    p[0] = 1;
    const int v = p[n];            // one past the end: ASan heap-buffer-overflow
    delete[] p;
    return v;
  }
  volatile int big = 0x7fffffff;
  return big + n;                  // UBSan: signed integer overflow
}

// The fixed 3x3 / pad-1 shape list of the plan table.  --plans writes the table
// to stdout (tests/golden/halo_plans.txt is that output; tests/test_asan_cpu.py
// compares); the default run checks the same plans silently.
void check_plan_shapes(std::FILE* out) {
  struct { int B, CI, H, W, CO, stride; } const shapes[] = {
      // tests/test_conv_gpu.py HALO_SHAPES
      {4, 64, 32, 32, 64, 1}, {3, 128, 16, 16, 128, 1}, {5, 256, 8, 8, 256, 1},
      {9, 512, 4, 4, 512, 1}, {2, 64, 8, 8, 128, 1}, {2, 64, 56, 56, 64, 1},
      {3, 128, 28, 28, 128, 1}, {3, 256, 14, 14, 256, 1}, {5, 512, 7, 7, 512, 1},
      // test_halo_wgrad_stride2, test_stride2_halo_dgrad_configs
      {3, 64, 32, 32, 128, 2}, {5, 128, 16, 16, 256, 2}, {9, 256, 8, 8, 512, 2},
      {2, 128, 56, 56, 128, 2}, {4, 64, 32, 32, 128, 2}, {2, 128, 16, 16, 256, 2},
      {8, 256, 8, 8, 512, 2}, {2, 64, 56, 56, 128, 2},
      // ResNet-18 CIFAR at batch 512
      {512, 64, 32, 32, 64, 1}, {512, 64, 32, 32, 128, 2}, {512, 128, 16, 16, 128, 1},
      {512, 128, 16, 16, 256, 2}, {512, 256, 8, 8, 256, 1}, {512, 256, 8, 8, 512, 2},
      {512, 512, 4, 4, 512, 1},
      // ResNet-50 ImageNet at batch 128
      {128, 64, 56, 56, 64, 1}, {128, 128, 56, 56, 128, 2}, {128, 128, 28, 28, 128, 1},
      {128, 256, 28, 28, 256, 2}, {128, 256, 14, 14, 256, 1}, {128, 512, 14, 14, 512, 2},
      {128, 512, 7, 7, 512, 1},
      // edges.  W not a multiple of 16 and H != W (28 / 14 / 7 wide: above)
      {2, 64, 9, 11, 64, 1},
      // a map smaller than any tile (4x4: above)
      {4, 64, 2, 2, 64, 1},
      // C not a multiple of 32 or 64
      {2, 48, 16, 16, 48, 1}, {2, 96, 16, 16, 96, 1},
      // batch 1, and batches past the 2 GiB guard
      {1, 64, 32, 32, 64, 1}, {16384, 64, 32, 32, 64, 1}, {1 << 20, 64, 32, 32, 128, 2},
  };
  if (out) std::fputs(kPlanLegend, out);
  for (const auto& s : shapes)
    check_plans({"plans", s.B, s.CI, s.H, s.W, s.CO, 3, 3, s.stride, 1}, out);
}

int main(int argc, char** argv) {
  if (const char* st = std::getenv("DMP_ASAN_SELFTEST")) return selftest(st);
  if (argc > 1 && std::strcmp(argv[1], "--plans") == 0) {
    check_plan_shapes(stdout);
    return g_fail == 0 ? 0 : 1;
  }
  std::vector<Conv> convs;
  for (int B : {1, 8, 64, 512, 1024}) resnet_convs(convs, "resnet18-cifar", B, false, true);
  for (int B : {1, 32, 128}) resnet_convs(convs, "resnet50-imagenet", B, true, false);
  // AlexNet-CIFAR (/root/reference/example/models.py:25-49) and LeNet
  for (int B : {64, 10000}) {
    convs.push_back({"alexnet", B, 3, 32, 32, 64, 11, 11, 4, 5});
    convs.push_back({"alexnet", B, 64, 4, 4, 192, 5, 5, 1, 2});
    convs.push_back({"alexnet", B, 192, 2, 2, 384, 3, 3, 1, 1});
    convs.push_back({"alexnet", B, 384, 2, 2, 256, 3, 3, 1, 1});
    convs.push_back({"alexnet", B, 256, 2, 2, 256, 3, 3, 1, 1});
    convs.push_back({"lenet", B, 3, 32, 32, 6, 5, 5, 1, 0});
  }
  for (const Conv& c : convs) check_conv(c);
  check_plan_shapes(nullptr);
  // ViT-B/16 bs64 (197 tokens, D 768, MLP 3072) and the CNN heads
  for (int M : {64 * 197, 8 * 197, 64 * 196})
    for (int NK : {768, 2304, 3072}) {
      check_gemm(M, NK, 768);
      check_gemm(M, 768, NK);
    }
  check_gemm(512, 10, 512);
  check_gemm(128, 1000, 2048);
  EXPECT(dmp::layernorm_supported(768), "layernorm 768");
  EXPECT(dmp::attention_max_tokens() >= 197 && dmp::attention_head_dim() == 64, "attention");
  EXPECT(dmp::gap_linear_supported(512, 10), "gap_linear 512 -> 10");
  EXPECT(dmp::bn_maxpool_supported(64, 3, 2, 1) && !dmp::bn_maxpool_supported(64, 2, 2, 0),
         "bn_maxpool window");
  check_guards();
  check_mx8_layout();
  check_dataset_guard();
  check_attention_plans();
  std::printf("host_check: %lld checks over %zu conv shapes, %d failed\n", g_checks, convs.size(),
              g_fail);
  return g_fail == 0 ? 0 : 1;
}
