// CPU check of the position-major halo tiles (halo_pm.h, plan_halo_pm): stand-alone,
// built with -fsanitize=address,undefined by tests/test_halo_pm_cpu.py.
//
//   (a) the tap-validity table against brute-force geometry on a zero-padded map,
//       and the live (fragment, tap) counts per wave row and per SIMD;
//   (b) the kernel's own maps walked end to end -- DMA slot -> source pixel,
//       fragment row -> staged row per live tap, epilogue row -> output pixel --
//       on a small integer conv for B in {1, 16, 17}, both tap orders (forward,
//       mirrored = data gradient), against a direct conv;
//   (c) bank conflicts of every live A-fragment ds_read_b128 over the four
//       16-lane groups the LDS serves it in, and the row epilogue's ds_write_b64.
//
// Prints one "halo_pm_check: ..." summary line; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "halo_plan.h"

using namespace dmp;

static long long g_checks = 0;
static int g_failed = 0;

#define CHECK(cond, ...)                            \
  do {                                              \
    ++g_checks;                                     \
    if (!(cond)) {                                  \
      ++g_failed;                                   \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                     \
      std::printf("\n");                            \
    }                                               \
  } while (0)

constexpr int kCfg = kHaloBase;   // 256 x 64 tile, 4 x 2 waves, two stages
constexpr int BK = 32, CPR = BK / 8, RPI = 64 / CPR;

// ---------------------------------------------------------------- (a) validity
static void check_validity() {
  // brute force: a 6 x 6 map with a one-pixel zero border, interior marked
  bool inside[pm::kH + 2][pm::kW + 2] = {};
  for (int h = 0; h < pm::kH; ++h)
    for (int w = 0; w < pm::kW; ++w) inside[h + 1][w + 1] = true;
  int pairs = 0;
  for (int h = 0; h < pm::kH; ++h)
    for (int w = 0; w < pm::kW; ++w)
      for (int t = 0; t < 9; ++t) {
        const bool ref = inside[h + t / 3][w + t % 3];
        CHECK(pm::tap_valid(h, w, t) == ref, "tap_valid(%d, %d, %d)", h, w, t);
        pairs += ref ? 1 : 0;
        if (ref) {
          const int src = h * pm::kW + w + pm::tap_shift(t);
          CHECK(src == (h + t / 3 - 1) * pm::kW + (w + t % 3 - 1) && src >= 0 && src < pm::kImg,
                "tap_shift(%d) at (%d, %d)", t, h, w);
        }
      }
  CHECK(pairs == 100, "in-image (pixel, tap) pairs: %d", pairs);
  // every position is exactly one fragment of one wave row ... of every wave row
  int live_wm[pm::kWM] = {};
  for (int wm = 0; wm < pm::kWM; ++wm) {
    bool hrow[pm::kH] = {}, wcol[pm::kW] = {};
    for (int i = 0; i < pm::kTM; ++i) {
      hrow[pm::frag_h(wm, i)] = true;
      wcol[pm::frag_w(wm, i)] = true;
      for (int t = 0; t < 9; ++t) live_wm[wm] += pm::live(wm, i, t) ? 1 : 0;
    }
    for (int k = 0; k < 4; ++k) CHECK(hrow[k] && wcol[k], "Latin square, wave row %d", wm);
    int by_tap = 0;
    for (int t = 0; t < 9; ++t) {
      CHECK(pm::live_count(wm, t) >= 2, "a tap with fewer than two live fragments");
      by_tap += pm::live_count(wm, t);
    }
    CHECK(by_tap == live_wm[wm], "live_count sums");
  }
  bool seen[pm::kImg] = {};
  for (int wm = 0; wm < pm::kWM; ++wm)
    for (int i = 0; i < pm::kTM; ++i) {
      CHECK(!seen[pm::frag_pos(wm, i)], "position %d twice", pm::frag_pos(wm, i));
      seen[pm::frag_pos(wm, i)] = true;
    }
  std::printf("live (fragment, tap) pairs per wave row: %d %d %d %d of 36\n", live_wm[0], live_wm[1],
              live_wm[2], live_wm[3]);
  CHECK(live_wm[0] == 26 && live_wm[1] == 25 && live_wm[2] == 24 && live_wm[3] == 25, "live counts");
  // waves wid and wid + 4 share a SIMD: wave rows wm and wm + 2 (WN = 2)
  for (int wm = 0; wm < 2; ++wm)
    CHECK(live_wm[wm] + live_wm[wm + 2] == 50, "SIMD %d: %d live pairs", wm,
          live_wm[wm] + live_wm[wm + 2]);
}

// ------------------------------------------------------------- (b) the kernel's maps
// x [B][16][C], w [CO][9][C] small integers; C = BK (one chunk), CO = 16 (one
// fragment column).  flip: the data gradient's mirrored weight tap.
static void check_conv(int B, bool flip) {
  const HaloPlan plan = plan_halo_pm(kCfg, pm::kH, pm::kW, BK, 3, 3, 1, 1);
  CHECK(plan.ok, "plan_halo_pm refuses the 4 x 4 map");
  if (!plan.ok) return;
  const HaloGeom& g = plan.g;
  CHECK(g.MV == pm::kBM && g.TB == pm::kTB && g.TH == pm::kH && g.PI == pm::kPI &&
            g.HROWS == pm::kRows && g.A_INS == pm::kPieces && g.PSW == 0,
        "plan geometry");
  const size_t stage_el = (size_t)g.A_INS * RPI * BK + (size_t)9 * plan.c.bn * BK;
  CHECK(plan.lds >= (size_t)plan.c.ns * stage_el * 2, "ring does not fit the plan's LDS");
  CHECK(plan.lds >= (size_t)pm::epi_elems(plan.c.bn) * 2, "epilogue tile does not fit");

  constexpr int C = BK, CO = 16;
  const int M = B * pm::kImg;
  std::vector<int> x((size_t)M * C), w((size_t)CO * 9 * C), y((size_t)M * CO, -12345),
      ref((size_t)M * CO, 0);
  unsigned s = 12345u + (unsigned)B * 2u + (flip ? 1u : 0u);
  auto rnd = [&] { s = s * 1664525u + 1013904223u; return (int)((s >> 24) % 7) - 3; };
  for (auto& v : x) v = rnd();
  for (auto& v : w) v = rnd();
  // direct conv
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < pm::kH; ++h)
      for (int ww = 0; ww < pm::kW; ++ww)
        for (int co = 0; co < CO; ++co) {
          int acc = 0;
          for (int t = 0; t < 9; ++t) {
            const int hh = h + t / 3 - 1, w2 = ww + t % 3 - 1;
            if (hh < 0 || hh >= pm::kH || w2 < 0 || w2 >= pm::kW) continue;
            const int wt = flip ? 8 - t : t;
            for (int c = 0; c < C; ++c)
              acc += x[((size_t)(b * pm::kImg + hh * pm::kW + w2)) * C + c] *
                     w[((size_t)co * 9 + wt) * C + c];
          }
          ref[((size_t)(b * pm::kImg + h * pm::kW + ww)) * CO + co] = acc;
        }
  std::vector<int> written((size_t)M, 0);
  const int tiles = (M + g.MV - 1) / g.MV;
  for (int tile = 0; tile < tiles; ++tile) {
    const int m0 = tile * g.MV, b0 = m0 / pm::kImg;
    // stage: LDS image [rows][physical chunk][8], lane-linear DMA pieces
    std::vector<int> lds((size_t)g.A_INS * RPI * BK, 777);
    for (int ins = 0; ins < g.A_INS; ++ins)
      for (int lane = 0; lane < 64; ++lane) {
        const int row = ins * RPI + lane / CPR, pc = lane % CPR;
        CHECK(row < g.HROWS, "DMA row %d past the staged image", row);
        const int tb = pm::row_tb(row), p = pm::row_p(row);
        CHECK(tb < g.TB, "DMA row %d: image %d", row, tb);
        const bool ok = p < pm::kImg && b0 + tb < B;
        const int lc = pm::swz(tb, pc);   // the logical chunk this lane fetches
        CHECK(lc >= 0 && lc < CPR && pm::swz(tb, lc) == pc, "swizzle is no involution");
        for (int e = 0; e < 8; ++e)
          lds[((size_t)row * CPR + pc) * 8 + e] =
              ok ? x[((size_t)((b0 + tb) * pm::kImg + p)) * C + lc * 8 + e] : 0;
      }
    // compute: wave row wm, fragment i, live taps in order; lane = (row tb, k-chunk kc)
    std::vector<int> acc((size_t)pm::kBM * CO, 0);
    for (int wm = 0; wm < pm::kWM; ++wm)
      for (int i = 0; i < pm::kTM; ++i)
        for (int t = 0; t < 9; ++t) {
          if (!pm::live(wm, i, t)) continue;
          const int wt = flip ? 8 - t : t;
          for (int lane = 0; lane < 64; ++lane) {
            const int tb = lane & 15, kc = lane >> 4;
            const int row = pm::staged_row(tb, pm::frag_pos(wm, i)) + pm::tap_shift(t);
            CHECK(row >= 0 && row < g.HROWS && pm::row_tb(row) == tb && pm::row_p(row) < pm::kImg,
                  "fragment (%d, %d) tap %d reads row %d", wm, i, t, row);
            if (row < 0 || row >= g.HROWS) continue;
            const int pc = pm::swz(tb, kc);
            const int ml = wm * 64 + i * 16 + tb;
            for (int co = 0; co < CO; ++co)
              for (int e = 0; e < 8; ++e)
                acc[(size_t)ml * CO + co] += lds[((size_t)row * CPR + pc) * 8 + e] *
                                             w[((size_t)co * 9 + wt) * C + kc * 8 + e];
          }
        }
    // epilogue
    bool hit[pm::kBM] = {};
    for (int ml = 0; ml < pm::kBM; ++ml) {
      const int op = pm::out_pixel(ml);
      CHECK(op >= 0 && op < pm::kBM && !hit[op], "out_pixel(%d) = %d", ml, op);
      if (op < 0 || op >= pm::kBM) continue;
      hit[op] = true;
      const int m = m0 + op;
      if (m >= M) continue;
      ++written[m];
      for (int co = 0; co < CO; ++co) y[(size_t)m * CO + co] = acc[(size_t)ml * CO + co];
    }
  }
  int bad = 0;
  for (int m = 0; m < M; ++m) {
    if (written[m] != 1) ++bad;
    for (int co = 0; co < CO; ++co) bad += y[(size_t)m * CO + co] != ref[(size_t)m * CO + co];
  }
  CHECK(bad == 0, "conv B=%d flip=%d: %d wrong outputs", B, (int)flip, bad);
}

// ------------------------------------------------------------- (c) bank conflicts
// ds_read_b128: 64 banks of 4 B (a 256-B row = 16 slots of 16 B), served in four
// 16-lane groups; a group is conflict-free iff its lanes hit 16 distinct slots
static const int kB128Groups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

static int check_read_conflicts() {
  int worst = 1, reads = 0;
  for (int wm = 0; wm < pm::kWM; ++wm)
    for (int i = 0; i < pm::kTM; ++i)
      for (int t = 0; t < 9; ++t) {
        if (!pm::live(wm, i, t)) continue;
        ++reads;
        for (const auto& grp : kB128Groups) {
          int slots[16] = {};
          for (int lane : grp) {
            const int tb = lane & 15, kc = lane >> 4;
            const int row = pm::staged_row(tb, pm::frag_pos(wm, i)) + pm::tap_shift(t);
            const int byte = row * (BK * 2) + pm::swz(tb, kc) * 16;
            const int d = ++slots[(byte / 16) % 16];
            if (d > worst) worst = d;
          }
        }
      }
  CHECK(reads == 100, "live reads: %d", reads);
  CHECK(worst == 1, "A-fragment ds_read_b128: %d-way bank conflict", worst);
  return worst;
}

// ds_write_b64 of the row epilogue's phase 1 (32 banks of 4 B, four groups of 16
// consecutive lanes; a lane writes 8 B at tile row (lane & 15), channels
// 4 * (lane >> 4)): the worst degree with the PM rows + skew must not exceed the
// dense tile's (16 consecutive rows)
static void check_write_conflicts(int bn) {
  const int pitch = bn + 8;
  int worst_pm = 1, worst_dense = 1;
  for (int wm = 0; wm < pm::kWM; ++wm)
    for (int i = 0; i < pm::kTM; ++i)
      for (int grp = 0; grp < 4; ++grp) {
        int pmb[32] = {}, deb[32] = {};
        for (int l = 0; l < 16; ++l) {
          const int ml = wm * 64 + i * 16 + l, nl = 4 * grp;
          const int mr = pm::out_pixel(ml);
          const int a_pm = (mr * pitch + (mr >> 4) * pm::kEpiSkew + nl) * 2;
          const int a_de = (ml * pitch + nl) * 2;
          for (int k = 0; k < 2; ++k) {
            const int dp = ++pmb[(a_pm / 4 + k) % 32], dd = ++deb[(a_de / 4 + k) % 32];
            if (dp > worst_pm) worst_pm = dp;
            if (dd > worst_dense) worst_dense = dd;
          }
        }
      }
  std::printf("row epilogue ds_write_b64 (BN %d): PM %d-way, dense %d-way\n", bn, worst_pm,
              worst_dense);
  CHECK(worst_pm <= worst_dense, "PM epilogue writes conflict more than the dense tile's");
  // phase 2 reads 16-B segments: the skew keeps them aligned
  CHECK((pm::kEpiSkew * 2) % 16 == 0 && (pitch * 2) % 16 == 0, "row segments not 16-B aligned");
}

int main() {
  check_validity();
  // the plan applies where it should and nowhere else
  CHECK(plan_halo_pm(kCfg, 4, 4, 512, 3, 3, 1, 1).ok, "cfg %d at 4 x 4", kCfg);
  CHECK(!plan_halo_pm(kCfg, 8, 8, 512, 3, 3, 1, 1).ok, "8 x 8 accepted");
  CHECK(!plan_halo_pm(kCfg, 4, 4, 512, 3, 3, 2, 1).ok, "stride 2 accepted");
  CHECK(!plan_halo_pm(kCfg, 4, 4, 512, 1, 1, 1, 0).ok, "1 x 1 accepted");
  CHECK(!plan_halo_pm(kCfg, 4, 4, 48, 3, 3, 1, 1).ok, "C %% 32 != 0 accepted");
  for (int cfg = kHaloBase; cfg < kHaloBase + kNumHaloConfigs; ++cfg) {
    const HaloPlan q = plan_halo_pm(cfg, 4, 4, 512, 3, 3, 1, 1);
    CHECK(q.ok == halo_pm_cfg(cfg), "cfg %d", cfg);
    // a PM plan only replaces a dense plan of the same id
    if (q.ok) CHECK(plan_halo(cfg, 4, 4, 512, 3, 3, 1, 1, true).ok, "cfg %d: no dense plan", cfg);
  }
  for (int B : {1, 16, 17})
    for (bool flip : {false, true}) check_conv(B, flip);
  const int deg = check_read_conflicts();
  check_write_conflicts(64);
  std::printf("halo_pm_check: %lld checks, %d failed, A-read conflict degree %d\n", g_checks,
              g_failed, deg);
  return g_failed ? 1 : 0;
}
