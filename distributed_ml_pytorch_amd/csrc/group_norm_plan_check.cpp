// Checks the GroupNorm planner (group_norm_plan.h) for tests/test_group_norm_cpu.py.
// Stand-alone: any host C++17 compiler, no HIP, no torch.  Enumerates the test
// geometries and every ResNet-18 / 34 / 50 map (CIFAR and ImageNet stems, G = 32)
// at batches 1..512, forward and backward, all three route requests, and checks
// every accepted plan; then that geometries outside coverage are refused.
// Prints "group_norm_plan_check: <checks> checks, <failed> failed" and one
// "plan ..." line for each geometry of the bench table.
#include <cstdio>

#include "group_norm_plan.h"

static long long g_checks = 0, g_failed = 0;

#define EXPECT(cond, ...)                 \
  do {                                    \
    ++g_checks;                           \
    if (!(cond)) {                        \
      ++g_failed;                         \
      std::printf("FAIL: " __VA_ARGS__);  \
      std::printf("\n");                  \
    }                                     \
  } while (0)

static void check_plan(long long N, int C, int H, int W, int G, int route, bool bwd) {
  const long long HW = (long long)H * W;
  const dmp::GnPlan p = dmp::plan_group_norm(N, C, HW, G, route, bwd);
  if (!p.ok) {
    // automatic and streaming requests of these geometries always have a plan
    EXPECT(route == 0, "N %lld C %d HW %lld G %d route %d bwd %d refused", N, C, HW, G, route, bwd);
    return;
  }
  const int cpg = C / G, SC = p.SV * dmp::kGnVec;
  EXPECT(route < 0 || p.route == route, "forced route %d became %d", route, p.route);
  EXPECT(p.cpg == cpg && SC % cpg == 0 && p.GS * cpg == SC, "C %d G %d: slice of %d channels", C,
         G, SC);
  EXPECT(p.CV * dmp::kGnVec == C && p.slices * p.SV == p.CV, "C %d: %d slices of %d vectors", C,
         p.slices, p.SV);
  EXPECT(p.PR >= 1 && p.T == p.PR * p.SV && p.T <= dmp::kGnThreads, "SV %d: %d live lanes", p.SV,
         p.T);
  EXPECT(p.lds_bytes <= dmp::kGnLdsMax && p.lds_apply <= dmp::kGnLdsMax, "C %d HW %lld: LDS %d / %d",
         C, HW, p.lds_bytes, p.lds_apply);
  // the parts cover the pixels exactly once; a lane's staged vectors fit its slots
  EXPECT(p.parts >= 1 && p.parts <= dmp::kGnMaxParts && (long long)p.parts * p.PP >= HW &&
             (long long)(p.parts - 1) * p.PP < HW,
         "HW %lld: %d parts of %d", HW, p.parts, p.PP);
  EXPECT((long long)p.IT * p.PR >= p.PP, "PP %d: %d rows x %d items", p.PP, p.PR, p.IT);
  EXPECT(p.route == 1 || p.parts == 1, "resident plan with %d parts", p.parts);
  const bool staged = p.route == 0 || !bwd;
  const dmp::GnLds l = dmp::gn_lds(p.T, staged ? p.IT : 0, SC, p.GS,
                                   staged ? (bwd ? 2 : 1) : 0, bwd ? 2 : 1);
  EXPECT(l.bytes == p.lds_bytes && l.chan % 8 == 0 && l.grp % 8 == 0 && l.tot % 8 == 0 &&
             l.dz % 16 == 0, "LDS image %d vs plan %d", l.bytes, p.lds_bytes);
  EXPECT(p.grid[0] == p.slices && p.grid[1] == p.parts && p.grid[0] <= 256 &&
             p.grid[2] >= 1 && p.grid[2] <= dmp::kGnMaxBatch, "grid %d %d %d", p.grid[0], p.grid[1],
         p.grid[2]);
  if (bwd) {
    EXPECT(p.NR >= 1 && p.NR <= N && p.grid[2] == p.NR && p.slab_rows == p.NR * p.parts &&
               p.slab_rows <= dmp::gn_slab_rows(C) &&
               (long long)p.slab_rows * 2 * C <= dmp::gn_slab_floats(C),
           "C %d: %d slab rows of %d", C, p.slab_rows, dmp::gn_slab_rows(C));
  } else {
    EXPECT(p.grid[2] == N, "forward grid z %d for N %lld", p.grid[2], N);
  }
}

static void check_all_routes(long long N, int C, int H, int W, int G) {
  for (int route = -1; route <= 1; ++route)
    for (int bwd = 0; bwd < 2; ++bwd) check_plan(N, C, H, W, G, route, bwd != 0);
}

int main() {
  // the cells of tests/test_group_norm_gpu.py
  const int cells[][5] = {{2, 64, 4, 4, 32}, {3, 32, 7, 7, 8},   {2, 64, 5, 3, 8},
                          {2, 96, 7, 7, 4},  {1, 128, 2, 2, 1},  {2, 16, 1, 1, 16},
                          {2, 64, 33, 17, 32}, {1, 64, 112, 112, 32}};
  for (const auto& c : cells) check_all_routes(c[0], c[1], c[2], c[3], c[4]);
  // ResNet-18 / 34 (CIFAR stem), ResNet-50 (ImageNet and CIFAR stems): (side, C)
  const int maps[][2] = {{32, 64},  {16, 128},  {8, 256},   {4, 512},   {112, 64}, {56, 64},
                         {56, 128}, {56, 256},  {28, 128},  {28, 256},  {28, 512}, {14, 256},
                         {14, 512}, {14, 1024}, {7, 512},   {7, 1024},  {7, 2048}, {32, 256},
                         {16, 256}, {16, 512},  {8, 512},   {8, 1024},  {4, 1024}, {4, 2048}};
  for (const auto& m : maps)
    for (long long N = 1; N <= 512; ++N) {
      if (N * m[0] * m[0] * m[1] * 2 >= (1ll << 31)) continue;   // refused below
      check_all_routes(N, m[1], m[0], m[0], 32);
    }
  // routes of the design note: the 112 x 112 stem map streams, CIFAR maps stay on chip
  EXPECT(dmp::plan_group_norm(1, 64, 112 * 112, 32, -1, false).route == 1, "112x112x64 resident");
  EXPECT(!dmp::plan_group_norm(1, 64, 112 * 112, 32, 0, false).ok, "112x112x64 forced resident");
  EXPECT(dmp::plan_group_norm(512, 64, 32 * 32, 32, -1, false).route == 0, "32x32x64 streams");
  EXPECT(dmp::plan_group_norm(512, 64, 32 * 32, 32, -1, true).route == 0, "32x32x64 bwd streams");
  const dmp::GnPlan rag = dmp::plan_group_norm(2, 64, 33 * 17, 32, 1, false);
  EXPECT(rag.ok && rag.parts >= 2 && 33 * 17 % rag.PP != 0, "33x17 stream: %d parts", rag.parts);
  // refusals
  EXPECT(!dmp::plan_group_norm(2, 24, 16, 8, -1, false).ok, "cpg 3 accepted");
  EXPECT(!dmp::plan_group_norm(2, 20, 16, 5, -1, false).ok, "C %% 8 != 0 accepted");
  EXPECT(!dmp::plan_group_norm(2, 4096, 16, 32, -1, false).ok, "C 4096 accepted");
  EXPECT(!dmp::plan_group_norm(2, 48, 16, 8, -1, false).ok, "cpg 6 accepted");
  EXPECT(!dmp::plan_group_norm(0, 64, 16, 32, -1, false).ok, "N 0 accepted");
  EXPECT(!dmp::plan_group_norm(70000, 64, 1, 32, -1, false).ok, "N over the grid accepted");
  EXPECT(!dmp::plan_group_norm(512, 64, 224 * 224, 32, -1, false).ok, "3 GiB tensor accepted");
  EXPECT(!dmp::plan_group_norm(1, 64, 1ll << 22, 32, -1, false).ok, "part over the LDS accepted");
  EXPECT(dmp::gn_slab_floats(64) == 256ll * 2 * 64 && dmp::gn_slab_rows(2048) == 64, "slab size");

  const int bench[][3] = {{512, 32, 64},  {512, 16, 128}, {512, 8, 256},   {512, 4, 512},
                          {128, 112, 64}, {128, 56, 64},  {128, 56, 256},  {128, 28, 512},
                          {128, 14, 1024}, {128, 7, 2048}};
  for (const auto& b : bench)
    for (int bwd = 0; bwd < 2; ++bwd) {
      const dmp::GnPlan p = dmp::plan_group_norm(b[0], b[2], b[1] * b[1], 32, -1, bwd != 0);
      std::printf("plan N %d %dx%dx%d %s: %s slice %d ch, %d parts of %d px, lds %d, grid %d %d %d\n",
                  b[0], b[1], b[1], b[2], bwd ? "bwd" : "fwd", p.route ? "stream" : "resident",
                  p.SV * dmp::kGnVec, p.parts, p.PP, p.lds_bytes, p.grid[0], p.grid[1], p.grid[2]);
    }
  std::printf("group_norm_plan_check: %lld checks, %lld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
