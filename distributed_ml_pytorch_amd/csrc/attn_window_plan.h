// Host-side plan of the shifted-window attention kernels (attention_window.hip).
// plan_window_attention turns (batch, map, heads, window side, shift) into the
// live strip count, the persistent grid, the LDS bytes of the two kernels and
// the partial-row count of the bias-table gradient slab, or refuses the shape.
// Plain C++ (no torch, no HIP), in the manner of attn_plan.h: the launchers and
// the bindings' argument check both use it.
#pragma once

#include <cstddef>

namespace dmp {

constexpr int kWinHeadDim = 32;          // one k-step of v_mfma_f32_16x16x32_bf16
constexpr int kWinMaxTokens = 64;        // N = ws * ws: the 64 x 64 score tile of one wave
constexpr int kWinStrip = 16;            // tokens per strip (one MFMA tile side)
constexpr int kWinRowStride = kWinHeadDim + 8;   // elements per LDS image row ([token][40] bf16)
constexpr int kWinWaves = 4;             // waves per workgroup, one (window, head) each
constexpr int kWinMaxBlocks = 512;       // persistent grid cap: 2 workgroups on each of 256 CUs
constexpr int kWinMaxHeads = 1024;
constexpr float kWinMaskValue = -100.0f; // added to scores across regions of a shifted window
constexpr int kWinLabelShift = 12;       // token code = ty * (2 ws - 1) + tx + (region << 12)

constexpr size_t kWinImageBytes = (size_t)kWinMaxTokens * kWinRowStride * 2;   // 5120
// per wave: token codes + pixel indices (64 ints each) and the bias column, padded
constexpr size_t win_side_bytes(int T) { return (size_t)(2 * kWinMaxTokens + ((T + 3) & ~3)) * 4; }

struct WinAttnPlan {
  bool ok;
  int N, T;            // tokens per window, bias-table rows (2 ws - 1)^2
  int strips;          // live 16-token strips: ceil(N / 16)
  long long windows;   // B * (Hm / ws) * (Wm / ws)
  long long items;     // windows * heads, one wave pass each
  int grid;            // workgroups; grid * kWinWaves is a multiple of heads
  int rows;            // waves per head = partial rows of the dtable slab
  size_t lds_fwd, lds_bwd;   // bytes per workgroup
};

inline int win_gcd(int a, int b) { return b == 0 ? a : win_gcd(b, a % b); }

// Wave w of the grid owns head w % heads for its whole life and the windows
// w / heads, w / heads + rows, ...: one head per wave lets the bias column stay
// in LDS and the dS sums stay in registers across windows, and the waves of a
// workgroup work on neighbouring heads of the same window.
inline WinAttnPlan plan_window_attention(long long B, int Hm, int Wm, int heads, int ws, int sh) {
  WinAttnPlan p{};
  if (B < 1 || Hm < 1 || Wm < 1 || heads < 1 || heads > kWinMaxHeads || ws < 1) return p;
  if (ws * ws > kWinMaxTokens || sh < 0 || sh >= ws || Hm % ws || Wm % ws) return p;
  p.N = ws * ws;
  p.T = (2 * ws - 1) * (2 * ws - 1);
  p.strips = (p.N + kWinStrip - 1) / kWinStrip;
  p.windows = B * (Hm / ws) * (Wm / ws);
  p.items = p.windows * heads;
  const long long lim = 0x7fffffffLL;
  // pixel indices and item counts are ints in the kernels
  if (B * Hm * Wm > lim / 4 || p.items > lim / 4) return p;
  const int m = heads / win_gcd(heads, kWinWaves);   // grid must be a multiple of m
  long long need = (p.items + kWinWaves - 1) / kWinWaves;
  if (need > kWinMaxBlocks) need = kWinMaxBlocks;
  p.grid = (int)((need + m - 1) / m) * m;
  p.rows = p.grid * kWinWaves / heads;
  p.lds_fwd = kWinWaves * (kWinImageBytes + win_side_bytes(p.T));
  // three images (K, Q, dO) overlaid by the [64][64] fp32 fold tile, + lse2 / Di rows
  p.lds_bwd = kWinWaves * ((size_t)kWinMaxTokens * kWinMaxTokens * 4 + win_side_bytes(p.T) +
                           (size_t)2 * kWinMaxTokens * 4);
  p.ok = true;
  return p;
}

}  // namespace dmp
