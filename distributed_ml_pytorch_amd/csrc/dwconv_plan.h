// Host-side plan of the depthwise conv kernels (dwconv.hip): tile sizes, LDS
// pitches and grids for a (H, W, C, K) geometry.  Plain C++ (no torch, no HIP),
// in the manner of halo_plan.h / attn_plan.h: the launchers, the bindings and
// the tests' multi-tile check all read the same function.
#pragma once

#include <cstdint>

namespace dmp {

constexpr int kDwThreads = 256;
constexpr int kDwRun = 4;                    // consecutive outputs along W a lane owns
constexpr int kDwVec = 8;                    // channels a lane owns (one 16-byte vector)
constexpr int kDwMaxTile = 32;               // most output rows / columns of a tile
constexpr int kDwLdsBudget = 48 * 1024;      // per workgroup: three fit the CU's 160 KiB
constexpr int kDwBankRow = 256;              // bytes the LDS serves per cycle (64 banks x 4 B)

// weight-gradient kernel: a lane owns kDwWgVec channels of one tap row
constexpr int kDwWgVec = 4;
constexpr int kDwWgChunk = 32;               // channels per workgroup
constexpr int kDwWgMaxParts = 1024;          // most slab partials (workgroups) of one launch

inline bool dw_kernel_ok(int K) { return K == 3 || K == 5 || K == 7; }

struct DwPlan {
  bool ok;
  int TH, TW, CC;              // output tile and channel chunk of a workgroup
  int tiles_h, tiles_w, chunks;
  int pitch;                   // bytes between staged pixels (CC * 2 + pad)
  int rowpitch;                // bytes between staged rows ((TW + K - 1) * pitch + pad)
  int lds_bytes;               // taps [K*K][CC] fp32, then the staged tile
};

// bytes between staged pixels of a CC-channel chunk.  A ds_read_b128 is served 16
// lanes at a time, one 256-byte bank row per cycle; those 16 lanes are CC / 8
// adjacent channel vectors of consecutive pixel runs (kDwRun pixels apart) and,
// where a tile row has fewer than 16 lanes, of consecutive tile rows.  The pixel
// pad makes kDwRun * pitch step by 64 bytes (32 channels) or 128 bytes (64)
// modulo 256, so the runs of one row fall on distinct 16-byte granules; the row
// pad (dw_row_pad) does the same for the rows.
inline int dw_pitch(int CC) { return CC * 2 + (CC == 64 ? 32 : 16); }

// the worst number of lanes of one 16-lane group that share a 16-byte granule
// of the bank row, for the forward kernel's window reads under `p` (first round
// of work items; 1 = conflict-free)
inline int dw_read_ways(const DwPlan& p) {
  const int CV = p.CC / kDwVec, runs = p.TW / kDwRun;
  const int items = CV * runs * p.TH < kDwThreads ? CV * runs * p.TH : kDwThreads;
  int worst = 1;
  for (int base = 0; base < items; base += 16) {
    int hits[kDwBankRow / 16] = {0};
    for (int l = base; l < base + 16 && l < items; ++l) {
      const int cv = l % CV, run = (l / CV) % runs, row = l / CV / runs;
      const long long a = (long long)row * p.rowpitch + (long long)run * kDwRun * p.pitch + cv * 16;
      const int w = ++hits[(a % kDwBankRow) / 16];
      if (w > worst) worst = w;
    }
  }
  return worst;
}

// the row pad (a multiple of 16 bytes, under one bank row) with the fewest ways.
// Over H, W in 1..64, K in {3, 5, 7} and C in {8, ..., 768} (147,456 plans) every
// plan of 32 or more channels per chunk comes out at 1 way; the 8- and
// 16-channel chunks of C < 32, whose pixel pitch cannot be padded off the bank
// row at 16-byte alignment, at up to 4.
inline void dw_row_pad(DwPlan& p, int K) {
  const int tight = (p.TW + K - 1) * p.pitch;
  int best_pad = 0, best_ways = 1 << 30;
  for (int pad = 0; pad < kDwBankRow && best_ways > 1; pad += 16) {
    p.rowpitch = tight + pad;
    const int w = dw_read_ways(p);
    if (w < best_ways) best_ways = w, best_pad = pad;
  }
  p.rowpitch = tight + best_pad;
  p.lds_bytes = K * K * p.CC * 4 + (p.TH + K - 1) * p.rowpitch;
}

// Tile search: every (TH, TW, CC) with TW a multiple of kDwRun, within the LDS
// budget; the cost is lane slots (a workgroup runs whole rounds of 256 work
// items, so a 7 x 7 map takes a wide channel chunk instead of idle lanes) plus
// the halo's staging traffic.  Tiles divide the map evenly where they can: the
// candidates are ceil(H / n) and ceil4(W / n).
inline DwPlan plan_dwconv(int H, int W, int C, int K) {
  DwPlan best{};
  if (H < 1 || W < 1 || C < 8 || C % 8 || !dw_kernel_ok(K)) return best;
  double best_cost = 0;
  const int cmax = C >= 32 ? 128 : 16;
  for (int CC = C >= 32 ? 32 : 8; CC <= cmax; CC *= 2) {
    if (CC > 32 && CC > (C + 31) / 32 * 32) break;
    const int chunks = (C + CC - 1) / CC;
    for (int nh = (H + kDwMaxTile - 1) / kDwMaxTile; nh <= H; ++nh) {
      const int TH = (H + nh - 1) / nh;
      if (TH > kDwMaxTile) continue;
      if (nh > 1 && (H + nh - 2) / (nh - 1) == TH) {              // same TH with fewer tiles
        if (TH == 1) break;
        continue;
      }
      for (int nw = (W + kDwMaxTile - 1) / kDwMaxTile; nw <= W; ++nw) {
        const int TW = ((W + nw - 1) / nw + kDwRun - 1) / kDwRun * kDwRun;
        if (TW > kDwMaxTile) continue;
        const int tiles_w = (W + TW - 1) / TW;
        if (tiles_w != nw) continue;
        const int pitch = dw_pitch(CC);
        const int lds = K * K * CC * 4 + (TH + K - 1) * ((TW + K - 1) * pitch + kDwBankRow);
        if (lds > kDwLdsBudget) continue;                          // (any row pad fits)
        const long long items = (long long)(CC / kDwVec) * (TW / kDwRun) * TH;
        const long long rounds = (items + kDwThreads - 1) / kDwThreads;
        const long long stage = (long long)(TH + K - 1) * (TW + K - 1) * (CC / kDwVec);
        const double wgs = (double)nh * nw * chunks;
        const double cost = wgs * (rounds * kDwThreads * (K * K * 36.0 + K * 110.0) +
                                   stage * 24.0 + 4096.0);
        if (!best.ok || cost < best_cost) {
          best = DwPlan{true, TH, TW, CC, nh, nw, chunks, pitch, 0, lds};
          best_cost = cost;
        }
        if (TW <= kDwRun) break;
      }
    }
  }
  if (best.ok) dw_row_pad(best, K);
  return best;
}

// ------------------------------------------------------------ weight gradient
// A workgroup stages a THW x TWW tile of dy and the x tile with its halo for 32
// channels; lane = (4-channel group, tap row, row group).  TWW is a multiple of
// K: the sliding window is unrolled K times so that it rotates through
// registers without moves.  Rows of the x image are an odd number of 64-byte
// pixels apart, so lanes of consecutive tap rows read distinct bank-row quarters.
struct DwWgPlan {
  bool ok;
  int TH, TW;                  // dy tile
  int row_groups;              // RG = 256 / (8 * K)
  int tiles_h, tiles_w, chunks;
  int parts;                   // workgroups per chunk = slab partials per chunk that are
                               // written and read; the slab holds dw_slab_parts() of them
  int xrow, dyrow;             // bytes between staged rows
  int lds_bytes;               // max(staging, the RG-way reduction image)
};

// slab partials per chunk: the most workgroups per chunk of any launch
inline int dw_slab_parts(int chunks) {
  return kDwWgMaxParts / chunks > 0 ? kDwWgMaxParts / chunks : 1;
}

inline DwWgPlan plan_dwconv_wgrad(long long N, int H, int W, int C, int K) {
  DwWgPlan p{};
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || !dw_kernel_ok(K)) return p;
  const int pix = kDwWgChunk * 2;
  p.row_groups = kDwThreads / (kDwWgChunk / kDwWgVec * K);
  const int mw = (W + K - 1) / K, mcap = kDwMaxTile / K;
  p.TW = K * (mw < mcap ? mw : mcap);
  p.xrow = ((p.TW + K - 1) | 1) * pix;
  p.dyrow = p.TW * pix;
  p.TH = H < 2 * p.row_groups ? H : 2 * p.row_groups;
  while (p.TH > 1 && (p.TH + K - 1) * p.xrow + p.TH * p.dyrow > kDwLdsBudget) --p.TH;
  p.tiles_h = (H + p.TH - 1) / p.TH;
  p.tiles_w = (W + p.TW - 1) / p.TW;
  p.chunks = (C + kDwWgChunk - 1) / kDwWgChunk;
  const long long tiles = N * p.tiles_h * p.tiles_w;
  const long long cap = dw_slab_parts(p.chunks);
  p.parts = (int)(tiles < cap ? tiles : cap);
  const int stage = (p.TH + K - 1) * p.xrow + p.TH * p.dyrow;
  const int red = p.row_groups * (K * K + 1) * kDwWgChunk * 4;
  p.lds_bytes = stage > red ? stage : red;
  p.ok = p.lds_bytes <= 64 * 1024;
  return p;
}

// floats of the persistent per-layer slab, [chunks][dw_slab_parts][K*K + 1][32]:
// a function of (C, K) alone.  It must not grow with the batch or the map: a
// captured step holds the slab's address, and an evaluation at another batch
// size runs the same layer.
inline long long dwconv_slab_floats(int C, int K) {
  const int chunks = (C + kDwWgChunk - 1) / kDwWgChunk;
  return (long long)chunks * dw_slab_parts(chunks) * (K * K + 1) * kDwWgChunk;
}

}  // namespace dmp
