// Host-side plan of the fused attention kernels (attention.hip: the resident
// route, attention_stream.hip: the streaming route).  plan_attention turns
// (tokens N, batch * heads, route request) into the route, the block counts,
// the tile sizes, the LDS bytes of each kernel and the grids, or refuses what no
// route takes.  Plain C++ (no torch, no HIP), in the manner of halo_plan.h: the
// launchers and the bindings' argument check use it, the sanitizer driver
// (host_check.cpp, `make asan`) and attn_plan_check.cpp run it on a CPU.
#pragma once

#include <cstddef>

namespace dmp {

constexpr int kAttnHeadDim = 64;
constexpr int kAttnRowStride = kAttnHeadDim + 8;   // elements per staged LDS row ([token][72] bf16)
constexpr int kAttnStrip = 16;                     // tokens per wave strip (one MFMA tile side)
constexpr int kAttnLdsLimit = 160 * 1024;          // LDS of a CU

// resident route: a head's whole K/V (or Q/dO) set staged once, one workgroup
// per (batch, head), rows padded to 32
constexpr int kAttnResidentMax = 256;
// streaming route: a workgroup of kAttnStreamWaves waves owns one 16-token strip
// per wave (kAttnStreamBlock tokens) and streams double-buffered tiles of
// kAttnStreamTile tokens of the other operand through LDS
constexpr int kAttnStreamWaves = 8;
constexpr int kAttnStreamBlock = kAttnStrip * kAttnStreamWaves;   // 128
constexpr int kAttnStreamTile = 128;
constexpr int kAttnStreamStages = 2;
constexpr int kAttnStreamMax = 4096;

enum AttnRoute { kAttnAuto = -1, kAttnResident = 0, kAttnStream = 1 };

struct AttnPlan {
  bool ok;
  int route;                  // kAttnResident or kAttnStream
  int waves;                  // waves per workgroup, every kernel
  int q_block, k_block;       // tokens a workgroup owns: forward / dQ, dK / dV
  int q_blocks, k_blocks;     // workgroups per (batch, head): forward / dQ, dK / dV
  int k_tile, q_tile;         // tokens per staged tile: forward / dQ (keys), dK / dV (queries)
  int k_tiles, q_tiles;       // staged tiles per workgroup
  int stages;                 // LDS images of a tile in flight
  size_t lds_fwd, lds_dq, lds_dkv;
  long long grid_fwd, grid_dq, grid_dkv;   // workgroups (1-D grids)
};

// two row-major [rows][72] bf16 images
constexpr size_t attn_image_pair_bytes(int rows) {
  return (size_t)2 * rows * kAttnRowStride * 2;
}

// Plan of N tokens for bh = batch * heads (batch, head) pairs.  request: kAttnAuto
// (resident up to kAttnResidentMax tokens, streaming above), kAttnResident or
// kAttnStream.  !ok: N < 1, N past the route's cap, an unknown request, bh < 1 or
// a grid past 2^31 - 1.
inline AttnPlan plan_attention(int N, int request, long long bh = 1) {
  AttnPlan p{};
  const long long lim = 0x7fffffffLL;
  if (N < 1 || bh < 1 || bh > lim || request < kAttnAuto || request > kAttnStream) return p;
  p.route = request == kAttnAuto ? (N <= kAttnResidentMax ? kAttnResident : kAttnStream) : request;
  p.waves = kAttnStreamWaves;
  if (p.route == kAttnResident) {
    if (N > kAttnResidentMax) return p;
    const int NP = (N + 31) & ~31;
    p.q_block = p.k_block = p.k_tile = p.q_tile = NP;
    p.q_blocks = p.k_blocks = p.k_tiles = p.q_tiles = 1;
    p.stages = 1;
    p.lds_fwd = p.lds_dq = attn_image_pair_bytes(NP);
    p.lds_dkv = p.lds_fwd + (size_t)2 * NP * 4;   // + lse2 / Di rows
  } else {
    if (N > kAttnStreamMax) return p;
    p.q_block = p.k_block = kAttnStreamBlock;
    p.k_tile = p.q_tile = kAttnStreamTile;
    p.q_blocks = p.k_blocks = (N + kAttnStreamBlock - 1) / kAttnStreamBlock;
    p.k_tiles = p.q_tiles = (N + kAttnStreamTile - 1) / kAttnStreamTile;
    p.stages = kAttnStreamStages;
    p.lds_fwd = p.lds_dq = (size_t)p.stages * attn_image_pair_bytes(kAttnStreamTile);
    p.lds_dkv = (size_t)p.stages * (attn_image_pair_bytes(kAttnStreamTile) +
                                    (size_t)2 * kAttnStreamTile * 4);
  }
  p.grid_fwd = p.grid_dq = bh * p.q_blocks;
  p.grid_dkv = bh * p.k_blocks;
  p.ok = p.grid_fwd <= lim && p.grid_dkv <= lim && p.lds_fwd <= (size_t)kAttnLdsLimit &&
         p.lds_dkv <= (size_t)kAttnLdsLimit;
  return p;
}

// most tokens any route takes
constexpr int attn_plan_max_tokens() { return kAttnStreamMax; }

}  // namespace dmp
