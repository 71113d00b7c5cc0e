// Shifted-window multi-head self-attention for the hierarchical window
// transformer (Swin: Liu et al. 2021), forward and backward, on gfx950 MFMA
// (v_mfma_f32_16x16x32_bf16).  Not in the reference (no sequence models).
//
// Contract (constants in attn_window_plan.h).  qkv is [B, Hm, Wm, 3, heads, 32]
// bf16, the qkv Linear's output rows in map order; out is [B, Hm, Wm, heads, 32].
// Token (ty, tx) of window (wy, wx) is map pixel ((wy ws + ty + sh) mod Hm,
// (wx ws + tx + sh) mod Wm): torch.roll(x, (-sh, -sh)) + window partition done by
// address arithmetic on the loads, and every store (out, dqkv) goes back to that
// pixel, so no roll, partition or reverse copy exists.  Scores are
//   s_ij = q_i . k_j * 32^-0.5 + table[(yi - yj + ws - 1)(2 ws - 1) + xi - xj + ws - 1, head]
// plus -100 when sh > 0 and tokens i, j lie in different regions of the rolled
// frame (per axis [0, L - ws), [L - ws, L - sh), [L - sh, L)).  table is the fp32
// parameter, read as it is.
//
// Design.  The problem is tens of thousands of tiny heads (N = ws^2 <= 64 tokens,
// head dim 32), so ONE WAVE owns one (window, head) end to end and nothing is
// shared between waves: no barrier in either kernel.  Head dim 32 is exactly one
// k-step of the MFMA, so a 16 x 16 score tile is one instruction and the whole
// 64 x 64 score tile of a window lives in registers strip by strip (16 fp32
// values per lane per strip).  Fragments (see attention.hip for the lane maps):
//   forward  S^T = K Q^T -> softmax over keys (16 in-lane values + two cross-lane
//            steps) -> O^T = V^T P^T, the packed D tiles feeding the product.
//   backward pass A (query strips): S^T, dP^T = V dO^T -> P, Di = sum_j P dP,
//            dS^T -> dQ^T = K^T dS^T; lse2 and Di go to 64-float LDS rows.
//            pass B (key strips): S = Q K^T, dP = dO V^T -> P, dS from the LDS
//            rows -> dV^T = dO^T P, dK^T = Q^T dS.
// Q, K, V, dO row fragments (16 B of one token: dims 8g .. 8g+7) come from global
// memory straight into registers, all of a window's loads issued before the first
// use; the same registers are stored once into row-major [token][40] LDS images
// for the operands that are also read transposed (ds_read_b64_tr_b16): V in the
// forward, K, Q and dO in the backward.  Per window the wave writes one int per
// token -- ty (2 ws - 1) + tx + (region << 12) -- so the bias index and the
// region test of a pair are ONE subtraction: the low 12 bits of
// code_i + off - code_j index the bias column, the rest is non-zero across
// regions.  The bias column of the wave's head sits in LDS, premultiplied by
// log2 e (the softmax runs in base 2 on v_exp_f32).  Dead strips are compiled
// out (template NS: ws = 4 runs one strip of four).
//
// Deviations from a shared-workgroup design, with the reasons: (1) the region
// codes are per wave, not per workgroup: 64 integer ops per window against a
// barrier that would couple four independent waves.  (2) The backward forms the
// score tile in both orientations (8 more MFMAs per strip) instead of bouncing
// dS through LDS: dQ reduces over keys and dK / dV over queries, so one of them
// needs the transpose whichever orientation is chosen; the kernel moves ~22 KB
// per (window, head) against ~100 MFMAs, and the bounce would cost 8 KB of LDS
// per wave on top of the 16 KB it has.  (3) Softmax statistics are recomputed in
// pass A, which needs S^T anyway: no lse2 tensor, and Di = sum_j P_ij dP_ij comes
// from registers, so the backward does not read `out`.
//
// Grid: persistent, wave w owns head w % heads and windows w / heads + k * rows
// (attn_window_plan.h).  That is what makes the bias-table gradient cheap and
// reproducible: dtable[idx, h] = sum of dS_ij over batch, windows and the pairs
// with index idx, and idx depends on (i, j) only, so a wave adds dS position-wise
// into 64 fp32 registers across all of its windows, folds the N x N positions to
// (2 ws - 1)^2 once at the end (through LDS, fixed order) and overwrites its own
// row of a [rows][T][heads] slab; win_attn_dtable_kernel adds the rows in index
// order into the arena gradient.  No atomics, nothing to zero, bitwise
// reproducible.  Measured (profiles/window_attention.txt): at four strips the
// backward holds 247 VGPRs + 24 AGPRs, one wave per SIMD (LDS alone would allow
// two workgroups per CU), and runs 5.3-6.1x the forward's time; the fragments of
// all four blocks, not the 64 sums alone, are what fills the file, and an
// LDS-side fold per window would add a 16 KB round trip per window to save them.
// Shortening the fragments' lifetimes is the open lever.  The forward needs 86
// VGPRs (5 waves per SIMD) and runs at 1.8-2.8x a copy of its bytes.
#include "attn_prims.h"
#include "attn_window_plan.h"

namespace dmp {

namespace {

constexpr int kWS = kWinRowStride;
constexpr float kLog2e = 1.4426950408889634f;

struct WinGeom {
  int Hm, Wm, heads, ws, sh, N, T, nwy, nwx, rows, windows;
};

// LDS written by some lanes of this wave and read by others: the DS queue of a
// wave is in order, so this only has to keep the compiler from moving accesses
// across it (and drains the queue, which costs nothing here).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ld_tr_perm of attn_prims.h on a [token][kWS] image (head dim 32)
__device__ __forceinline__ bf16x8 win_ld_tr(const u16* img, int row0, int col0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const u16* a = img + (row0 + 4 * g + q) * kWS + col0 + 4 * p;
  const s16x4_t lo =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(a + 16 * kWS));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// this lane's token (ty, tx) of window `win`: its code and its map pixel
__device__ __forceinline__ void win_token(const WinGeom& g, int win, int ty, int tx, int& code,
                                          int& pix) {
  const int per = g.nwy * g.nwx, b = win / per, rem = win - b * per;
  const int wy = rem / g.nwx, wx = rem - wy * g.nwx;
  const int ry = wy * g.ws + ty, rx = wx * g.ws + tx;   // rolled-frame coordinates
  int py = ry + g.sh, px = rx + g.sh;
  py -= py >= g.Hm ? g.Hm : 0;
  px -= px >= g.Wm ? g.Wm : 0;
  int label = 0;
  if (g.sh > 0) {
    const int ay = ry < g.Hm - g.ws ? 0 : (ry < g.Hm - g.sh ? 1 : 2);
    const int ax = rx < g.Wm - g.ws ? 0 : (rx < g.Wm - g.sh ? 1 : 2);
    label = 3 * ay + ax;
  }
  code = ty * (2 * g.ws - 1) + tx + (label << kWinLabelShift);
  pix = (b * g.Hm + py) * g.Wm + px;
}

// base-2 logit of a pair from the raw dot product: d = code_i + off - code_j
__device__ __forceinline__ float win_logit(float dot, int d, const float* bias, float sl2) {
  const float m = (d >> kWinLabelShift) != 0 ? kWinMaskValue * kLog2e : 0.f;
  return dot * sl2 + bias[d & ((1 << kWinLabelShift) - 1)] + m;
}

__device__ __forceinline__ float wave_max4(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}

__device__ __forceinline__ float wave_sum4(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

}  // namespace

// ----------------------------------------------------------------- forward
// NS live strips; NB = NS rounded up to the 32-key k-step of the P V product
// (the odd block's keys get zero weight, its rows repeat token N - 1).
template <int NS>
__global__ void __launch_bounds__(64 * kWinWaves) win_attn_fwd_kernel(
    const u16* __restrict__ qkv, const float* __restrict__ table, u16* __restrict__ out,
    const WinGeom g, const float sl2) {
  constexpr int NB = (NS + 1) & ~1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, gq = lane >> 4, l16 = lane & 15;
  unsigned char* base = smem + wid * (kWinImageBytes + win_side_bytes(g.T));
  u16* Vs = reinterpret_cast<u16*>(base);                         // [64][kWS], read transposed
  int* code = reinterpret_cast<int*>(base + kWinImageBytes);      // [64]
  int* pix = code + kWinMaxTokens;                                // [64]
  float* bias = reinterpret_cast<float*>(pix + kWinMaxTokens);    // [T] table column * log2 e
  const int w = blockIdx.x * kWinWaves + wid, h = w % g.heads, C = g.heads * kWinHeadDim;
  for (int t = lane; t < g.T; t += 64) bias[t] = table[t * g.heads + h] * kLog2e;
  const int tt = min(lane, g.N - 1), ty = tt / g.ws, tx = tt - ty * g.ws;
  const int off = (g.ws - 1) * (2 * g.ws - 1) + g.ws - 1;

  for (int win = w / g.heads; win < g.windows; win += g.rows) {
    int c, p;
    win_token(g, win, ty, tx, c, p);
    code[lane] = c;
    pix[lane] = p;
    wave_lds_sync();
    bf16x8 qf[NS], kf[NB];
    int kc[NB][4];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const int tok = kb * 16 + l16;
      const u16* src = qkv + (long long)pix[tok] * 3 * C + h * kWinHeadDim + 8 * gq;
      if (kb < NS) qf[kb] = ld16(src);
      kf[kb] = ld16(src + C);
      *reinterpret_cast<bf16x8*>(Vs + tok * kWS + 8 * gq) = ld16(src + 2 * C);
      const int4 k4 = *reinterpret_cast<const int4*>(code + kb * 16 + 4 * gq);
      kc[kb][0] = k4.x, kc[kb][1] = k4.y, kc[kb][2] = k4.z, kc[kb][3] = k4.w;
    }
    wave_lds_sync();
#pragma unroll
    for (int qs = 0; qs < NS; ++qs) {
      const int q = qs * 16 + l16, qcode = code[q] + off;
      f32x4 s[NB];
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        const f32x4 acc = mfma16(kf[kb], qf[qs], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = (kb * 16 + 4 * gq + r) < g.N
                              ? win_logit(acc[r], qcode - kc[kb][r], bias, sl2) : -INFINITY;
          s[kb][r] = v;
          mx = fmaxf(mx, v);
        }
      }
      mx = wave_max4(mx);
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - mx);   // <= 0: v_exp_f32
          sum += s[kb][r];
        }
      sum = wave_sum4(sum);
      f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kp = 0; kp < NB / 2; ++kp) {
        const bf16x8 pb = pack8(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          o[nb] = mfma16(win_ld_tr(Vs, 32 * kp, nb * 16, lane), pb, o[nb]);
      }
      if (q < g.N) {
        const float inv = 1.f / sum;
        u16* orow = out + (long long)pix[q] * C + h * kWinHeadDim + 4 * gq;
        st4(orow, o[0], inv);
        st4(orow + 16, o[1], inv);
      }
    }
    wave_lds_sync();   // the next window overwrites code, pix and the image
  }
}

// ---------------------------------------------------------------- backward
template <int NS>
__global__ void __launch_bounds__(64 * kWinWaves) win_attn_bwd_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ dout, const float* __restrict__ table,
    u16* __restrict__ dqkv, float* __restrict__ slab, const WinGeom g, const float sl2,
    const float scale) {
  constexpr int NB = (NS + 1) & ~1;
  constexpr size_t kTile = (size_t)kWinMaxTokens * kWinMaxTokens * 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, gq = lane >> 4, l16 = lane & 15;
  unsigned char* base =
      smem + wid * (kTile + win_side_bytes(g.T) + (size_t)2 * kWinMaxTokens * 4);
  u16* Ks = reinterpret_cast<u16*>(base);                 // three [64][kWS] images, read
  u16* Qs = Ks + kWinMaxTokens * kWS;                     // transposed; overlaid by the
  u16* Ds = Qs + kWinMaxTokens * kWS;                     // [64][64] fp32 fold tile at the end
  float* Ls = reinterpret_cast<float*>(base + kTile);     // [64] lse2 (+inf past N)
  float* Di = Ls + kWinMaxTokens;                         // [64] sum_j P dP (0 past N)
  int* code = reinterpret_cast<int*>(Di + kWinMaxTokens);
  int* pix = code + kWinMaxTokens;
  float* bias = reinterpret_cast<float*>(pix + kWinMaxTokens);
  const int w = blockIdx.x * kWinWaves + wid, h = w % g.heads, C = g.heads * kWinHeadDim;
  for (int t = lane; t < g.T; t += 64) bias[t] = table[t * g.heads + h] * kLog2e;
  const int tt = min(lane, g.N - 1), ty = tt / g.ws, tx = tt - ty * g.ws;
  const int off = (g.ws - 1) * (2 * g.ws - 1) + g.ws - 1;
  if (lane >= 16 * NS) {   // the odd block's queries: pass A never writes them
    Ls[lane] = INFINITY;
    Di[lane] = 0.f;
  }
  // dS summed position-wise over this wave's windows: [query strip][key block][4 keys]
  f32x4 tsum[NS][NB];
#pragma unroll
  for (int qs = 0; qs < NS; ++qs)
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) tsum[qs][kb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int win = w / g.heads; win < g.windows; win += g.rows) {
    int c, p;
    win_token(g, win, ty, tx, c, p);
    code[lane] = c;
    pix[lane] = p;
    wave_lds_sync();
    bf16x8 qf[NB], kf[NB], vf[NB], df[NB];
    int kc[NB][4];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const long long px = pix[kb * 16 + l16];
      const u16* src = qkv + px * 3 * C + h * kWinHeadDim + 8 * gq;
      qf[kb] = ld16(src);
      kf[kb] = ld16(src + C);
      vf[kb] = ld16(src + 2 * C);
      df[kb] = ld16(dout + px * C + h * kWinHeadDim + 8 * gq);
    }
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      const int o = (kb * 16 + l16) * kWS + 8 * gq;
      *reinterpret_cast<bf16x8*>(Ks + o) = kf[kb];
      *reinterpret_cast<bf16x8*>(Qs + o) = qf[kb];
      *reinterpret_cast<bf16x8*>(Ds + o) = df[kb];
      const int4 k4 = *reinterpret_cast<const int4*>(code + kb * 16 + 4 * gq);
      kc[kb][0] = k4.x, kc[kb][1] = k4.y, kc[kb][2] = k4.z, kc[kb][3] = k4.w;
    }
    wave_lds_sync();

    // pass A, query strips: P, Di, dS^T -> dQ; statistics to LDS; dS into tsum
#pragma unroll
    for (int qs = 0; qs < NS; ++qs) {
      const int q = qs * 16 + l16, qcode = code[q] + off;
      f32x4 s[NB], dp[NB];
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        const f32x4 acc = mfma16(kf[kb], qf[qs], f32x4{0.f, 0.f, 0.f, 0.f});
        dp[kb] = mfma16(vf[kb], df[qs], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = (kb * 16 + 4 * gq + r) < g.N
                              ? win_logit(acc[r], qcode - kc[kb][r], bias, sl2) : -INFINITY;
          s[kb][r] = v;
          mx = fmaxf(mx, v);
        }
      }
      mx = wave_max4(mx);
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - mx);
          sum += s[kb][r];
        }
      sum = wave_sum4(sum);
      const float inv = 1.f / sum;
      float di = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kb][r] *= inv;
          di += s[kb][r] * dp[kb][r];
        }
      di = wave_sum4(di);
      const bool live = q < g.N;
      if (gq == 0) {
        Ls[q] = live ? mx + log2f(sum) : INFINITY;
        Di[q] = live ? di : 0.f;
      }
#pragma unroll
      for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kb][r] = s[kb][r] * (dp[kb][r] - di);   // dS; exactly 0 on padding keys (P = 0)
          tsum[qs][kb][r] += live ? s[kb][r] : 0.f;
        }
      f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kp = 0; kp < NB / 2; ++kp) {
        const bf16x8 db = pack8(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          dq[nb] = mfma16(win_ld_tr(Ks, 32 * kp, nb * 16, lane), db, dq[nb]);
      }
      if (live) {
        u16* dst = dqkv + (long long)pix[q] * 3 * C + h * kWinHeadDim + 4 * gq;
        st4(dst, dq[0], scale);
        st4(dst + 16, dq[1], scale);
      }
    }
    wave_lds_sync();   // Ls, Di: written by the g = 0 lanes, read by all

    // pass B, key strips: P and dS in the other orientation -> dV, dK
#pragma unroll
    for (int ks = 0; ks < NS; ++ks) {
      const int key = ks * 16 + l16, kcode = code[key] - off;
      f32x4 dk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int qp = 0; qp < NB / 2; ++qp) {
        f32x4 pp[2], ds[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int qb = 2 * qp + hf;
          const f32x4 acc = mfma16(qf[qb], kf[ks], f32x4{0.f, 0.f, 0.f, 0.f});
          const f32x4 dp = mfma16(df[qb], vf[ks], f32x4{0.f, 0.f, 0.f, 0.f});
          const int4 qc = *reinterpret_cast<const int4*>(code + qb * 16 + 4 * gq);
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(Ls + qb * 16 + 4 * gq);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(Di + qb * 16 + 4 * gq);
          const int qcs[4] = {qc.x, qc.y, qc.z, qc.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // Ls = +inf past N: P = 0
            const float pv = __builtin_amdgcn_exp2f(
                win_logit(acc[r], qcs[r] - kcode, bias, sl2) - l4[r]);
            pp[hf][r] = pv;
            ds[hf][r] = pv * (dp[r] - d4[r]);
          }
        }
        const bf16x8 pb = pack8(pp[0], pp[1]), db = pack8(ds[0], ds[1]);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          dv[nb] = mfma16(win_ld_tr(Ds, 32 * qp, nb * 16, lane), pb, dv[nb]);
          dk[nb] = mfma16(win_ld_tr(Qs, 32 * qp, nb * 16, lane), db, dk[nb]);
        }
      }
      if (key < g.N) {
        u16* dst = dqkv + (long long)pix[key] * 3 * C + h * kWinHeadDim + 4 * gq;
        st4(dst + C, dk[0], scale);
        st4(dst + C + 16, dk[1], scale);
        st4(dst + 2 * C, dv[0], 1.f);
        st4(dst + 2 * C + 16, dv[1], 1.f);
      }
    }
    wave_lds_sync();   // the next window overwrites code, pix, Ls, Di and the images
  }

  // fold the N x N positions to the (2 ws - 1)^2 table rows, fixed order, and
  // overwrite this wave's slab row (all of it: zeros from a wave without windows)
  if (slab == nullptr) return;
  float* F = reinterpret_cast<float*>(base);   // [query][64 keys]
#pragma unroll
  for (int qs = 0; qs < NS; ++qs)
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
      *reinterpret_cast<f32x4*>(F + (qs * 16 + l16) * kWinMaxTokens + kb * 16 + 4 * gq) =
          tsum[qs][kb];
  wave_lds_sync();
  const int side = 2 * g.ws - 1;
  float* row = slab + (long long)(w / g.heads) * g.T * g.heads + h;
  for (int t = lane; t < g.T; t += 64) {
    const int dy = t / side - (g.ws - 1), dx = t - (t / side) * side - (g.ws - 1);
    float v = 0.f;
    for (int yj = max(0, -dy); yj < min(g.ws, g.ws - dy); ++yj)
      for (int xj = max(0, -dx); xj < min(g.ws, g.ws - dx); ++xj)
        v += F[((yj + dy) * g.ws + xj + dx) * kWinMaxTokens + yj * g.ws + xj];
    row[(long long)t * g.heads] = v;
  }
}

// dtable[e] += sum over the slab rows, in index order
__global__ void __launch_bounds__(256) win_attn_dtable_kernel(const float* __restrict__ slab,
                                                              float* __restrict__ dtable, int n,
                                                              int rows) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float v = 0.f;
  for (int r = 0; r < rows; ++r) v += slab[(long long)r * n + e];
  dtable[e] += v;
}

// ---------------------------------------------------------------- launchers
namespace {

WinGeom win_geom(const WinAttnPlan& p, int Hm, int Wm, int heads, int ws, int sh) {
  return WinGeom{Hm, Wm, heads, ws, sh, p.N, p.T, Hm / ws, Wm / ws, p.rows, (int)p.windows};
}

float win_scale() { return 1.f / sqrtf((float)kWinHeadDim); }

}  // namespace

long long window_attention_slab_floats(long long B, int Hm, int Wm, int heads, int ws, int sh) {
  const WinAttnPlan p = plan_window_attention(B, Hm, Wm, heads, ws, sh);
  return p.ok ? (long long)p.rows * p.T * heads : 0;
}

#define DMP_WIN_STRIPS(n, CALL) \
  switch (n) {                  \
    case 1: CALL(1); break;     \
    case 2: CALL(2); break;     \
    case 3: CALL(3); break;     \
    default: CALL(4); break;    \
  }

void launch_window_attention_fwd(const u16* qkv, const float* table, u16* out, long long B, int Hm,
                                 int Wm, int heads, int ws, int sh, hipStream_t s) {
  const WinAttnPlan p = plan_window_attention(B, Hm, Wm, heads, ws, sh);
  if (!p.ok) return;
  const WinGeom g = win_geom(p, Hm, Wm, heads, ws, sh);
  const float sl2 = win_scale() * kLog2e;
#define DMP_WIN_FWD(NS)                                                                        \
  allow_lds(win_attn_fwd_kernel<NS>, p.lds_fwd);                                               \
  hipLaunchKernelGGL(win_attn_fwd_kernel<NS>, dim3(p.grid), dim3(64 * kWinWaves), p.lds_fwd, s, \
                     qkv, table, out, g, sl2)
  DMP_WIN_STRIPS(p.strips, DMP_WIN_FWD)
#undef DMP_WIN_FWD
}

// dtable / slab both null: no bias-table gradient.  slab: uninitialised,
// window_attention_slab_floats fp32 elements.
void launch_window_attention_bwd(const u16* qkv, const u16* dout, const float* table, u16* dqkv,
                                 float* dtable, float* slab, long long B, int Hm, int Wm, int heads,
                                 int ws, int sh, hipStream_t s) {
  const WinAttnPlan p = plan_window_attention(B, Hm, Wm, heads, ws, sh);
  if (!p.ok) return;
  const WinGeom g = win_geom(p, Hm, Wm, heads, ws, sh);
  const float scale = win_scale(), sl2 = scale * kLog2e;
  float* sl = dtable ? slab : nullptr;
#define DMP_WIN_BWD(NS)                                                                        \
  allow_lds(win_attn_bwd_kernel<NS>, p.lds_bwd);                                               \
  hipLaunchKernelGGL(win_attn_bwd_kernel<NS>, dim3(p.grid), dim3(64 * kWinWaves), p.lds_bwd, s, \
                     qkv, dout, table, dqkv, sl, g, sl2, scale)
  DMP_WIN_STRIPS(p.strips, DMP_WIN_BWD)
#undef DMP_WIN_BWD
  if (sl) {
    const int n = p.T * heads;
    hipLaunchKernelGGL(win_attn_dtable_kernel, dim3((n + 255) / 256), dim3(256), 0, s, sl, dtable,
                       n, p.rows);
  }
}

#undef DMP_WIN_STRIPS

}  // namespace dmp
