// Fused multi-head self-attention for ViT (BASELINE.json config #5, ViT-B/16:
// N = 197 tokens, head dim 64), forward and backward, on gfx950 MFMA
// (v_mfma_f32_16x16x32_bf16).  Not in the reference (no sequence models,
// SURVEY §5.7).
//
// Layout: the qkv projection output is consumed as is, [B, N, 3, H, 64] bf16
// (= the [B*N, 3D] rows of the qkv Linear), the output is written as
// [B, N, H, 64] (= the [B*N, D] input rows of the proj Linear) and the
// backward writes dqkv in the qkv layout: no permute / contiguous copies, no
// zero-filled select-backward buffers, no gradient adds, no materialised
// [B, H, N, N] scores.  One workgroup per (batch, head): the whole key/value
// (or query/dO) set of a head, <= 256 tokens, is staged once in LDS.  These are
// the RESIDENT kernels; longer sequences take the streaming kernels of
// attention_stream.hip, which also holds the public launchers.  The fragment
// helpers both share live in attn_prims.h, the shape -> LDS / grid plan in
// attn_plan.h.
//
// MFMA 16x16x32 fragments (lane l, g = l / 16, l16 = l % 16):
//   A (16 x 32): row l16, k = 8g .. 8g+7        B (32 x 16): col l16, k = 8g .. 8g+7
//   D (16 x 16): col l16, rows 4g .. 4g+3 (4 VGPRs)
// A D tile whose ROW index is a reduction index of the next product feeds that
// product directly: two adjacent 16-row D blocks, packed {block0[0..3],
// block1[0..3]}, are the 8 k-values {4g..4g+3, 16+4g..16+4g+3} of a 32-deep
// k-step; the other operand is read with the same k permutation by two
// ds_read_b64_tr_b16 hardware-transposed reads of the ROW-MAJOR token image
// (ld_tr_perm), so each of K/V (or Q/dO) is staged once, with 16-B stores, and
// serves both the row-wise and the transposed reads.  Every product runs on
// registers + LDS with no shuffles:
//   forward  (query strips):  S^T = K Q^T  ->  softmax  ->  O^T = V^T P^T
//   dQ       (query strips):  S^T, dP^T = V dO^T  ->  dS^T  ->  dQ^T = K^T dS^T
//   dK, dV   (key strips):    S = Q K^T, dP = dO V^T -> dS -> dV^T = dO^T P,
//                             dK^T = Q^T dS
// and every output tile is written as 4 consecutive head-dim values per lane
// (8-B stores).  Softmax statistics are saved as a base-2 log-sum-exp of the
// scaled scores (lse2), so P = exp2(s * scale * log2e - lse2) in the backward.
#include <cstdlib>

#include "attn_plan.h"
#include "attn_prims.h"

namespace dmp {

namespace {

constexpr int kMaxKB = kAttnResidentMax / 16;   // <= 256 tokens: 16 blocks of 16

// Stage token rows [0, NP) of two [token][64] head slices into row-major LDS
// images (stride kRS).  Rows >= N repeat row N-1 -- finite values that every
// consumer gives zero weight -- so the loads are unconditional and each thread
// issues all of its 2 * U loads before its first LDS store (one HBM round trip
// instead of one per row chunk).
template <int NT>
__device__ __forceinline__ void stage2(const u16* __restrict__ s0, int rs0,
                                       const u16* __restrict__ s1, int rs1, long long tok0, int N,
                                       int NP, u16* d0, u16* d1) {
  constexpr int U = 16 * kMaxKB * 8 / NT;
  const int total = NP * 8;
  bf16x8 v0[U], v1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = min(u * NT + (int)threadIdx.x, total - 1);
    const long long t = tok0 + min(i >> 3, N - 1);
    v0[u] = ld16(s0 + t * rs0 + (i & 7) * 8);
    v1[u] = ld16(s1 + t * rs1 + (i & 7) * 8);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = u * NT + threadIdx.x;
    if (i < total) {
      const int o = (i >> 3) * kRS + (i & 7) * 8;
      *reinterpret_cast<bf16x8*>(d0 + o) = v0[u];
      *reinterpret_cast<bf16x8*>(d1 + o) = v1[u];
    }
  }
}

}  // namespace

// KB > 0 would make the key / query block count a compile-time constant: measured
// 2.2x SLOWER on the backward at N = 197 (the fully unrolled loops hoisted every
// fragment read: 256 VGPRs, one workgroup per CU), so only KB = 0 is launched.
// The softmax exponentials use v_exp_f32 directly (__builtin_amdgcn_exp2f: the
// arguments are <= 0 or -inf), not exp2f's range-reduced sequence -- attention
// fwd 35.6 -> 28.9 us, bwd -> 73.6 us per ViT-B/16 layer (profiles/attention_exp2_r4.txt).
// ----------------------------------------------------------------- forward
template <int NW, int KB = 0>
__global__ void __launch_bounds__(64 * NW) attn_fwd_kernel(const u16* __restrict__ qkv,
                                                          u16* __restrict__ out,
                                                          float* __restrict__ lse2, int N, int H,
                                                          float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  const int NP = (N + 31) & ~31, D = H * kDH;
  u16* Ks = smem;              // [NP][kRS]
  u16* Vs = smem + NP * kRS;   // [NP][kRS], read transposed
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  stage2<64 * NW>(base + D, 3 * D, base + 2 * D, 3 * D, tok0, N, NP, Ks, Vs);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int nkb = KB > 0 ? KB : NP / 16, nstrips = (N + 15) / 16;
  for (int qs = wid; qs < nstrips; qs += NW) {
    const int q = qs * 16 + l16, qc = q < N ? q : N - 1;
    const u16* qrow = base + (tok0 + qc) * 3 * D;
    const bf16x8 qf0 = ld16(qrow + 8 * g), qf1 = ld16(qrow + 32 + 8 * g);
    f32x4 s[kMaxKB];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < kMaxKB; ++kb) {
      if (kb < nkb) {
        const u16* kr = Ks + (kb * 16 + l16) * kRS + 8 * g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mfma16(ld16(kr), qf0, acc);
        acc = mfma16(ld16(kr + 32), qf1, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = (kb * 16 + 4 * g + r) < N ? acc[r] * scale_log2 : -INFINITY;
          s[kb][r] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < kMaxKB; ++kb) {
      if (kb < nkb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - mx);   // <= 0: v_exp_f32, no range fix-up
          sum += s[kb][r];
        }
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    f32x4 o[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kp = 0; kp < kMaxKB / 2; ++kp) {
      if (2 * kp < nkb) {
        const bf16x8 pb = pack8(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          o[nb] = mfma16(ld_tr_perm(Vs, 32 * kp, nb * 16, lane), pb, o[nb]);
      }
    }
    if (q < N) {
      const float inv = 1.f / sum;
      u16* orow = out + (tok0 + q) * D + h * kDH + 4 * g;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) st4(orow + nb * 16, o[nb], inv);
      if (g == 0) lse2[(long long)bh * N + q] = mx + log2f(sum);
    }
  }
}

// ------------------------------------------------------------- backward: dQ
template <int NW, int KB = 0>
__global__ void __launch_bounds__(64 * NW) attn_bwd_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ out, const u16* __restrict__ dout,
    const float* __restrict__ lse2, u16* __restrict__ dqkv, int N, int H, float scale_log2,
    float scale) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  const int NP = (N + 31) & ~31, D = H * kDH;
  u16* Ks = smem;                   // [NP][kRS], read row-wise and transposed
  u16* Vs = Ks + NP * kRS;          // [NP][kRS]
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  stage2<64 * NW>(base + D, 3 * D, base + 2 * D, 3 * D, tok0, N, NP, Ks, Vs);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int nkb = KB > 0 ? KB : NP / 16, nstrips = (N + 15) / 16;
  for (int qs = wid; qs < nstrips; qs += NW) {
    const int q = qs * 16 + l16, qc = q < N ? q : N - 1;
    const u16* qrow = base + (tok0 + qc) * 3 * D;
    const u16* orow = out + (tok0 + qc) * D + h * kDH;
    const u16* drow = dout + (tok0 + qc) * D + h * kDH;
    const bf16x8 qf0 = ld16(qrow + 8 * g), qf1 = ld16(qrow + 32 + 8 * g);
    const bf16x8 df0 = ld16(drow + 8 * g), df1 = ld16(drow + 32 + 8 * g);
    const bf16x8 of0 = ld16(orow + 8 * g), of1 = ld16(orow + 32 + 8 * g);
    float di = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      di += bf2f(df0.v[k]) * bf2f(of0.v[k]) + bf2f(df1.v[k]) * bf2f(of1.v[k]);
    di += __shfl_xor(di, 16, 64);
    di += __shfl_xor(di, 32, 64);
    const float L = lse2[(long long)bh * N + qc];
    f32x4 dq[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kp = 0; kp < kMaxKB / 2; ++kp) {
      if (2 * kp < nkb) {
        f32x4 ds[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int kb = 2 * kp + hf;
          const u16* kr = Ks + (kb * 16 + l16) * kRS + 8 * g;
          const u16* vr = Vs + (kb * 16 + l16) * kRS + 8 * g;
          f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
          st = mfma16(ld16(kr), qf0, st);
          st = mfma16(ld16(kr + 32), qf1, st);
          dp = mfma16(ld16(vr), df0, dp);
          dp = mfma16(ld16(vr + 32), df1, dp);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = (kb * 16 + 4 * g + r) < N
                                ? __builtin_amdgcn_exp2f(st[r] * scale_log2 - L) : 0.f;
            ds[hf][r] = p * (dp[r] - di);
          }
        }
        const bf16x8 db = pack8(ds[0], ds[1]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          dq[nb] = mfma16(ld_tr_perm(Ks, 32 * kp, nb * 16, lane), db, dq[nb]);
      }
    }
    if (q < N) {
      u16* dst = dqkv + (tok0 + q) * 3 * D + h * kDH + 4 * g;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) st4(dst + nb * 16, dq[nb], scale);
    }
  }
}

// --------------------------------------------------------- backward: dK, dV
template <int NW, int KB = 0>
__global__ void __launch_bounds__(64 * NW) attn_bwd_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ out, const u16* __restrict__ dout,
    const float* __restrict__ lse2, u16* __restrict__ dqkv, int N, int H, float scale_log2,
    float scale) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  constexpr int NT = 64 * NW, U = 16 * kMaxKB * 8 / NT;
  const int NP = (N + 31) & ~31, D = H * kDH;
  u16* Qs = smem;                   // [NP][kRS], read row-wise and transposed
  u16* Ds = Qs + NP * kRS;          // dO [NP][kRS], read row-wise and transposed
  float* Ls = reinterpret_cast<float*>(Ds + NP * kRS);   // [NP] lse2 (+inf past N)
  float* Di = Ls + NP;                                   // [NP] rowsum(dO * O) (0 past N)
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  // stage Q and dO (as stage2) and reduce Di[q] = dO[q] . O[q] from the dO
  // chunks already in registers: 8 consecutive threads own one row
  {
    const int total = NP * 8;
    bf16x8 vq[U], vd[U], vo[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = min(u * NT + (int)threadIdx.x, total - 1);
      const long long t = tok0 + min(i >> 3, N - 1);
      vq[u] = ld16(base + t * 3 * D + (i & 7) * 8);
      vd[u] = ld16(dout + t * D + h * kDH + (i & 7) * 8);
      vo[u] = ld16(out + t * D + h * kDH + (i & 7) * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = u * NT + threadIdx.x, n = i >> 3;
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) d += bf2f(vo[u].v[k]) * bf2f(vd[u].v[k]);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      if (i < total) {
        const int o = n * kRS + (i & 7) * 8;
        *reinterpret_cast<bf16x8*>(Qs + o) = vq[u];
        *reinterpret_cast<bf16x8*>(Ds + o) = vd[u];
        if ((i & 7) == 0) {
          Di[n] = n < N ? d : 0.f;
          Ls[n] = n < N ? lse2[(long long)bh * N + n] : INFINITY;
        }
      }
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int nqb = KB > 0 ? KB : NP / 16, nstrips = (N + 15) / 16;
  for (int ks = wid; ks < nstrips; ks += NW) {
    const int key = ks * 16 + l16, kc = key < N ? key : N - 1;
    const u16* krow = base + (tok0 + kc) * 3 * D + D;
    const bf16x8 kf0 = ld16(krow + 8 * g), kf1 = ld16(krow + 32 + 8 * g);
    const bf16x8 vf0 = ld16(krow + D + 8 * g), vf1 = ld16(krow + D + 32 + 8 * g);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      dk[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dv[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int qp = 0; qp < kMaxKB / 2; ++qp) {
      if (2 * qp < nqb) {
        f32x4 pp[2], ds[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int qb = 2 * qp + hf;
          const u16* qr = Qs + (qb * 16 + l16) * kRS + 8 * g;
          const u16* dr = Ds + (qb * 16 + l16) * kRS + 8 * g;
          f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
          s = mfma16(ld16(qr), kf0, s);
          s = mfma16(ld16(qr + 32), kf1, s);
          dp = mfma16(ld16(dr), vf0, dp);
          dp = mfma16(ld16(dr + 32), vf1, dp);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qq = qb * 16 + 4 * g + r;
            const float p = __builtin_amdgcn_exp2f(s[r] * scale_log2 - Ls[qq]);   // Ls = +inf past N
            pp[hf][r] = p;
            ds[hf][r] = p * (dp[r] - Di[qq]);
          }
        }
        const bf16x8 pb = pack8(pp[0], pp[1]), db = pack8(ds[0], ds[1]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          dv[nb] = mfma16(ld_tr_perm(Ds, 32 * qp, nb * 16, lane), pb, dv[nb]);
          dk[nb] = mfma16(ld_tr_perm(Qs, 32 * qp, nb * 16, lane), db, dk[nb]);
        }
      }
    }
    if (key < N) {
      u16* dst = dqkv + (tok0 + key) * 3 * D + h * kDH + 4 * g;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        st4(dst + D + nb * 16, dk[nb], scale);
        st4(dst + 2 * D + nb * 16, dv[nb], 1.f);
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
// The resident route.  attention_stream.hip owns the public launchers
// (launch_attention_fwd / _bwd): they plan (attn_plan.h) and dispatch here.
namespace {
constexpr int kFwdWaves = 8, kBwdWaves = 8;
static_assert(kFwdWaves == kAttnStreamWaves && kBwdWaves == kAttnStreamWaves, "AttnPlan::waves");
}  // namespace

// two row-major [NP][kRS] bf16 images per kernel (+ lse2 / Di rows for dK,dV):
// 64.5 KiB at N = 197, two workgroups per CU (AttnPlan::lds_*)
void launch_attention_resident_fwd(const AttnPlan& p, const u16* qkv, u16* out, float* lse2, int B,
                                   int N, int H, float scale, hipStream_t s) {
  const size_t lds = p.lds_fwd;
  const float sl2 = scale * 1.4426950408889634f;
  allow_lds(attn_fwd_kernel<kFwdWaves>, lds);
  hipLaunchKernelGGL(attn_fwd_kernel<kFwdWaves>, dim3(B * H), dim3(64 * kFwdWaves), lds, s, qkv,
                     out, lse2, N, H, sl2);
}

void launch_attention_resident_bwd(const AttnPlan& p, const u16* qkv, const u16* out,
                                   const u16* dout, const float* lse2, u16* dqkv, int B, int N,
                                   int H, float scale, hipStream_t s) {
  const float sl2 = scale * 1.4426950408889634f;
  const size_t l1 = p.lds_dkv, l2 = p.lds_dq;
  allow_lds(attn_bwd_dkv_kernel<kBwdWaves>, l1);
  allow_lds(attn_bwd_dq_kernel<kBwdWaves>, l2);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<kBwdWaves>, dim3(B * H), dim3(64 * kBwdWaves), l1, s, qkv,
                     out, dout, lse2, dqkv, N, H, sl2, scale);
  hipLaunchKernelGGL(attn_bwd_dq_kernel<kBwdWaves>, dim3(B * H), dim3(64 * kBwdWaves), l2, s, qkv,
                     out, dout, lse2, dqkv, N, H, sl2, scale);
}

}  // namespace dmp
