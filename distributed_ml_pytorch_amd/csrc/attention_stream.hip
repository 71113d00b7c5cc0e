// Streaming ("flash"-style) fused multi-head self-attention for head dim 64,
// bf16, 1 <= N <= 4096 tokens, forward and backward, on gfx950 MFMA: the second
// route beside the resident kernels of attention.hip (which stage a head's whole
// token set once and stop at 256 tokens), and the public launchers of both.
//
// Same contracts as the resident route: qkv rows [B, N, 3, H, 64] in, out
// [B, N, H, 64], lse2 [B, H, N] (base-2 log-sum-exp of the scaled scores), dqkv
// in the qkv layout; no permute copies, no [B, H, N, N] scores, no zero fills, no
// gradient adds, no atomics: every output element is written by exactly one
// wave, so two runs give the same bits.  The two routes exchange only out and
// lse2, so a forward of one route can be followed by the backward of the other.
//
// A workgroup of 8 waves owns a block of 128 tokens, one 16-token strip per wave
// held in registers with the fragment layouts of attention.hip, and streams
// tiles of kKT = 128 tokens of the other operand through LDS as row-major
// [kKT][kRS] images (the resident kernels' images, read row-wise and with
// ld_tr_perm).  The images are double-buffered: the global loads of tile t + 1
// are issued into registers before tile t's MFMAs and stored to the other stage
// after them, one barrier per tile (a stage is rewritten only after the barrier
// that ends the last tile that read it).
//   forward  (query strips, key tiles):   S^T = K Q^T -> online softmax -> O^T += V^T P^T
//   dQ       (query strips, key tiles):   P from lse2, dQ^T += K^T dS^T
//   dK, dV   (key strips, query tiles):   dV^T += dO^T P, dK^T += Q^T dS
// 36 KiB per stage, 72 KiB per workgroup (74 KiB for dK, dV with the lse2 / Di
// rows): two workgroups per CU.  Plans (blocks, tiles, LDS, grids): attn_plan.h.
#include <cstdio>
#include <cstdlib>

#include "attn_plan.h"
#include "attn_prims.h"

namespace dmp {

// attention.hip
void launch_attention_resident_fwd(const AttnPlan& p, const u16* qkv, u16* out, float* lse2, int B,
                                   int N, int H, float scale, hipStream_t s);
void launch_attention_resident_bwd(const AttnPlan& p, const u16* qkv, const u16* out,
                                   const u16* dout, const float* lse2, u16* dqkv, int B, int N,
                                   int H, float scale, hipStream_t s);

namespace {

constexpr int kNW = kAttnStreamWaves, kNT = 64 * kNW;
constexpr int kKT = kAttnStreamTile;       // tokens per staged tile
constexpr int kQB = kAttnStreamBlock;      // tokens per workgroup
constexpr int kU = kKT * 8 / kNT;          // 16-B chunks per thread per image
constexpr int kImg = kKT * kRS;            // elements of one image
static_assert(kKT * 8 % kNT == 0 && kKT % 32 == 0 && kQB == 16 * kNW, "tile / block shape");

// One tile of two [token][64] head slices in flight in registers: rows row0 ..
// row0 + kKT - 1 of the head, rows >= N repeat row N - 1 (finite values that
// every consumer gives zero weight), so the loads are unconditional.
struct TileRegs {
  bf16x8 a[kU], b[kU];
};

__device__ __forceinline__ void tile_load(TileRegs& r, const u16* __restrict__ s0, int rs0,
                                          const u16* __restrict__ s1, int rs1, long long tok0,
                                          int row0, int N) {
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = u * kNT + (int)threadIdx.x;
    const long long t = tok0 + min(row0 + (i >> 3), N - 1);
    r.a[u] = ld16(s0 + t * rs0 + (i & 7) * 8);
    r.b[u] = ld16(s1 + t * rs1 + (i & 7) * 8);
  }
}

__device__ __forceinline__ void tile_store(const TileRegs& r, u16* d0, u16* d1) {
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = u * kNT + (int)threadIdx.x;
    const int o = (i >> 3) * kRS + (i & 7) * 8;
    *reinterpret_cast<bf16x8*>(d0 + o) = r.a[u];
    *reinterpret_cast<bf16x8*>(d1 + o) = r.b[u];
  }
}

// 16-row blocks of tile t that hold a valid token, rounded up to a pair (the
// 32-deep k-step of the second product)
__device__ __forceinline__ int tile_blocks(int N, int t) {
  const int left = N - t * kKT;
  return left >= kKT ? kKT / 16 : ((left + 31) & ~31) / 16;
}

}  // namespace

// ----------------------------------------------------------------- forward
// Online softmax in the S^T = K Q^T layout: a lane's D-tile column is its query,
// so the running max m, the running sum l and the rescale factor exp2(m_old -
// m_new) are per-lane scalars (equal in the four lanes g of a query after the
// two __shfl_xor reductions).  P = exp2(s - m_new) is rounded to bf16 relative
// to the running max including this tile; O^T stays in fp32 and is multiplied by
// the factor before the tile's V^T P^T.
// Padded keys get -inf.  Every staged tile holds at least one valid key (tiles =
// ceil(N / kKT)) and valid scores are finite, so m_new is finite in every tile:
// the first tile's m_old = -inf gives the factor exp2(-inf) = 0 (on l = 0 and
// O = 0), never inf - inf.
__global__ void __launch_bounds__(kNT) attn_stream_fwd_kernel(const u16* __restrict__ qkv,
                                                             u16* __restrict__ out,
                                                             float* __restrict__ lse2, int N, int H,
                                                             int nqb, float scale_log2) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  const int D = H * kDH;
  const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  const u16* ksrc = base + D;
  const u16* vsrc = base + 2 * D;
  const int nt = (N + kKT - 1) / kKT;
  TileRegs tr;
  tile_load(tr, ksrc, 3 * D, vsrc, 3 * D, tok0, 0, N);
  tile_store(tr, smem, smem + kImg);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int q0 = qblk * kQB + wid * 16;
  const bool active = q0 < N;            // wave-uniform
  const int q = q0 + l16, qc = q < N ? q : N - 1;
  const u16* qrow = base + (tok0 + qc) * 3 * D;
  const bf16x8 qf0 = ld16(qrow + 8 * g), qf1 = ld16(qrow + 32 + 8 * g);
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;        // block-uniform
    if (more) tile_load(tr, ksrc, 3 * D, vsrc, 3 * D, tok0, (t + 1) * kKT, N);
    if (active) {
      const u16* Ks = smem + (t & 1) * 2 * kImg;
      const u16* Vs = Ks + kImg;
      const int nkb = tile_blocks(N, t), key0 = t * kKT;
      f32x4 s[kKT / 16];
      float mx = m;
#pragma unroll
      for (int kb = 0; kb < kKT / 16; ++kb) {
        if (kb < nkb) {
          const u16* kr = Ks + (kb * 16 + l16) * kRS + 8 * g;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = mfma16(ld16(kr), qf0, acc);
          acc = mfma16(ld16(kr + 32), qf1, acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = (key0 + kb * 16 + 4 * g + r) < N ? acc[r] * scale_log2 : -INFINITY;
            s[kb][r] = v;
            mx = fmaxf(mx, v);
          }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float f = __builtin_amdgcn_exp2f(m - mx);   // <= 0, -inf in the first tile: 0
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < kKT / 16; ++kb) {
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
      l = l * f + sum;
      m = mx;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) o[nb] *= f;
#pragma unroll
      for (int kp = 0; kp < kKT / 32; ++kp) {
        if (2 * kp < nkb) {
          const bf16x8 pb = pack8(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
          for (int nb = 0; nb < 4; ++nb)
            o[nb] = mfma16(ld_tr_perm(Vs, 32 * kp, nb * 16, lane), pb, o[nb]);
        }
      }
    }
    if (more) {
      u16* st = smem + ((t + 1) & 1) * 2 * kImg;
      tile_store(tr, st, st + kImg);
    }
    __syncthreads();
  }
  if (q < N) {
    const float inv = 1.f / l;
    u16* orow = out + (tok0 + q) * D + h * kDH + 4 * g;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) st4(orow + nb * 16, o[nb], inv);
    if (g == 0) lse2[(long long)bh * N + q] = m + log2f(l);
  }
}

// ------------------------------------------------------------- backward: dQ
// P is recomputed from lse2, di = rowsum(dO * O) per strip; dQ accumulates in
// registers across the key tiles with no rescale.  The strip's di also goes to
// the [B, H, N] fp32 buffer di_out, which the dK, dV kernel reads.
__global__ void __launch_bounds__(kNT) attn_stream_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ out, const u16* __restrict__ dout,
    const float* __restrict__ lse2, u16* __restrict__ dqkv, float* __restrict__ di_out, int N, int H,
    int nqb, float scale_log2, float scale) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  const int D = H * kDH;
  const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  const u16* ksrc = base + D;
  const u16* vsrc = base + 2 * D;
  const int nt = (N + kKT - 1) / kKT;
  TileRegs tr;
  tile_load(tr, ksrc, 3 * D, vsrc, 3 * D, tok0, 0, N);
  tile_store(tr, smem, smem + kImg);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int q0 = qblk * kQB + wid * 16;
  const bool active = q0 < N;            // wave-uniform
  const int q = q0 + l16, qc = q < N ? q : N - 1;
  const u16* qrow = base + (tok0 + qc) * 3 * D;
  const u16* orow = out + (tok0 + qc) * D + h * kDH;
  const u16* drow = dout + (tok0 + qc) * D + h * kDH;
  const bf16x8 qf0 = ld16(qrow + 8 * g), qf1 = ld16(qrow + 32 + 8 * g);
  const bf16x8 df0 = ld16(drow + 8 * g), df1 = ld16(drow + 32 + 8 * g);
  float di = 0.f;
  {
    const bf16x8 of0 = ld16(orow + 8 * g), of1 = ld16(orow + 32 + 8 * g);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      di += bf2f(df0.v[k]) * bf2f(of0.v[k]) + bf2f(df1.v[k]) * bf2f(of1.v[k]);
  }
  di += __shfl_xor(di, 16, 64);
  di += __shfl_xor(di, 32, 64);
  const float L = lse2[(long long)bh * N + qc];
  f32x4 dq[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;        // block-uniform
    if (more) tile_load(tr, ksrc, 3 * D, vsrc, 3 * D, tok0, (t + 1) * kKT, N);
    if (active) {
      const u16* Ks = smem + (t & 1) * 2 * kImg;   // read row-wise and transposed
      const u16* Vs = Ks + kImg;
      const int nkb = tile_blocks(N, t), key0 = t * kKT;
#pragma unroll
      for (int kp = 0; kp < kKT / 32; ++kp) {
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
              const float p = (key0 + kb * 16 + 4 * g + r) < N
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
    }
    if (more) {
      u16* st = smem + ((t + 1) & 1) * 2 * kImg;
      tile_store(tr, st, st + kImg);
    }
    __syncthreads();
  }
  if (q < N) {
    u16* dst = dqkv + (tok0 + q) * 3 * D + h * kDH + 4 * g;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) st4(dst + nb * 16, dq[nb], scale);
    if (g == 0) di_out[(long long)bh * N + q] = di;
  }
}

// --------------------------------------------------------- backward: dK, dV
// A query tile carries Q and dO with their Ls (lse2, +inf past N) and Di
// (rowsum(dO * O), 0 past N) rows.  Di comes from the [B, H, N] buffer the dQ
// kernel wrote (launched before this one on the same stream): reducing it per
// staged tile from dO and O, as the resident kernel does, measured 15-19 %
// slower on the whole backward (profiles/attention_stream.txt) and was dropped.
// Held to 128 VGPRs (4 waves per SIMD) so that two workgroups share a CU.
__global__ void __launch_bounds__(kNT, 4) attn_stream_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ dout, const float* __restrict__ lse2,
    const float* __restrict__ di_in, u16* __restrict__ dqkv, int N, int H, int nkblk,
    float scale_log2, float scale) {
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  constexpr int kStage = 2 * kImg + 2 * kKT * 2;   // u16 elements: Q, dO images, Ls, Di rows
  const int D = H * kDH;
  const int bh = blockIdx.x / nkblk, kblk = blockIdx.x - bh * nkblk, b = bh / H, h = bh - b * H;
  const long long tok0 = (long long)b * N;
  const u16* base = qkv + h * kDH;
  const u16* dsrc = dout + h * kDH;
  const float* lrow = lse2 + (long long)bh * N;
  const float* drow = di_in + (long long)bh * N;
  const int nt = (N + kKT - 1) / kKT;
  const int srow = threadIdx.x >> 3;               // staged row of chunk u: u * (kNT / 8) + srow
  const bool rowlead = (threadIdx.x & 7) == 0;

  TileRegs tr;
  float tl[kU], td[kU];
  auto load = [&](int row0) {
    tile_load(tr, base, 3 * D, dsrc, D, tok0, row0, N);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int n = row0 + u * (kNT / 8) + srow;
      const bool valid = rowlead && n < N;
      tl[u] = valid ? lrow[n] : INFINITY;
      td[u] = valid ? drow[n] : 0.f;
    }
  };
  auto store = [&](int stage) {
    u16* Qs = smem + stage * kStage;
    u16* Ds = Qs + kImg;
    float* Ls = reinterpret_cast<float*>(Ds + kImg);
    float* Di = Ls + kKT;
    tile_store(tr, Qs, Ds);
    if (rowlead) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        Ls[u * (kNT / 8) + srow] = tl[u];
        Di[u * (kNT / 8) + srow] = td[u];
      }
    }
  };
  load(0);
  store(0);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, l16 = lane & 15;
  const int k0 = kblk * kQB + wid * 16;
  const bool active = k0 < N;            // wave-uniform
  const int key = k0 + l16, kc = key < N ? key : N - 1;
  const u16* krow = base + (tok0 + kc) * 3 * D + D;
  const bf16x8 kf0 = ld16(krow + 8 * g), kf1 = ld16(krow + 32 + 8 * g);
  const bf16x8 vf0 = ld16(krow + D + 8 * g), vf1 = ld16(krow + D + 32 + 8 * g);
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    dk[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;        // block-uniform
    if (more) load((t + 1) * kKT);
    if (active) {
      const u16* Qs = smem + (t & 1) * kStage;     // read row-wise and transposed
      const u16* Ds = Qs + kImg;                   // dO, read row-wise and transposed
      const float* Ls = reinterpret_cast<const float*>(Ds + kImg);
      const float* Di = Ls + kKT;
      const int nqb = tile_blocks(N, t);
#pragma unroll
      for (int qp = 0; qp < kKT / 32; ++qp) {
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
    }
    if (more) store((t + 1) & 1);
    __syncthreads();
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

// ---------------------------------------------------------------- launchers
int attention_max_tokens() { return attn_plan_max_tokens(); }
int attention_head_dim() { return kDH; }

namespace {

AttnPlan plan_or_die(int B, int N, int H, int route) {
  const AttnPlan p = plan_attention(N, route, (long long)B * H);
  if (!p.ok) {
    std::fprintf(stderr, "attention: no route for N = %d, route %d, B * H = %lld\n", N, route,
                 (long long)B * H);
    std::abort();
  }
  return p;
}

}  // namespace

long long attention_bwd_workspace_floats(int B, int N, int H, int route) {
  const AttnPlan p = plan_attention(N, route, (long long)B * H);
  if (!p.ok || p.route != kAttnStream) return 0;
  return (long long)B * H * N;
}

void launch_attention_fwd(const u16* qkv, u16* out, float* lse2, int B, int N, int H, float scale,
                          int route, hipStream_t s) {
  const AttnPlan p = plan_or_die(B, N, H, route);
  if (p.route == kAttnResident)
    return launch_attention_resident_fwd(p, qkv, out, lse2, B, N, H, scale, s);
  const float sl2 = scale * 1.4426950408889634f;
  allow_lds(attn_stream_fwd_kernel, p.lds_fwd);
  hipLaunchKernelGGL(attn_stream_fwd_kernel, dim3((unsigned)p.grid_fwd), dim3(kNT), p.lds_fwd, s,
                     qkv, out, lse2, N, H, p.q_blocks, sl2);
}

void launch_attention_bwd(const u16* qkv, const u16* out, const u16* dout, const float* lse2,
                          u16* dqkv, float* ws, int B, int N, int H, float scale, int route,
                          hipStream_t s) {
  const AttnPlan p = plan_or_die(B, N, H, route);
  if (p.route == kAttnResident)
    return launch_attention_resident_bwd(p, qkv, out, dout, lse2, dqkv, B, N, H, scale, s);
  const float sl2 = scale * 1.4426950408889634f;
  if (ws == nullptr) {
    std::fprintf(stderr, "attention backward: the streaming route needs its Di workspace\n");
    std::abort();
  }
  allow_lds(attn_stream_dq_kernel, p.lds_dq);
  hipLaunchKernelGGL(attn_stream_dq_kernel, dim3((unsigned)p.grid_dq), dim3(kNT), p.lds_dq, s, qkv,
                     out, dout, lse2, dqkv, ws, N, H, p.q_blocks, sl2, scale);
  allow_lds(attn_stream_dkv_kernel, p.lds_dkv);
  hipLaunchKernelGGL(attn_stream_dkv_kernel, dim3((unsigned)p.grid_dkv), dim3(kNT), p.lds_dkv, s,
                     qkv, dout, lse2, ws, dqkv, N, H, p.k_blocks, sl2, scale);
}

}  // namespace dmp
