// Random-resized-crop form of the batch assembler (utils/device_data.py,
// assemble_rrc_reference): every sample is a box of its stored Hs x Ws image,
// resampled to the Ho x Wo output with integer bilinear weights, flipped and
// normalised through the [C][256] bf16 look-up table.  No floating-point
// arithmetic decides a pixel, so the output is the CPU definition bit for bit.
//
// Draw: one Philox4x32-10 call per sample on
//   ctr = (dataset index, epoch, 1, 0x64617461), key = (seed lo, seed hi)
// (counter word 2 is 1: apart from the crop form's stream).  t = (r.x T) >> 32
// picks the box size (bh, bw) from the host-built table, y0 = (r.y (Hs - bh + 1))
// >> 32, x0 = (r.z (Ws - bw + 1)) >> 32, f = r.w >> 31.  A fixed box (evaluation)
// replaces (y0, x0, bh, bw) for every sample.
//
// Resample, per axis (output extent O, box extent b, o mirrored first when f):
//   num = max((2 o + 1) b - O, 0), i0 = num / 2O, fr = ((num % 2O) 256 + O) / 2O,
//   i1 = min(i0 + 1, b - 1)
//   v = (256 - fy)((256 - fx) p00 + fx p01) + fy((256 - fx) p10 + fx p11) < 2^24
//   byte = (v + 32768) >> 16
//
// Work split: one workgroup of four waves per (sample, strip of R output rows);
// R comes from guard::rrc_plan.  The workgroup
//   1. fills the column table in LDS, one u32 per output column
//      (i0 * C | (i1 - i0) << 15 | fx << 16, the flip folded in), shared by every
//      row of the strip, and the strip's row table (two row offsets and fy);
//   2. staged form: copies the source rows of the box that the strip touches into
//      LDS as raw bytes, one wave per row.  A row starts at byte x0 * C of its
//      image row, anywhere; it is stored at its global 16-byte phase, so the body
//      moves as aligned 16-byte loads and only the first and last chunk of a row
//      go byte by byte.  A source byte is fetched once per strip;
//      direct form (not even one output row's sources fit the budget, e.g. a
//      1024-wide image reduced to 8 x 8): the row offsets address global memory
//      and the four taps are gathered through L2;
//   3. every lane forms 8 consecutive output values, four taps and one LUT read
//      each, and writes them with one 16-byte store (value by value where
//      Ho Wo C % 8 != 0 or a strip does not start on a group).
// The mixing form (MIX) stages and resamples two views, row b's and the view of
// index[count - 1 - b], and combines them as data.hip's mixing kernel does.
// Arguments by value, no atomics, no device counter: graph-capturable.  Offsets
// are 32-bit behind guard::dataset_ok / rrc_ok (bind/data.cpp).
#include "common.h"
#include "geom_guard.h"
#include "launchers.h"

namespace dmp {

constexpr int kRrcThreads = 256;
constexpr int kRrcWaves = kRrcThreads / kWave;
constexpr int kRrcRows = guard::kRrcMaxStrip;
constexpr u32 kRrcDomain = 0x64617461u;   // "data", as data.hip
constexpr u32 kRrcStream = 1u;            // counter word 2

// the ten rounds of dropout.hip
__device__ __forceinline__ uint4 rrc_philox(uint4 ctr, uint2 key) {
  constexpr u32 M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u32 hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const u32 hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

struct RrcArgs {
  const u8* data;          // [N][Hs][Ws][C]
  const long long* labels; // [N]
  const u16* lut;          // [C][256] bf16
  const int* index;        // [count] dataset indices
  const short* table;      // [T][2] box sizes (bh, bw); unused with a fixed box
  u16* out_x;              // [>= count][Ho][Wo][C] bf16
  long long* out_y;        // [>= count]
  short* draws;            // [count][5] (y0, x0, bh, bw, f) or null
  int count, N, Hs, Ws, C, Ho, Wo, T, flip;
  int fixed, fy0, fx0, fbh, fbw;   // fixed != 0: this box for every sample
  u32 seed_lo, seed_hi, epoch;
  int strip, strips;       // R and ceil(Ho / R)
  int stage_rows, pitch;   // staged rows per view, bytes between them
  int table_bytes;         // LDS before the staged rows
  int vec;                 // 16-byte output stores
};

struct RrcMix {
  long long* out_y2;       // [>= count] the partner's label
  float* out_lam;          // [>= count] label_lam
  float pix_lam, label_lam;
  int y0, y1, x0, x1;
};

struct RrcView {
  const u8* src;           // the sample's stored image
  bool valid;
  int y0, x0, bh, bw, f;
};

// i0, i1 and the 8-bit weight of output coordinate o on an axis of O outputs over b inputs
__device__ __forceinline__ void rrc_axis(int o, int b, int O, u32& i0, u32& i1, u32& fr) {
  const int n = (2 * o + 1) * b - O;
  const u32 num = n > 0 ? (u32)n : 0u, den = 2u * (u32)O;
  i0 = num / den;
  fr = ((num - i0 * den) * 256u + (u32)O) / den;
  i1 = min(i0 + 1u, (u32)b - 1u);
}

__device__ __forceinline__ RrcView rrc_draw(const RrcArgs& a, int i) {
  RrcView v;
  v.valid = i >= 0 && i < a.N;
  v.src = a.data + (v.valid ? (u32)i * (u32)(a.Hs * a.Ws * a.C) : 0u);
  const uint4 r = rrc_philox(make_uint4((u32)i, a.epoch, kRrcStream, kRrcDomain),
                             make_uint2(a.seed_lo, a.seed_hi));
  if (a.fixed) {
    v.y0 = a.fy0, v.x0 = a.fx0, v.bh = a.fbh, v.bw = a.fbw;
  } else {
    const u32 t = __umulhi(r.x, (u32)a.T);
    // a table the binding has checked holds only sizes inside the image; the
    // clamp keeps every address in range whatever the table holds
    v.bh = min(max((int)a.table[2 * t], 1), a.Hs);
    v.bw = min(max((int)a.table[2 * t + 1], 1), a.Ws);
    v.y0 = (int)__umulhi(r.y, (u32)(a.Hs - v.bh + 1));
    v.x0 = (int)__umulhi(r.z, (u32)(a.Ws - v.bw + 1));
  }
  v.f = a.flip ? (int)(r.w >> 31) : 0;
  return v;
}

// byte offset of the box's row `row` (box coordinates) from the image start
__device__ __forceinline__ u32 rrc_row_offset(const RrcArgs& a, const RrcView& v, u32 row) {
  return (((u32)v.y0 + row) * (u32)a.Ws + (u32)v.x0) * (u32)a.C;
}

// Tables of one view for output rows [r0, r1), and in the staged form the source
// rows those touch.  col: Wo entries; row0 / row1 / rowf: r1 - r0 entries, the
// offsets of the two source rows (into `stage`, or from v.src) and fy.
template <bool STAGED>
__device__ __forceinline__ void rrc_prepare(const RrcArgs& a, const RrcView& v, int r0, int r1,
                                            u32* col, u32* row0, u32* row1, u32* rowf,
                                            u8* stage) {
  const int tid = threadIdx.x;
  for (int w = tid; w < a.Wo; w += kRrcThreads) {
    u32 i0, i1, fx;
    rrc_axis(v.f ? a.Wo - 1 - w : w, v.bw, a.Wo, i0, i1, fx);
    col[w] = (i0 * (u32)a.C) | ((i1 - i0) << 15) | (fx << 16);
  }
  u32 lo, hi, unused_i, unused_f;
  rrc_axis(r0, v.bh, a.Ho, lo, unused_i, unused_f);        // first source row of the strip
  rrc_axis(r1 - 1, v.bh, a.Ho, unused_i, hi, unused_f);    // last
  const u32 phase0 = (u32)(reinterpret_cast<uintptr_t>(v.src) & 15u);
  if (tid < r1 - r0) {
    u32 i0, i1, fy;
    rrc_axis(r0 + tid, v.bh, a.Ho, i0, i1, fy);
    const u32 g0 = rrc_row_offset(a, v, i0), g1 = rrc_row_offset(a, v, i1);
    row0[tid] = STAGED ? (i0 - lo) * (u32)a.pitch + ((phase0 + g0) & 15u) : g0;
    row1[tid] = STAGED ? (i1 - lo) * (u32)a.pitch + ((phase0 + g1) & 15u) : g1;
    rowf[tid] = fy;
  }
  if constexpr (STAGED) {
    if (!v.valid) return;
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    const u32 len = (u32)(v.bw * a.C);
    for (u32 s = wave; s <= hi - lo; s += kRrcWaves) {      // s < stage_rows: guard::rrc_strip_rows
      const u8* __restrict__ g = v.src + rrc_row_offset(a, v, lo + s);
      const u32 ph = (u32)(reinterpret_cast<uintptr_t>(g) & 15u);
      u8* d = stage + s * (u32)a.pitch;                     // byte j of the row at d[ph + j]
      for (u32 k = lane; k * 16u < ph + len; k += kWave) {
        const u32 p0 = max(k * 16u, ph), p1 = min(k * 16u + 16u, ph + len);
        if (p1 - p0 == 16u) {
          *reinterpret_cast<uint4*>(d + p0) = *reinterpret_cast<const uint4*>(g - ph + p0);
        } else {
          for (u32 p = p0; p < p1; ++p) d[p] = g[p - ph];
        }
      }
    }
  }
}

// the resampled byte of one output value: c is the channel, ce the column entry
__device__ __forceinline__ u32 rrc_byte(const u8* base, u32 ro0, u32 ro1, u32 fy, u32 ce, int c,
                                        int C) {
  const u32 x0 = (ce & 0x7fffu) + (u32)c, x1 = x0 + ((ce >> 15) & 1u ? (u32)C : 0u);
  const u32 fx = ce >> 16;
  const u32 p00 = base[ro0 + x0], p01 = base[ro0 + x1], p10 = base[ro1 + x0], p11 = base[ro1 + x1];
  const u32 top = (256u - fx) * p00 + fx * p01, bot = (256u - fx) * p10 + fx * p11;
  return ((256u - fy) * top + fy * bot + 32768u) >> 16;
}

// fl32(fl32(a * lam) + fl32(p * wl)), never contracted into an fma (data.hip, mix_blend)
__device__ __forceinline__ float rrc_blend(float a, float p, float lam, float wl) {
#pragma clang fp contract(off)
  const float ta = a * lam;
  const float tp = p * wl;
  return ta + tp;
}

template <bool STAGED, bool MIX>
__global__ void __launch_bounds__(kRrcThreads)
batch_assemble_rrc_kernel(const RrcArgs a, const RrcMix m) {
  extern __shared__ uint4 rrc_lds[];
  constexpr int kViews = MIX ? 2 : 1;
  u16* slut = reinterpret_cast<u16*>(rrc_lds);                          // [4][256]
  u32* tabs = reinterpret_cast<u32*>(slut + 4 * 256);                   // per view: col, 3 x rows
  u8* stage = reinterpret_cast<u8*>(rrc_lds) + a.table_bytes;           // per view: stage_rows x pitch
  const int tid = threadIdx.x;
  for (int t = tid; t < a.C * 256; t += kRrcThreads) slut[t] = a.lut[t];

  const int b = (int)(blockIdx.x / (u32)a.strips);
  const int strip = (int)(blockIdx.x - (u32)b * (u32)a.strips);
  const int r0 = strip * a.strip, r1 = min(r0 + a.strip, a.Ho);
  const u32 view_tab = (u32)a.Wo + 3u * kRrcRows, view_stage = (u32)(a.stage_rows * a.pitch);

  const int i = a.index[b];
  const RrcView va = rrc_draw(a, i);
  rrc_prepare<STAGED>(a, va, r0, r1, tabs, tabs + a.Wo, tabs + a.Wo + kRrcRows,
                      tabs + a.Wo + 2 * kRrcRows, stage);
  RrcView vp = va;
  bool blend = false, boxed = false;
  int i2 = i;
  if constexpr (MIX) {
    i2 = a.index[a.count - 1 - b];
    vp = rrc_draw(a, i2);
    blend = m.pix_lam != 1.f;
    boxed = m.x0 < m.x1 && m.y0 < r1 && m.y1 > r0;     // the box meets this strip
    if (blend || boxed)                                // the partner's bytes are read at all
      rrc_prepare<STAGED>(a, vp, r0, r1, tabs + view_tab, tabs + view_tab + a.Wo,
                          tabs + view_tab + a.Wo + kRrcRows, tabs + view_tab + a.Wo + 2 * kRrcRows,
                          stage + view_stage);
  }
  __syncthreads();                                     // LUT, tables and staged rows visible

  if (strip == 0 && tid == 0) {
    a.out_y[b] = va.valid ? a.labels[i] : -100ll;
    if constexpr (MIX) {
      m.out_y2[b] = vp.valid ? a.labels[i2] : -100ll;
      m.out_lam[b] = m.label_lam;
    }
    if (a.draws) {
      short* d = a.draws + b * 5;
      d[0] = (short)va.y0, d[1] = (short)va.x0, d[2] = (short)va.bh, d[3] = (short)va.bw;
      d[4] = (short)va.f;
    }
  }

  const u8* base_a = STAGED ? stage : va.src;
  const u8* base_p = STAGED ? stage + view_stage : vp.src;
  const u32* col_a = tabs;
  const u32* col_p = tabs + view_tab;
  const float lam = m.pix_lam, wl = __fsub_rn(1.f, lam);
  const u32 row_vals = (u32)(a.Wo * a.C);
  const u32 e_lo = (u32)r0 * row_vals, e_hi = (u32)r1 * row_vals;       // the strip's values
  u16* __restrict__ dst = a.out_x + (u32)b * ((u32)a.Ho * row_vals);
  for (u32 g = tid; g * 8u < e_hi - e_lo; g += kRrcThreads) {
    const u32 e0 = e_lo + g * 8u;
    const u32 p = e0 / (u32)a.C;
    int c = (int)(e0 - p * (u32)a.C);
    int h = (int)(p / (u32)a.Wo), w = (int)(p - (u32)h * (u32)a.Wo);
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      u16 o = 0;
      if (e0 + k < e_hi) {
        const int j = h - r0;
        bool inbox = false;
        if constexpr (MIX) inbox = h >= m.y0 && h < m.y1 && w >= m.x0 && w < m.x1;
        u32 byte = 0, byte2 = 0;                       // an index outside [0, N): byte 0
        if (!inbox && va.valid)
          byte = rrc_byte(base_a, col_a[a.Wo + j], col_a[a.Wo + kRrcRows + j],
                          col_a[a.Wo + 2 * kRrcRows + j], col_a[w], c, a.C);
        if (MIX && (inbox || blend) && vp.valid)
          byte2 = rrc_byte(base_p, col_p[a.Wo + j], col_p[a.Wo + kRrcRows + j],
                           col_p[a.Wo + 2 * kRrcRows + j], col_p[w], c, a.C);
        o = slut[c * 256 + byte];
        if constexpr (MIX) {
          const u16 op = slut[c * 256 + byte2];
          if (inbox)
            o = op;
          else if (blend)
            o = f2bf(rrc_blend(bf2f(o), bf2f(op), lam, wl));
        }
      }
      v.v[k] = o;
      if (++c == a.C) {
        c = 0;
        if (++w == a.Wo) {
          w = 0;
          ++h;
        }
      }
    }
    if (a.vec) {
      *reinterpret_cast<bf16x8*>(dst + e0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (e0 + k < e_hi) dst[e0 + k] = v.v[k];
    }
  }
}

void launch_batch_assemble_rrc(const u8* data, const long long* labels, const u16* lut,
                               const int* index, int count, int N, int Hs, int Ws, int C,
                               const short* table, int T, const int* box, int Ho, int Wo,
                               u16* out_x, long long* out_y, short* draws, bool flip,
                               unsigned long long seed, u32 epoch, const RrcMixParams* mix,
                               int path, hipStream_t s) {
  if (count <= 0) return;
  const guard::RrcPlan plan = guard::rrc_plan(Hs, Ws, C, Ho, Wo, mix != nullptr, path == 0);
  RrcArgs a;
  a.data = data;
  a.labels = labels;
  a.lut = lut;
  a.index = index;
  a.table = table;
  a.out_x = out_x;
  a.out_y = out_y;
  a.draws = draws;
  a.count = count;
  a.N = N;
  a.Hs = Hs;
  a.Ws = Ws;
  a.C = C;
  a.Ho = Ho;
  a.Wo = Wo;
  a.T = T;
  a.flip = flip ? 1 : 0;
  a.fixed = box != nullptr;
  a.fy0 = box ? box[0] : 0;
  a.fx0 = box ? box[1] : 0;
  a.fbh = box ? box[2] : 1;
  a.fbw = box ? box[3] : 1;
  a.seed_lo = (u32)seed;
  a.seed_hi = (u32)(seed >> 32);
  a.epoch = epoch;
  a.strip = plan.strip;
  a.strips = (Ho + plan.strip - 1) / plan.strip;
  a.stage_rows = plan.stage_rows;
  a.pitch = plan.pitch;
  a.table_bytes = plan.table_bytes;
  const long long img = (long long)Ho * Wo * C, strip_vals = (long long)plan.strip * Wo * C;
  a.vec = img % 8 == 0 && (a.strips == 1 || strip_vals % 8 == 0) &&
          reinterpret_cast<uintptr_t>(out_x) % 16 == 0;
  RrcMix m{};
  if (mix) {
    m.out_y2 = mix->out_y2;
    m.out_lam = mix->out_lam;
    m.pix_lam = mix->pix_lam;
    m.label_lam = mix->label_lam;
    m.y0 = mix->y0;
    m.y1 = mix->y1;
    m.x0 = mix->x0;
    m.x1 = mix->x1;
  }
  const dim3 grid((unsigned)((long long)count * a.strips)), block(kRrcThreads);
  const size_t lds = (size_t)plan.lds_bytes;
  if (plan.staged) {
    if (mix)
      hipLaunchKernelGGL((batch_assemble_rrc_kernel<true, true>), grid, block, lds, s, a, m);
    else
      hipLaunchKernelGGL((batch_assemble_rrc_kernel<true, false>), grid, block, lds, s, a, m);
  } else {
    if (mix)
      hipLaunchKernelGGL((batch_assemble_rrc_kernel<false, true>), grid, block, lds, s, a, m);
    else
      hipLaunchKernelGGL((batch_assemble_rrc_kernel<false, false>), grid, block, lds, s, a, m);
  }
}

}  // namespace dmp
