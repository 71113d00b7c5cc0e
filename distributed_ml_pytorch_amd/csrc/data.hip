// Batch assembler of the device-resident datasets (utils/device_data.py).
//
// The dataset lives in HBM as dense uint8 NHWC images.  One launch gathers the
// `count` samples a slice of the epoch's permutation names and writes them as
// normalised bf16 NHWC images and int64 labels straight into the training
// step's input buffers, optionally through a per-sample random crop (zero
// padding of `pad` pixels, then an H x W window) and a horizontal flip.
//
// Normalisation is a [C][256] bf16 look-up table built on the host, so the
// kernel does no floating-point arithmetic and its output is the host path's
// `normalize_uint8(x).to(bf16)` bit for bit.  The draw of a sample is one
// Philox4x32-10 call (the rounds of dropout.hip) on
//   ctr = (dataset index, epoch, 0, 0x64617461), key = (seed lo, seed hi),
// a pure function of (seed, epoch, dataset index): no device-side counter, all
// arguments by value, so a launch is graph-capturable and replays identically.
//
// One wave assembles one chunk of one output image; a lane writes 8 consecutive
// bf16 values (one 16-byte store) along the NHWC output, the crop and the flip
// are resolved on the byte read.  Two forms:
//   * staged: the wave first copies its source image into LDS with 16-byte
//     loads (images of a 16-byte-multiple size at aligned starts, at most
//     kDataStageBytes: CIFAR 3072 B, MNIST 784 B);
//   * direct: bytes are gathered through L2 (any size, any alignment); a large
//     image is cut into chunks of kDataChunkGroups stores so that many waves
//     share it.
// Both stay: at the CIFAR shape the direct form alone measured 13.0-14.0 us per
// launch against 11.1 us staged (bs 512, profiles/device_data.txt), well outside
// the run-to-run spread.
// Offsets are 32-bit behind guard::dataset_ok / assemble_ok (bind/data.cpp).
// The mixing form (Mixup / CutMix: two samples per output row) is a sibling
// kernel of the same geometry, after the plain one.
#include "common.h"

namespace dmp {

constexpr int kDataWaves = 2;             // waves (images or chunks) per workgroup
constexpr int kDataStageBytes = 4096;     // largest staged image
constexpr int kDataChunkGroups = 1024;    // 8-value groups per chunk (direct form)
constexpr u32 kDataDomain = 0x64617461u;  // "data": keeps the stream apart from dropout's

// the ten rounds of dropout.hip
__device__ __forceinline__ uint4 data_philox(uint4 ctr, uint2 key) {
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

struct DataArgs {
  const u8* data;          // [N][H][W][C]
  const long long* labels; // [N]
  const u16* lut;          // [C][256] bf16
  const int* index;        // [count] dataset indices
  u16* out_x;              // [>= count][H][W][C] bf16
  long long* out_y;        // [>= count]
  signed char* draws;      // [count][3] (dy, dx, flip) or null
  int count, N, H, W, C, pad, flip;
  u32 seed_lo, seed_hi, epoch;
  int chunks;              // waves per image
  int vec;                 // 16-byte output stores (H*W*C % 8 == 0, aligned out_x)
};

template <bool STAGED>
__global__ void __launch_bounds__(kDataWaves* kWave) batch_assemble_kernel(const DataArgs a) {
  __shared__ u16 slut[4 * 256];
  __shared__ uint4 simg[STAGED ? kDataWaves * (kDataStageBytes / 16) : 1];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int t = threadIdx.x; t < a.C * 256; t += kDataWaves * kWave) slut[t] = a.lut[t];

  const long long wid = (long long)blockIdx.x * kDataWaves + wave;
  const int b = (int)(wid / a.chunks), chunk = (int)(wid - (long long)b * a.chunks);
  const bool live = b < a.count;                 // wave-uniform
  const u32 img = (u32)(a.H * a.W * a.C);        // values (= source bytes) per image
  int i = 0;
  bool valid = false;
  if (live) {
    i = a.index[b];
    valid = i >= 0 && i < a.N;
  }
  const u8* __restrict__ gsrc = a.data + (valid ? (u32)i * img : 0u);
  const u8* wimg = reinterpret_cast<const u8*>(simg) + (STAGED ? wave * kDataStageBytes : 0);
  if constexpr (STAGED) {
    if (valid) {
      const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(gsrc);
      uint4* w4 = simg + wave * (kDataStageBytes / 16);
      for (u32 t = lane; t < img / 16; t += kWave) w4[t] = g4[t];
    }
  }
  __syncthreads();                               // LUT (and the staged images) visible
  if (!live) return;

  const uint4 r = data_philox(make_uint4((u32)i, a.epoch, 0u, kDataDomain),
                              make_uint2(a.seed_lo, a.seed_hi));
  const u32 span = 2u * (u32)a.pad + 1u;
  const int dy = (int)__umulhi(r.x, span), dx = (int)__umulhi(r.y, span);
  const int f = a.flip ? (int)(r.z >> 31) : 0;
  if (chunk == 0 && lane == 0) {
    a.out_y[b] = valid ? a.labels[i] : -100ll;
    if (a.draws) {
      a.draws[b * 3 + 0] = (signed char)dy;
      a.draws[b * 3 + 1] = (signed char)dx;
      a.draws[b * 3 + 2] = (signed char)f;
    }
  }

  const int oy = dy - a.pad, ox = dx - a.pad;
  const u32 ngroups = (img + 7) / 8;
  const u32 g0 = (u32)chunk * kDataChunkGroups;
  const u32 g1 = a.chunks == 1 ? ngroups : min(ngroups, g0 + kDataChunkGroups);
  u16* __restrict__ dst = a.out_x + (u32)b * img;
  for (u32 g = g0 + lane; g < g1; g += kWave) {
    const u32 e0 = g * 8;
    u32 p = e0 / (u32)a.C;
    int c = (int)(e0 - p * (u32)a.C);
    int h = (int)(p / (u32)a.W), w = (int)(p - (u32)h * (u32)a.W);
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int sh = h + oy, sw = (f ? a.W - 1 - w : w) + ox;
      u32 byte = 0;                              // padding: black before normalisation
      if (valid && sh >= 0 && sh < a.H && sw >= 0 && sw < a.W && e0 + k < img) {
        const u32 off = (u32)(sh * a.W + sw) * (u32)a.C + (u32)c;
        byte = STAGED ? wimg[off] : gsrc[off];
      }
      v.v[k] = slut[c * 256 + byte];
      if (++c == a.C) {
        c = 0;
        if (++w == a.W) {
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
        if (e0 + k < img) dst[e0 + k] = v.v[k];
    }
  }
}

bool batch_assemble_staged(const void* data, int H, int W, int C) {
  const long long img = (long long)H * W * C;
  return img % 16 == 0 && img <= kDataStageBytes && reinterpret_cast<uintptr_t>(data) % 16 == 0;
}

void launch_batch_assemble(const u8* data, const long long* labels, const u16* lut,
                           const int* index, int count, int N, int H, int W, int C, u16* out_x,
                           long long* out_y, signed char* draws, int pad, bool flip,
                           unsigned long long seed, u32 epoch, int path, hipStream_t s) {
  if (count <= 0) return;
  const long long img = (long long)H * W * C;
  // path: 0 forces the direct form (measurement, tests); the staged form only where it applies
  const bool staged = path != 0 && batch_assemble_staged(data, H, W, C);
  DataArgs a;
  a.data = data;
  a.labels = labels;
  a.lut = lut;
  a.index = index;
  a.out_x = out_x;
  a.out_y = out_y;
  a.draws = draws;
  a.count = count;
  a.N = N;
  a.H = H;
  a.W = W;
  a.C = C;
  a.pad = pad;
  a.flip = flip ? 1 : 0;
  a.seed_lo = (u32)seed;
  a.seed_hi = (u32)(seed >> 32);
  a.epoch = epoch;
  const long long ngroups = (img + 7) / 8;
  a.chunks = staged ? 1 : (int)((ngroups + kDataChunkGroups - 1) / kDataChunkGroups);
  a.vec = img % 8 == 0 && reinterpret_cast<uintptr_t>(out_x) % 16 == 0;
  const long long waves = (long long)count * a.chunks;
  const dim3 grid((unsigned)((waves + kDataWaves - 1) / kDataWaves));
  if (staged)
    hipLaunchKernelGGL((batch_assemble_kernel<true>), grid, dim3(kDataWaves * kWave), 0, s, a);
  else
    hipLaunchKernelGGL((batch_assemble_kernel<false>), grid, dim3(kDataWaves * kWave), 0, s, a);
}

// ---------------------------------------------------------------- mixing form
// Mixup / CutMix (utils/device_data.py, assemble_mix_reference): output row b is
// built from the views of TWO samples, its own (index[b]) and its partner's
// (index[count - 1 - b]), each with its own Philox draw.  Inside the box
// [y0, y1) x [x0, x1) (output coordinates) the partner's value is stored; outside
// it row b's, or at pix_lam != 1 the blend
//   bf16_rne(fl32(fl32(a * lam) + fl32(p * fl32(1 - lam))))
// of the two LUT values, four separately rounded fp32 operations (no fma, see
// mix_blend: the bits are pinned to the CPU form).  A byte is read only where its value is
// stored.  Lane 0 of chunk 0 also writes the partner's label and label_lam.
// Same geometry as the kernel above; the staged form holds both images in LDS.
struct MixArgs {
  DataArgs d;
  long long* out_y2;       // [>= count] the partner's label
  float* out_lam;          // [>= count] label_lam
  float pix_lam, label_lam;
  int y0, y1, x0, x1;
};

// fl32(fl32(a * lam) + fl32(p * wl)).  __fmul_rn / __fadd_rn are plain * and + in
// this toolchain's headers and, like them, are fused into an fma under the default
// -ffp-contract=fast-honor-pragmas: the operations are written out here with
// contraction switched off for the block.
__device__ __forceinline__ float mix_blend(float a, float p, float lam, float wl) {
#pragma clang fp contract(off)
  const float ta = a * lam;
  const float tp = p * wl;
  return ta + tp;
}

template <bool STAGED>
__global__ void __launch_bounds__(kDataWaves* kWave) batch_assemble_mix_kernel(const MixArgs m) {
  __shared__ u16 slut[4 * 256];
  __shared__ uint4 simg[STAGED ? kDataWaves * 2 * (kDataStageBytes / 16) : 1];
  const DataArgs& a = m.d;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int t = threadIdx.x; t < a.C * 256; t += kDataWaves * kWave) slut[t] = a.lut[t];

  const long long wid = (long long)blockIdx.x * kDataWaves + wave;
  const int b = (int)(wid / a.chunks), chunk = (int)(wid - (long long)b * a.chunks);
  const bool live = b < a.count;                 // wave-uniform
  const u32 img = (u32)(a.H * a.W * a.C);        // values (= source bytes) per image
  const bool blend = m.pix_lam != 1.f;
  const bool boxed = m.y0 < m.y1 && m.x0 < m.x1;
  int i = 0, i2 = 0;
  bool valid = false, valid2 = false;
  if (live) {
    i = a.index[b];
    i2 = a.index[a.count - 1 - b];
    valid = i >= 0 && i < a.N;
    valid2 = i2 >= 0 && i2 < a.N;
  }
  const bool partner = blend || boxed;           // the partner's bytes are read at all
  const u8* __restrict__ gsrc = a.data + (valid ? (u32)i * img : 0u);
  const u8* __restrict__ gsrc2 = a.data + (valid2 ? (u32)i2 * img : 0u);
  const u8* wimg = reinterpret_cast<const u8*>(simg) + (STAGED ? wave * 2 * kDataStageBytes : 0);
  const u8* wimg2 = wimg + (STAGED ? kDataStageBytes : 0);
  if constexpr (STAGED) {
    uint4* w4 = simg + wave * 2 * (kDataStageBytes / 16);
    if (valid) {
      const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(gsrc);
      for (u32 t = lane; t < img / 16; t += kWave) w4[t] = g4[t];
    }
    if (valid2 && partner) {
      const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(gsrc2);
      for (u32 t = lane; t < img / 16; t += kWave) w4[kDataStageBytes / 16 + t] = g4[t];
    }
  }
  __syncthreads();                               // LUT (and the staged images) visible
  if (!live) return;

  const uint2 key = make_uint2(a.seed_lo, a.seed_hi);
  const uint4 r = data_philox(make_uint4((u32)i, a.epoch, 0u, kDataDomain), key);
  const uint4 r2 = data_philox(make_uint4((u32)i2, a.epoch, 0u, kDataDomain), key);
  const u32 span = 2u * (u32)a.pad + 1u;
  const int dy = (int)__umulhi(r.x, span), dx = (int)__umulhi(r.y, span);
  const int f = a.flip ? (int)(r.z >> 31) : 0;
  const int dy2 = (int)__umulhi(r2.x, span), dx2 = (int)__umulhi(r2.y, span);
  const int f2 = a.flip ? (int)(r2.z >> 31) : 0;
  if (chunk == 0 && lane == 0) {
    a.out_y[b] = valid ? a.labels[i] : -100ll;
    m.out_y2[b] = valid2 ? a.labels[i2] : -100ll;
    m.out_lam[b] = m.label_lam;
    if (a.draws) {
      a.draws[b * 3 + 0] = (signed char)dy;
      a.draws[b * 3 + 1] = (signed char)dx;
      a.draws[b * 3 + 2] = (signed char)f;
    }
  }

  const float lam = m.pix_lam, wl = __fsub_rn(1.f, lam);
  const int oy = dy - a.pad, ox = dx - a.pad, oy2 = dy2 - a.pad, ox2 = dx2 - a.pad;
  const u32 ngroups = (img + 7) / 8;
  const u32 g0 = (u32)chunk * kDataChunkGroups;
  const u32 g1 = a.chunks == 1 ? ngroups : min(ngroups, g0 + kDataChunkGroups);
  u16* __restrict__ dst = a.out_x + (u32)b * img;
  for (u32 g = g0 + lane; g < g1; g += kWave) {
    const u32 e0 = g * 8;
    u32 p = e0 / (u32)a.C;
    int c = (int)(e0 - p * (u32)a.C);
    int h = (int)(p / (u32)a.W), w = (int)(p - (u32)h * (u32)a.W);
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool inbox = h >= m.y0 && h < m.y1 && w >= m.x0 && w < m.x1;
      const bool tail = e0 + k < img;
      u32 byte = 0, byte2 = 0;                   // padding: black before normalisation
      if (!inbox) {
        const int sh = h + oy, sw = (f ? a.W - 1 - w : w) + ox;
        if (valid && sh >= 0 && sh < a.H && sw >= 0 && sw < a.W && tail) {
          const u32 off = (u32)(sh * a.W + sw) * (u32)a.C + (u32)c;
          byte = STAGED ? wimg[off] : gsrc[off];
        }
      }
      if (inbox || blend) {
        const int sh = h + oy2, sw = (f2 ? a.W - 1 - w : w) + ox2;
        if (valid2 && sh >= 0 && sh < a.H && sw >= 0 && sw < a.W && tail) {
          const u32 off = (u32)(sh * a.W + sw) * (u32)a.C + (u32)c;
          byte2 = STAGED ? wimg2[off] : gsrc2[off];
        }
      }
      const u16 va = slut[c * 256 + byte], vp = slut[c * 256 + byte2];
      u16 o = va;
      if (inbox)
        o = vp;
      else if (blend)
        o = f2bf(mix_blend(bf2f(va), bf2f(vp), lam, wl));
      v.v[k] = o;
      if (++c == a.C) {
        c = 0;
        if (++w == a.W) {
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
        if (e0 + k < img) dst[e0 + k] = v.v[k];
    }
  }
}

void launch_batch_assemble_mix(const u8* data, const long long* labels, const u16* lut,
                               const int* index, int count, int N, int H, int W, int C,
                               u16* out_x, long long* out_y, long long* out_y2, float* out_lam,
                               signed char* draws, int pad, bool flip, unsigned long long seed,
                               u32 epoch, float pix_lam, float label_lam, int y0, int y1, int x0,
                               int x1, int path, hipStream_t s) {
  if (count <= 0) return;
  const long long img = (long long)H * W * C;
  const bool staged = path != 0 && batch_assemble_staged(data, H, W, C);
  MixArgs m;
  DataArgs& a = m.d;
  a.data = data;
  a.labels = labels;
  a.lut = lut;
  a.index = index;
  a.out_x = out_x;
  a.out_y = out_y;
  a.draws = draws;
  a.count = count;
  a.N = N;
  a.H = H;
  a.W = W;
  a.C = C;
  a.pad = pad;
  a.flip = flip ? 1 : 0;
  a.seed_lo = (u32)seed;
  a.seed_hi = (u32)(seed >> 32);
  a.epoch = epoch;
  const long long ngroups = (img + 7) / 8;
  a.chunks = staged ? 1 : (int)((ngroups + kDataChunkGroups - 1) / kDataChunkGroups);
  a.vec = img % 8 == 0 && reinterpret_cast<uintptr_t>(out_x) % 16 == 0;
  m.out_y2 = out_y2;
  m.out_lam = out_lam;
  m.pix_lam = pix_lam;
  m.label_lam = label_lam;
  m.y0 = y0;
  m.y1 = y1;
  m.x0 = x0;
  m.x1 = x1;
  const long long waves = (long long)count * a.chunks;
  const dim3 grid((unsigned)((waves + kDataWaves - 1) / kDataWaves));
  if (staged)
    hipLaunchKernelGGL((batch_assemble_mix_kernel<true>), grid, dim3(kDataWaves * kWave), 0, s, m);
  else
    hipLaunchKernelGGL((batch_assemble_mix_kernel<false>), grid, dim3(kDataWaves * kWave), 0, s, m);
}

}  // namespace dmp
