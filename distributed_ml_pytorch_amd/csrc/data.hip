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

}  // namespace dmp
