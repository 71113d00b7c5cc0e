// Host-side shape arithmetic and 32-bit offset guards shared by the PyTorch
// bindings (bind/*.cpp) and the sanitizer driver (host_check.cpp, `make asan`).
//
// Every HIP kernel here addresses its operands through buffer descriptors with
// 32-bit BYTE offsets (num_records is a 32-bit field), so a tensor the kernels
// touch must stay under 2 GiB; these checks are the only thing standing between
// an oversize batch and a wrapped offset.  Plain C++ (no torch, no HIP) so the
// sanitizer build can drive them over every model's shape set, including the
// rejection paths, with -fsanitize=address,undefined.
#pragma once

#include <cstdint>

namespace dmp {
namespace guard {

constexpr int64_t kTwoGiB = int64_t(1) << 31;

// output extent of a convolution / pooling window; <= 0 when empty or invalid
inline int64_t conv_out(int64_t in, int64_t pad, int64_t k, int64_t stride) {
  if (stride < 1 || pad < 0 || k < 1 || in < 1) return 0;
  const int64_t span = in + 2 * pad - k;
  return span < 0 ? 0 : span / stride + 1;
}

// a value that must fit the kernels' `int` arguments
inline bool fits_int(int64_t v) { return v >= 0 && v < kTwoGiB; }

// scale * a * b * c * d < limit, every factor >= 0, without overflowing int64
// on the way (checked factor by factor)
inline bool prod_lt(int64_t limit, int64_t scale, int64_t a, int64_t b, int64_t c, int64_t d) {
  int64_t e = scale;
  for (int64_t f : {a, b, c, d}) {
    if (f < 0) return false;
    if (f != 0 && e > INT64_MAX / f) return false;
    e *= f;
  }
  return e < limit;
}

// bf16 NHWC tensor of n*h*w*c elements addressable with 32-bit byte offsets
inline bool bf16_bytes_ok(int64_t n, int64_t h, int64_t w, int64_t c) {
  return prod_lt(kTwoGiB, 2, n, h, w, c);
}

// implicit-GEMM conv (conv.hip / conv_wgrad.hip): input, output and weight
// all under 2 GiB of bf16 (1 << 30 elements) and every extent an int
inline bool conv_offsets_ok(int64_t B, int64_t H, int64_t W, int64_t CI, int64_t OH, int64_t OW,
                            int64_t CO, int64_t R, int64_t S) {
  for (int64_t v : {B, H, W, CI, OH, OW, CO, R, S})
    if (!fits_int(v)) return false;
  return bf16_bytes_ok(B, H, W, CI) && bf16_bytes_ok(B, OH, OW, CO) &&
         bf16_bytes_ok(CO, CI, R, S);
}

// depthwise K x K / stride 1 / "same" conv (dwconv.hip): 32-bit element offsets
// into the one [N, H, W, C] bf16 geometry that input, output and both gradients
// share; the image index and the 32-channel chunk index are grid dimensions
// (<= 65535 each)
inline bool dwconv_ok(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K) {
  for (int64_t v : {N, H, W, C})
    if (v < 1 || !fits_int(v)) return false;
  return (K == 3 || K == 5 || K == 7) && C % 8 == 0 && N <= 65535 && (C + 31) / 32 <= 65535 &&
         bf16_bytes_ok(N, H, W, C);
}

// few-input-channel stem convs (conv_small.hip): 32-bit ELEMENT indexing of the
// output, 2 GiB of input
inline bool small_conv_ok(int64_t B, int64_t OH, int64_t OW, int64_t CO, int64_t x_numel) {
  for (int64_t v : {B, OH, OW, CO})
    if (!fits_int(v)) return false;
  return prod_lt(kTwoGiB, 1, B, OH, OW, CO) && x_numel >= 0 && x_numel < (int64_t(1) << 30);
}

// ImageNet stem (stem.hip): the [B, H/2, W/2, 64] output under 2 GiB
inline bool stem_batch_ok(int64_t B, int64_t H, int64_t W) {
  return fits_int(B) && bf16_bytes_ok(B, H / 2, W / 2, 64);
}

// a row-major [rows][ld] operand of `elem`-byte elements (gemm.hip)
inline bool rows_bytes_ok(int64_t elem, int64_t rows, int64_t ld) {
  if (elem <= 0 || rows < 0 || ld < 0) return false;
  if (rows != 0 && ld > INT64_MAX / rows / elem) return false;
  return elem * rows * ld < kTwoGiB;
}

// device-resident uint8 NHWC dataset (data.hip): 32-bit BYTE offsets into the
// n*h*w*c image bytes, an `int` sample count, 1..4 channels (the look-up table
// the kernel keeps in LDS is [4][256])
constexpr int64_t kDatasetMaxChannels = 4;
constexpr int64_t kDatasetMaxPad = 16;
inline bool dataset_ok(int64_t n, int64_t h, int64_t w, int64_t c) {
  if (c < 1 || c > kDatasetMaxChannels || h < 1 || w < 1 || !fits_int(n)) return false;
  return prod_lt(kTwoGiB, 1, n, h, w, c);
}

// one assembled batch: `count` bf16 NHWC images under 2 GiB, pad in range
inline bool assemble_ok(int64_t count, int64_t h, int64_t w, int64_t c, int64_t pad) {
  return pad >= 0 && pad <= kDatasetMaxPad && fits_int(count) && bf16_bytes_ok(count, h, w, c);
}

// mixing form of the assembler: the CutMix box [y0, y1) x [x0, x1) inside the
// h x w output (empty allowed), both weights finite and in [0, 1] (a NaN fails
// every comparison)
inline bool mix_ok(int64_t h, int64_t w, int64_t y0, int64_t y1, int64_t x0, int64_t x1,
                   double pix_lam, double label_lam) {
  if (!(0 <= y0 && y0 <= y1 && y1 <= h && 0 <= x0 && x0 <= x1 && x1 <= w)) return false;
  return pix_lam >= 0.0 && pix_lam <= 1.0 && label_lam >= 0.0 && label_lam <= 1.0;
}

// random-resized-crop form of the assembler (data_rrc.hip): a box of the stored
// hs x ws image resampled to ho x wo.  Extents up to 4096 keep every product of
// the integer bilinear weights in 32 bits ((2 o + 1) b <= 2^25, i0 * c <= 2^14).
constexpr int64_t kRrcMaxExtent = 4096;
constexpr int64_t kRrcMaxTable = 4096;         // the 64 x 64 grid of box cells
inline bool rrc_ok(int64_t count, int64_t hs, int64_t ws, int64_t c, int64_t ho, int64_t wo) {
  for (int64_t v : {hs, ws, ho, wo})
    if (v < 1 || v > kRrcMaxExtent) return false;
  return c >= 1 && c <= kDatasetMaxChannels && fits_int(count) && bf16_bytes_ok(count, ho, wo, c);
}

// a box (y0, x0, bh, bw) of at least one pixel inside the hs x ws image
inline bool rrc_box_ok(int64_t hs, int64_t ws, int64_t y0, int64_t x0, int64_t bh, int64_t bw) {
  return bh >= 1 && bw >= 1 && y0 >= 0 && x0 >= 0 && bh <= hs && bw <= ws && y0 <= hs - bh &&
         x0 <= ws - bw;
}

// Source rows staged for `r` consecutive output rows of a bh -> ho resample.
// Output row o reads rows i0(o) = floor(s(o)) and i0(o) + 1 with s(o + 1) - s(o)
// = bh / ho, so the rows from the strip's first tap to its last number
// floor(s + d) - floor(s) + 2 <= ceil(d) + 2, d = (r - 1) bh / ho: what the
// kernel copies.  The plan counts the strip's whole footprint, floor(r bh / ho) +
// 2 rows, where that is more (it is from bh >= ho on): a reduction whose taps
// skip rows would stage bytes nobody reads, and is better off in the direct
// form.  Never more rows than the box holds.
inline int64_t rrc_strip_rows(int64_t r, int64_t bh, int64_t ho) {
  const int64_t taps = ((r - 1) * bh + ho - 1) / ho + 2, footprint = r * bh / ho + 2;
  const int64_t rows = taps > footprint ? taps : footprint;
  return rows < bh ? rows : bh;
}

// LDS of one workgroup of data_rrc.hip: the [4][256] bf16 look-up table, then per
// view the column table (wo x u32), three row tables of kRrcMaxStrip u32 and the
// staged source rows.  A staged row keeps its global 16-byte phase, so its pitch
// is the widest box row plus 15 bytes, rounded up to 16.
constexpr int kRrcMaxStrip = 8;
constexpr int64_t kRrcStageBudget = 48 * 1024;  // staged source bytes, both views together
constexpr int64_t kRrcLdsLimit = 64 * 1024;     // what a launch gets without an attribute
struct RrcPlan {
  bool staged;        // false: the four taps are gathered through L2
  int strip;          // R: output rows per workgroup
  int stage_rows;     // staged rows per view (0 in the direct form)
  int pitch;          // bytes between staged rows
  int table_bytes;    // look-up table + column and row tables, a multiple of 16
  int lds_bytes;      // dynamic LDS of the launch
};

// The largest strip of 8 / 4 / 2 / 1 output rows whose worst case (a box of the
// whole image) fits the staging budget, halved per view when two are staged
// (mix); the direct form, at the full strip, where not even one row does or
// where `direct` asks for it.
inline RrcPlan rrc_plan(int64_t hs, int64_t ws, int64_t c, int64_t ho, int64_t wo, bool mix,
                        bool direct = false) {
  const int64_t views = mix ? 2 : 1;
  RrcPlan p{};
  p.pitch = (int)((ws * c + 15 + 15) / 16 * 16);
  p.table_bytes = (int)((4 * 256 * 2 + views * (wo * 4 + 3 * kRrcMaxStrip * 4) + 15) / 16 * 16);
  p.strip = kRrcMaxStrip;
  int64_t budget = kRrcLdsLimit - p.table_bytes;
  if (budget > kRrcStageBudget) budget = kRrcStageBudget;
  for (int r = kRrcMaxStrip; r >= 1 && !direct; r /= 2) {
    const int64_t rows = rrc_strip_rows(r, hs, ho);
    if (rows * p.pitch * views <= budget) {
      p.staged = true;
      p.strip = r;
      p.stage_rows = (int)rows;
      break;
    }
  }
  p.lds_bytes = p.table_bytes + (int)(views * p.stage_rows * p.pitch);
  return p;
}

}  // namespace guard
}  // namespace dmp
