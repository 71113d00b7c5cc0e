// Index maps of the position-major ("PM") form of conv_halo_kernel: 3x3 / stride 1
// / pad 1 on 4 x 4 maps, BM 256 = 16 whole images per tile, WM 4, TM 4.
//
// The dense kernel's 16-row MFMA fragment is 16 consecutive pixels = one whole
// 4 x 4 image, so every fragment has a valid row for every tap and all nine taps
// run, although 44 of the 144 (pixel, tap) pairs of an image read the zero halo.
// Here a fragment is ONE pixel position across the tile's 16 images: a tap is in
// the image for the whole fragment or for none of it, and the dead (fragment,
// tap) pairs -- their ds_read_b128 and their MFMAs -- are not issued.  No halo is
// staged either: only the images' real pixels.
//
// Plain constexpr C++ (no HIP, no torch): the kernel (conv.hip), the planner
// (halo_plan.h) and the CPU checker (halo_pm_check.cpp) share these functions.
#pragma once

namespace dmp {
namespace pm {

constexpr int kH = 4, kW = 4, kImg = kH * kW;   // the map
constexpr int kBM = 256, kWM = 4, kTM = 4;      // tile rows, waves along M, fragments per wave
constexpr int kTB = kBM / kImg;                 // images per tile = rows of a fragment (16)

// ---------------------------------------------------------- fragment -> position
// Fragment i of wave row wm is pixel (h, w) = (i, (i + wm) & 3), fragment row
// (lane & 15) is image tb of the tile.  The Latin square gives the four wave rows
// 26 / 25 / 24 / 25 live (fragment, tap) pairs of 36, and the two waves of one
// SIMD (wm, wm + 2) 50 of 72 on every SIMD: the 100 / 144 average, no imbalance.
constexpr int frag_h(int /*wm*/, int i) { return i; }
constexpr int frag_w(int wm, int i) { return (i + wm) & 3; }
constexpr int frag_pos(int wm, int i) { return frag_h(wm, i) * kW + frag_w(wm, i); }

// ------------------------------------------------------------------ tap validity
// tap t = (t / 3, t % 3) of the ACTIVATION (the data gradient mirrors only the
// weight tap, 8 - t): true iff it reads a pixel inside the image
constexpr bool tap_valid(int h, int w, int t) {
  const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
  return hh >= 0 && hh < kH && ww >= 0 && ww < kW;
}
constexpr bool live(int wm, int i, int t) { return tap_valid(frag_h(wm, i), frag_w(wm, i), t); }
constexpr int live_count(int wm, int t) {
  int n = 0;
  for (int i = 0; i < kTM; ++i) n += live(wm, i, t) ? 1 : 0;
  return n;
}
// pixel-index shift of tap t: source pixel = p + tap_shift(t) where the tap is valid
constexpr int tap_shift(int t) { return (t / 3 - 1) * kW + (t % 3 - 1); }

// --------------------------------------------------------------- staged A image
// Only real pixels: the row of (image tb, pixel p) is tb * kPI + p.  kPI = 17 is
// odd, so the 16 images of one position fall on all four 64-B quarters of the
// 256-B bank row; row 16 of every image block is a pad row (staged as zeros,
// never read).
constexpr int kPI = kImg + 1;
constexpr int kRows = kTB * kPI;       // 272 staged rows
constexpr int kPieces = kRows / 16;    // 17 LDS-DMA pieces of 16 rows x 64 B (BK 32)
static_assert(kRows % 16 == 0, "whole DMA pieces");
constexpr int staged_row(int tb, int p) { return tb * kPI + p; }
// DMA slot: staged row -> image of the tile and pixel (p == kImg: the pad row)
constexpr int row_tb(int row) { return row / kPI; }
constexpr int row_p(int row) { return row % kPI; }
// 16-B chunk swizzle of a staged row (an involution, keyed on the image): with the
// odd pitch it puts the 16 lanes of every ds_read_b128 lane group on 16 distinct
// 16-B slots (halo_pm_check.cpp counts them over every live read)
constexpr int swz(int tb, int c) { return c ^ ((tb >> 3) << 1); }

// -------------------------------------------------------------------- epilogue
// tile row ml = wm * 64 + i * 16 + tb of the accumulator fragments -> pixel of
// the tile (pixel m0 + tb * 16 + p of the output)
constexpr int out_pixel(int ml) {
  return (ml & 15) * kImg + frag_pos(ml >> 6, (ml >> 4) & 3);
}
// The row-staged epilogue's LDS tile gets this many extra elements per image: a
// fragment's 16 rows are 16 pixels apart there (16 x 144 B = 9 bank rows), and
// 16 B more per image spreads them over the banks like 16 consecutive rows
constexpr int kEpiSkew = 8;
constexpr int epi_elems(int bn) { return kBM * (bn + 8) + (kTB - 1) * kEpiSkew; }

}  // namespace pm
}  // namespace dmp
