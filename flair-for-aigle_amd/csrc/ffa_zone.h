// The crossing rule of the zone rasterisers (zone_mask.hip, zone_stats.hip), in one place so that the two cannot drift.
// include/flairhip.h ("geozone clipping") holds the normative text.
#pragma once
#include "ffa_common.h"

// xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) must round every operation separately: no a * b + c -> fma.  The pragma
// holds from here to the end of the translation unit; the including files state it again ahead of their own code.
#pragma clang fp contract(off)

// Does the edge (x0, y0) -> (x1, y1) cross pixel row r (yc = r + 0.5), and at which column does it toggle?  *col is
// floor(xc - 0.5) + 1 clamped to [0, W]: a toggle at W has no effect.  A NaN (overflow in the product) lands on column 0,
// like any far-left crossing.
__device__ __forceinline__ bool ffa_zone_crossing(double x0, double y0, double x1, double y1, int r, int W, int* col) {
  const double yc = (double)r + 0.5;
  if ((y0 <= yc) == (y1 <= yc)) return false;
  const double xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0);
  double t = floor(xc - 0.5) + 1.0;
  t = fmin(fmax(t, 0.0), (double)W);
  *col = (int)t;
  return true;
}

// Prefix XOR inside a word: bit k = XOR of the word's bits <= k; bit 31 = parity of the word.
__device__ __forceinline__ unsigned int ffa_zone_prefix_xor(unsigned int p) {
  p ^= p << 1;
  p ^= p << 2;
  p ^= p << 4;
  p ^= p << 8;
  p ^= p << 16;
  return p;
}
