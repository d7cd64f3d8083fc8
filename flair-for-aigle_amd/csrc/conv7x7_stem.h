// Geometry of conv7x7_stem_kernel (conv7x7_stem.hip), shared with the packer of its weight operand (conv_pack.hip).
#pragma once

struct StemGeom {
  static constexpr int TH = 16, TW = 32, NW = 8, NTHR = 512;
  static constexpr int IH = 2 * TH + 5;           // 37 input rows
  static constexpr int IWH = 36;                  // pixel pairs per row and parity (2 * TW + 5 = 69 columns)
  static constexpr int ROWP = 2 * IWH;            // 16-byte pieces per halo row: [parity][IWH]
  static constexpr int HP = IH * ROWP;            // 2664 pieces
  static constexpr int NHW = (HP + NTHR - 1) / NTHR;
  static constexpr int HBYTES = HP * 16;
  static constexpr int KSTEPS = 14;
  static constexpr int WBYTES = KSTEPS * 4096;    // [k-step][64 rows][64 B]
  static constexpr int WP = WBYTES / 16;
  static constexpr int W_OFF = 0, H_OFF = WBYTES, RED_OFF = WBYTES + 2 * HBYTES;
  static constexpr int RED_BYTES = NW * 64 * 2 * 4;
  static constexpr int LDS_BYTES = RED_OFF + RED_BYTES;
  static_assert(WP % NTHR == 0, "every thread issues the same number of weight pieces");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
