// Weight packing: the OIHW f32 master weight of a convolution -> the MFMA operand of the kernel that ffa_conv_plan
// chose for the layer.  The layout rides in the high bits of `bco` (none: conv_igemm.hip, FFA_BCO_RING:
// conv3x3_ring.hip, FFA_BCO_THIN: conv3x3_thin.hip, FFA_BCO_STEM: conv7x7_stem.hip).  Every layout shares one
// descriptor (PackDesc), one host fill (pack_fill) and one launch (pack_launch); each has ONE kernel, which serves the
// one-off call (descriptor in the kernel arguments) and the batched one (blockIdx.y selects a descriptor of a table in
// device memory, built once on the host and replayed every optimizer step).  The kernels stay apart on purpose:
// ring16_pack_rowslot holds 72 floats, and a merged kernel would give every layout its register footprint.
//
// A new layout adds its geometry fields to PackDesc, a case to pack_fill / ffa_pack_conv_weight_bytes / pack_launch,
// and a kernel.
#include "ffa_common.h"

#include "conv7x7_stem.h"

// src element (row, ch, r, s) is read at src[row*s_row + ch*s_ch + r*kw + s]; flip mirrors the taps (dgrad operand:
// rows = ci, ch = co, flipped).  scale[row] (optional) folds an eval-mode BatchNorm into the weights.
struct PackDesc {
  const float* src;
  void* dst;
  const float* scale;
  long long s_row, s_ch;
  int rows, chs;  // valid rows / channels in src
  int flip, kh, kw;
  int nchunks;       // conv_igemm: 32-byte chunks of the channel pitch; ring: 64-byte chunks
  int rg, bco, ncb;  // conv_igemm: kernel rows per chunk, rows per block, blocks
  int ncb64;         // ring: 64-row groups
  int mt, ci;        // thin: 16-row tiles, channel pitch
};
// Every kernel begins `PackDesc p = one; if (table) p = table[blockIdx.y];` -- two scalar loads and a uniform branch, so
// the descriptor stays in SGPRs.  `table ? table[blockIdx.y] : one` selects between a kernel-argument and a global
// ADDRESS instead: the loads go through a flat pointer into VGPRs (+24 in every kernel, 28 bytes of scratch in the ring one).

// ------------------------------------------------------------------------------------------------
// conv_igemm layout: per-(co block, chunk, row group) LDS-image slabs
//   dst[cb][cc][rg][row < BCO][tap < RG*KW][e < 32/sizeof(T)]

// one thread = eight consecutive channels of one (row, tap): the index arithmetic (seven divisions by run-time
// values) is paid once per 16-byte store instead of once per element (201 -> ~50 us for the 186 operands of the
// U-Net at batch time)
__device__ __forceinline__ void pack_eight(const PackDesc& p, long long i8, int dtype) {
  const int EPC = (dtype == FFA_BF16) ? 16 : 8;
  const int G8 = EPC / 8;
  const int taps = p.rg * p.kw;
  const int nrg = p.kh / p.rg;
  long long t = i8;
  const int e0 = (int)(t % G8) * 8; t /= G8;
  const int tap = t % taps; t /= taps;
  const int row_l = t % p.bco; t /= p.bco;
  const int rg = t % nrg; t /= nrg;
  const int cc = t % p.nchunks; t /= p.nchunks;
  const int cb = (int)t;
  int row_in_block = row_l;
  if (p.bco >= 64) {  // fragment order inside each 64-row wave group (see conv_igemm_kernel)
    const int j = row_l & 63, mt = j >> 5, rho = j & 31;
    row_in_block = (row_l & ~63) + 16 * (rho >> 3) + 8 * ((rho >> 2) & 1) + 4 * mt + (rho & 3);
  }
  const int row = cb * p.bco + row_in_block;
  const int ch0 = cc * EPC + e0;
  int r = rg * p.rg + tap / p.kw;
  int sx = tap % p.kw;
  if (p.flip) {
    r = p.kh - 1 - r;
    sx = p.kw - 1 - sx;
  }
  float v[8];
  const bool row_ok = row < p.rows;
  const float sc = (row_ok && p.scale) ? p.scale[row] : 1.f;
  const float* src = p.src + (long long)row * p.s_row + r * p.kw + sx;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = ch0 + j;
    v[j] = (row_ok && ch < p.chs) ? src[(long long)ch * p.s_ch] * sc : 0.f;
  }
  if (dtype == FFA_BF16)
    ffa_store8<ffa_bf16>(static_cast<ffa_bf16*>(p.dst) + i8 * 8, v);
  else
    ffa_store8<float>(static_cast<float*>(p.dst) + i8 * 8, v);
}

__global__ void pack_igemm_kernel(PackDesc one, const PackDesc* __restrict__ table, int dtype) {
  PackDesc p = one;
  if (table) p = table[blockIdx.y];
  const int EPC = (dtype == FFA_BF16) ? 16 : 8;
  const long long total8 = (long long)p.ncb * p.nchunks * (p.kh / p.rg) * p.bco * (p.rg * p.kw) * (EPC / 8);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8;
       i += (long long)gridDim.x * blockDim.x)
    pack_eight(p, i, dtype);
}

// ------------------------------------------------------------------------------------------------
// ring layout (f32 operand of conv3x3_ring_kernel):
//   dst[cb64][chunk][kernel row r][tap s][k-step][row < 64 (fragment order)][half'][elements of 16 B]
// half' = half ^ bit 3 of the row.

template <typename T>
__device__ __forceinline__ void ring_pack_piece(const PackDesc& p, long long i16) {
  // one thread = one 16-byte piece
  constexpr int EPF = ElemTraits<T>::kPerFrag;
  long long t = i16;
  const int hp = (int)(t % 2); t /= 2;
  const int row_l = (int)(t % 64); t /= 64;
  const int ks = (int)(t % 2); t /= 2;
  const int s = (int)(t % 3); t /= 3;
  const int r = (int)(t % 3); t /= 3;
  const int cc = (int)(t % p.nchunks); t /= p.nchunks;
  const int cb = (int)t;
  const int mt = row_l >> 5, rho = row_l & 31;
  const int row = cb * 64 + 16 * (rho >> 3) + 8 * ((rho >> 2) & 1) + 4 * mt + (rho & 3);
  const int hsrc = hp ^ ((row_l >> 3) & 1);
  const int ch0 = cc * (4 * EPF) + ks * (2 * EPF) + hsrc * EPF;
  int rr = r, ss = s;
  if (p.flip) {
    rr = 2 - r;
    ss = 2 - s;
  }
  float v[8];
  const bool row_ok = row < p.rows;
  const float sc = (row_ok && p.scale) ? p.scale[row] : 1.f;
  const float* src = p.src + (long long)row * p.s_row + rr * 3 + ss;
#pragma unroll
  for (int j = 0; j < EPF; ++j) {
    const int ch = ch0 + j;
    v[j] = (row_ok && ch < p.chs) ? src[(long long)ch * p.s_ch] * sc : 0.f;
  }
  if constexpr (EPF == 8) {
    ffa_store8<ffa_bf16>(static_cast<ffa_bf16*>(p.dst) + i16 * 8, v);
  } else {
    *reinterpret_cast<float4*>(static_cast<float*>(p.dst) + i16 * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// bf16 operand of conv3x3_ring16_kernel: dst[cb64][chunk][kernel row r][tap s][row < 64][slot' < 4][8 elements],
// LDS row mt*16 + 4*kg + i holds output channel 16*kg + 4*mt + i of the 64-row group, slot' = slot ^ 2 when bit 2 of
// the row is set (slot = channels 8*slot .. 8*slot+7 of the 32-channel chunk).  Same bytes per (group, chunk) as the
// 32x32 layout, so sizes and strides are shared.
// One thread = one (row, 16-byte slot) of a chunk, all nine taps: it reads 8 channels x 9 contiguous taps of the OIHW
// master (36-byte runs; a thread per piece touched a 32-byte sector per 4 useful bytes: 287 us per step for the
// U-Net's operands) and writes its nine pieces, one into each tap plane.  Threads of a block run over the 64 rows first,
// so the transposed (dgrad) operand -- whose rows are the contiguous axis of the master -- reads whole runs too.
__device__ __forceinline__ void ring16_pack_rowslot(const PackDesc& p, long long idx) {
  // lanes follow the contiguous axis of the master: (slot, chunk) = consecutive 288-byte runs of one row for the
  // forward operand [row][ch][tap]; rows = consecutive 36-byte runs for the transposed one [ch][row][tap]
  long long t = idx;
  int row_l, sp, cc;
  if (!p.flip) {
    sp = (int)(t % 4); t /= 4;
    cc = (int)(t % p.nchunks); t /= p.nchunks;
    row_l = (int)(t % 64); t /= 64;
  } else {
    row_l = (int)(t % 64); t /= 64;
    sp = (int)(t % 4); t /= 4;
    cc = (int)(t % p.nchunks); t /= p.nchunks;
  }
  const int cb = (int)t;
  const int mt = row_l >> 4, kg = (row_l >> 2) & 3, i = row_l & 3;
  const int row = cb * 64 + 16 * kg + 4 * mt + i;
  const int slot = sp ^ (((row_l >> 2) & 1) << 1);
  const int ch0 = cc * 32 + slot * 8;
  const bool row_ok = row < p.rows;
  const float sc = (row_ok && p.scale) ? p.scale[row] : 1.f;
  float v[8][9];
  if (!p.flip && row_ok && ch0 + 8 <= p.chs && (p.s_row & 3) == 0 && ((size_t)p.src & 15) == 0) {
    // forward operand: the 8 channels x 9 taps of this thread are 72 CONTIGUOUS floats of the master -> 18 16-byte
    // loads (a 4-byte load per element made every wave instruction touch 64 cache lines: 171 us per step)
    const ffa_f32x4* src4 = reinterpret_cast<const ffa_f32x4*>(p.src + (long long)row * p.s_row + (long long)ch0 * 9);
    float f[72];
#pragma unroll
    for (int q = 0; q < 18; ++q) {
      const ffa_f32x4 t4 = src4[q];
      f[4 * q] = t4[0]; f[4 * q + 1] = t4[1]; f[4 * q + 2] = t4[2]; f[4 * q + 3] = t4[3];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) v[j][tp] = f[j * 9 + tp] * sc;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = ch0 + j;
      const bool ok = row_ok && ch < p.chs;
      const float* src = p.src + (long long)(ok ? row : 0) * p.s_row + (long long)(ok ? ch : 0) * p.s_ch;
      // destination tap tp reads source tap tp, or 8 - tp for the mirrored (dgrad) operand: the choice goes into the
      // ADDRESS -- indexing v[][] with a run-time value would send the array to scratch memory
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) v[j][tp] = ok ? src[p.flip ? 8 - tp : tp] * sc : 0.f;
    }
  }
  ffa_bf16* dst = static_cast<ffa_bf16*>(p.dst) + ((((long long)cb * p.nchunks + cc) * 9) * 256 + row_l * 4 + sp) * 8;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp) {  // destination tap (r, s) = tp
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = v[j][tp];
    ffa_store8<ffa_bf16>(dst + (long long)tp * 256 * 8, o);
  }
}

__global__ void pack_ring_kernel(PackDesc one, const PackDesc* __restrict__ table, int dtype) {
  PackDesc p = one;
  if (table) p = table[blockIdx.y];
  if (dtype == FFA_BF16) {
    const long long total = (long long)p.ncb64 * p.nchunks * 64 * 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
      ring16_pack_rowslot(p, i);
    return;
  }
  const long long total = (long long)p.ncb64 * p.nchunks * 3 * 3 * 2 * 64 * 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    ring_pack_piece<float>(p, i);
}

// ------------------------------------------------------------------------------------------------
// thin layout: dst[mt][k-step][lane][8 bf16], lane = (row = lane & 15, kg = lane >> 4)
//   tile row 4*q + i of tile mt  <->  output channel 8*q + 4*mt + i (two tiles) / 4*q + i (one tile)
//   32 channels: k-step = tap, elements = channels 8*kg .. 8*kg+7
//   16 channels: k-step = taps (2*ks, 2*ks + 1); kg >> 1 picks the tap (tap 9 = zeros), kg & 1 the channel half

__device__ __forceinline__ void thin_pack_piece(const PackDesc& p, int idx) {
  const int ks_n = (p.ci == 32) ? 9 : 5;
  const int lane = idx % 64;
  const int ks = (idx / 64) % ks_n;
  const int mt = idx / (64 * ks_n);
  const int r = lane & 15, kg = lane >> 4;
  const int q = r >> 2, i = r & 3;
  const int row = (p.mt == 2) ? (8 * q + 4 * mt + i) : (4 * q + i);
  int tap, ch0;
  if (p.ci == 32) {
    tap = ks;
    ch0 = 8 * kg;
  } else {
    tap = 2 * ks + (kg >> 1);
    ch0 = 8 * (kg & 1);
  }
  float v[8];
  const bool ok = row < p.rows && tap < 9;
  const float sc = (ok && p.scale) ? p.scale[row] : 1.f;
  const int st = p.flip ? 8 - tap : tap;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = ch0 + j;
    v[j] = (ok && ch < p.chs) ? p.src[(long long)row * p.s_row + (long long)ch * p.s_ch + st] * sc : 0.f;
  }
  ffa_store8<ffa_bf16>(static_cast<ffa_bf16*>(p.dst) + (long long)idx * 8, v);
}

__global__ void pack_thin_kernel(PackDesc one, const PackDesc* __restrict__ table) {
  PackDesc p = one;
  if (table) p = table[blockIdx.y];
  const int total = p.mt * ((p.ci == 32) ? 9 : 5) * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) thin_pack_piece(p, i);
}

// ------------------------------------------------------------------------------------------------
// stem layout: dst[k-step = r * 2 + half][LDS row rho][slot'][8 channels] (bf16), LDS row rho = mt * 16 + 4 * q + i
// holds output channel 16 * q + 4 * mt + i (so that an accumulator lane ends up with 16 consecutive channels), slot =
// tap 4 * half + slot of kernel row r (tap 7: zeros), slot' = slot ^ 2 when bit 2 of rho.  rows = O <= 64, chs = I <= 8.

__global__ void pack_stem_kernel(PackDesc one, const PackDesc* __restrict__ table) {
  PackDesc p = one;
  if (table) p = table[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // one thread = one 16-byte slot
  if (i >= StemGeom::KSTEPS * 64 * 4) return;
  const int slotp = i & 3, rho = (i >> 2) & 63, ks = i >> 8;
  const int slot = slotp ^ (((rho >> 2) & 1) << 1);
  const int r = ks >> 1, s = 4 * (ks & 1) + slot;
  const int mt = rho >> 4, q = (rho >> 2) & 3, ii = rho & 3;
  const int co = 16 * q + 4 * mt + ii;
  unsigned short v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float x = 0.f;
    if (co < p.rows && c < p.chs && s < 7) {
      x = p.src[((size_t)(co * p.chs + c) * 7 + r) * 7 + s];
      if (p.scale) x *= p.scale[co];
    }
    v[c] = ffa_f32_to_bf16_bits(x);
  }
  uint4 u;
  u.x = v[0] | ((unsigned)v[1] << 16);
  u.y = v[2] | ((unsigned)v[3] << 16);
  u.z = v[4] | ((unsigned)v[5] << 16);
  u.w = v[6] | ((unsigned)v[7] << 16);
  reinterpret_cast<uint4*>(p.dst)[i] = u;
}

// ------------------------------------------------------------------------------------------------
// host side

// Descriptor of the column block W[:, col0 : col0 + ncols] of a weight with I_total input channels (the whole tensor:
// col0 = 0, ncols = I_total).  A proper block is one modality's share of a FusionHandler 1x1 convolution
// (flair_hub/models/flair_model.py:470-475,533-541): the source strides stay those of the whole tensor, so the slices
// of every stage ride in the batched pack instead of one copy + one pack launch each.  ffa_conv_plan gives a 1x1 operand
// no other layout than conv_igemm's, so only that layout takes one.
// co_rows / ci_pitch: padded row count (a multiple of the block size in `bco`) and the channel pitch of the activation
// the conv will read.  transpose = 1 builds the dgrad operand from the same OIHW tensor (rows = input channels,
// channels = output channels, taps mirrored).
static int pack_fill(PackDesc& p, const float* w_oihw, const float* scale, void* dst, int O, int I_total, int col0,
                     int ncols, int kh, int kw, int transpose, int co_rows, int ci_pitch, int bco, int rg, int dtype) {
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "pack: bad dtype");
  FFA_REQUIRE(w_oihw && dst, "pack: null pointer");
  FFA_REQUIRE(col0 >= 0 && ncols > 0 && col0 + ncols <= I_total, "pack: column block outside the tensor");
  const int eb = (dtype == FFA_BF16) ? 2 : 4;
  memset(&p, 0, sizeof(p));
  p.src = w_oihw + (long long)col0 * kh * kw;
  p.dst = dst;
  p.scale = scale;
  if (!transpose) {
    p.rows = O; p.chs = ncols;
    p.s_row = (long long)I_total * kh * kw;
    p.s_ch = (long long)kh * kw;
    p.flip = 0;
  } else {
    p.rows = ncols; p.chs = O;
    p.s_row = (long long)kh * kw;
    p.s_ch = (long long)I_total * kh * kw;
    p.flip = 1;
  }
  p.kh = kh; p.kw = kw;
  FFA_REQUIRE(p.rows <= co_rows && p.chs <= ci_pitch, "pack: padded dims smaller than the tensor");
  FFA_REQUIRE(ncols == I_total || !(bco & (FFA_BCO_STEM | FFA_BCO_THIN | FFA_BCO_RING)),
              "pack: a column block needs the conv_igemm layout");
  if (bco & FFA_BCO_STEM) {
    FFA_REQUIRE(kh == 7 && kw == 7 && dtype == FFA_BF16 && !transpose, "pack: the stem layout is for the bf16 7x7 forward operand");
    FFA_REQUIRE(O > 0 && O <= 64 && ncols > 0 && ncols <= 8, "stem pack: 1..64 output and 1..8 input channels, got %d / %d", O, ncols);
  } else if (bco & FFA_BCO_THIN) {
    FFA_REQUIRE(kh == 3 && kw == 3 && dtype == FFA_BF16, "pack: the thin layout is for bf16 3x3 kernels");
    FFA_REQUIRE((co_rows == 16 || co_rows == 32) && (ci_pitch == 16 || ci_pitch == 32), "thin pack: rows %d / pitch %d",
                co_rows, ci_pitch);
    p.mt = co_rows / 16;
    p.ci = ci_pitch;
  } else if (bco & FFA_BCO_RING) {
    FFA_REQUIRE(kh == 3 && kw == 3, "pack: the ring layout is for 3x3 kernels");
    FFA_REQUIRE(co_rows % 64 == 0 && (ci_pitch * eb) % 64 == 0, "ring pack: rows %d / pitch %d not whole groups", co_rows,
                ci_pitch);
    p.nchunks = ci_pitch * eb / 64;
    p.ncb64 = co_rows / 64;
  } else {
    FFA_REQUIRE(bco > 0 && co_rows % bco == 0, "pack: rows %d not a multiple of block %d", co_rows, bco);
    FFA_REQUIRE(rg > 0 && kh % rg == 0, "pack: bad row group");
    FFA_REQUIRE(ci_pitch % 16 == 0, "pack: channel pitch must be a multiple of 16");
    p.rg = rg; p.bco = bco;
    p.nchunks = ci_pitch * eb / 32;
    p.ncb = co_rows / bco;
  }
  return FFA_OK;
}

// One launch for `n` descriptors of the layout in `bco`: the table when there is one, else `one`.
static int pack_launch(int dtype, int bco, const PackDesc& one, const PackDesc* table, int n, hipStream_t stream) {
  if (bco & FFA_BCO_STEM) {
    hipLaunchKernelGGL(pack_stem_kernel, dim3(ffa_cdiv(StemGeom::KSTEPS * 64 * 4, 256), n), dim3(256), 0, stream, one, table);
    return ffa_check_launch("pack_stem");
  }
  if (bco & FFA_BCO_THIN) {
    hipLaunchKernelGGL(pack_thin_kernel, dim3(5, n), dim3(256), 0, stream, one, table);
    return ffa_check_launch("pack_thin");
  }
  if (bco & FFA_BCO_RING) {
    hipLaunchKernelGGL(pack_ring_kernel, dim3(256, n), dim3(256), 0, stream, one, table, dtype);
    return ffa_check_launch("pack_ring");
  }
  // 256 blocks per descriptor: the largest operands (2.4 M elements) set the tail, small ones exit at once
  hipLaunchKernelGGL(pack_igemm_kernel, dim3(256, n), dim3(256), 0, stream, one, table, dtype);
  return ffa_check_launch("pack_igemm");
}

extern "C" long long ffa_pack_conv_weight_bytes(int dtype, int co_rows, int ci_pitch, int kh, int kw, int bco) {
  if (bco & FFA_BCO_STEM) return StemGeom::WBYTES;
  if (bco & FFA_BCO_THIN) return (long long)(co_rows / 16) * ((ci_pitch == 32) ? 9 : 5) * 1024;
  const long long eb = (dtype == FFA_BF16) ? 2 : 4;
  return (long long)co_rows * ci_pitch * kh * kw * eb;  // conv_igemm and ring: the padded tensor, permuted
}

extern "C" int ffa_pack_conv_weight(int dtype, const float* w_oihw, const float* scale, void* dst, int O, int I,
                                    int kh, int kw, int transpose, int co_rows, int ci_pitch, int bco, int rg,
                                    hipStream_t stream) {
  PackDesc p;
  const int rc = pack_fill(p, w_oihw, scale, dst, O, I, 0, I, kh, kw, transpose, co_rows, ci_pitch, bco, rg, dtype);
  if (rc != FFA_OK) return rc;
  return pack_launch(dtype, bco, p, nullptr, 1, stream);
}

extern "C" int ffa_pack_desc_bytes(void) { return (int)sizeof(PackDesc); }

// Fills one HOST descriptor (pointers are device pointers) of a table for ffa_pack_conv_weights_batched.
extern "C" int ffa_pack_desc_fill(void* host_desc, const float* w_oihw, const float* scale, void* dst, int O,
                                  int I_total, int col0, int ncols, int kh, int kw, int transpose, int co_rows,
                                  int ci_pitch, int bco, int rg, int dtype) {
  FFA_REQUIRE(host_desc, "pack_desc_fill: null pointer");
  PackDesc p;
  const int rc = pack_fill(p, w_oihw, scale, dst, O, I_total, col0, ncols, kh, kw, transpose, co_rows, ci_pitch, bco, rg,
                           dtype);
  if (rc != FFA_OK) return rc;
  memcpy(host_desc, &p, sizeof(p));
  return FFA_OK;
}

// Every operand of one layout (the layout bits of `bco`) in one launch.
extern "C" int ffa_pack_conv_weights_batched(int dtype, int bco, const void* descs_device, int n, hipStream_t stream) {
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "pack_batched: bad dtype");
  FFA_REQUIRE(descs_device && n > 0 && n <= 65535, "pack_batched: bad descriptor table");
  return pack_launch(dtype, bco, PackDesc{}, static_cast<const PackDesc*>(descs_device), n, stream);
}
