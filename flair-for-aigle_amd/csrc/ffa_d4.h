// What the D4 passes share (augment.hip: the layout / label kernels of a batch tensor; sample_gather.hip: the same
// passes reading a device-resident sample store through an index vector; series_gather.hip: the layout pass reading a
// ragged store of time series): the code -> source-rectangle map, the tile
// sizes, the normalisation expression and the layout pass of one tile itself (d4_layout_image).  One definition, so that
// the two families agree bit for bit by construction.
//
// One uint8 code per sample: bit 0 horizontal flip, bit 1 vertical flip, bits 2-3 k.  The reference flips axis -1, flips
// axis -2, then rot90(k); for a square n x n plane out[i, j] = in[si, sj] with (si, sj) = (i, j), k times
// (si, sj) <- (sj, n-1-si), then si <- n-1-si if vflip, sj <- n-1-sj if hflip.  In closed form: odd k swaps the roles
// of i and j, and each source coordinate is either the destination coordinate or its mirror image (d4_decode).
#pragma once
#include "ffa_common.h"

#define FFA_D4_THREADS 256
#define FFA_D4_TS 32                    // layout tile: 32 x 32 pixels, one destination row of bf16 x 16 channels = 1 KB
#define FFA_D4_PITCH (FFA_D4_TS + 1)    // floats
#define FFA_D4_LTS 64                   // label tile: 64 x 64 bytes
#define FFA_D4_LPITCH (FFA_D4_LTS + 4)  // bytes: 17 dwords

struct D4Map {
  int swap, fi, fj;        // source row comes from the destination column (odd k); mirrored source row / column
  int i0, j0, th, tw;      // destination tile: origin and extent (clipped to the plane)
  int si0, sj0, srows, scols;  // source tile
};

__device__ __forceinline__ D4Map d4_decode(int code, int n, int tile, int ts) {
  const int nt = (n + ts - 1) / ts;
  D4Map m;
  const int k = (code >> 2) & 3;
  m.swap = k & 1;
  m.fi = (k >> 1) ^ ((code >> 1) & 1);               // k = 2, 3 mirror the source row; so does the vertical flip
  m.fj = ((k == 1 || k == 2) ? 1 : 0) ^ (code & 1);  // k = 1, 2 mirror the source column; so does the horizontal flip
  m.i0 = (tile / nt) * ts;
  m.j0 = (tile % nt) * ts;
  m.th = min(ts, n - m.i0);
  m.tw = min(ts, n - m.j0);
  const int a0 = m.swap ? m.j0 : m.i0, al = m.swap ? m.tw : m.th;  // the destination axis the source row follows
  const int b0 = m.swap ? m.i0 : m.j0, bl = m.swap ? m.th : m.tw;  // ... and the source column
  m.srows = al;
  m.scols = bl;
  m.si0 = m.fi ? n - a0 - al : a0;
  m.sj0 = m.fj ? n - b0 - bl : b0;
  return m;
}

// the identity on an H x W plane (no code: nothing is flipped or rotated, so the plane need not be square)
__device__ __forceinline__ D4Map d4_identity(int H, int W, int tile, int ts) {
  const int ntw = (W + ts - 1) / ts;
  D4Map m;
  m.swap = m.fi = m.fj = 0;
  m.i0 = (tile / ntw) * ts;
  m.j0 = (tile % ntw) * ts;
  m.th = min(ts, H - m.i0);
  m.tw = min(ts, W - m.j0);
  m.srows = m.th;
  m.scols = m.tw;
  m.si0 = m.i0;
  m.sj0 = m.j0;
  return m;
}

// destination pixel (li, lj) of the tile -> its source pixel's position in the staged source tile
__device__ __forceinline__ void d4_local(const D4Map& m, int li, int lj, int& r, int& c) {
  const int a = m.swap ? lj : li, b = m.swap ? li : lj;
  r = m.fi ? m.srows - 1 - a : a;
  c = m.fj ? m.scols - 1 - b : b;
}

// the normalisation of every layout pass: a division, never a multiplication by a reciprocal
__device__ __forceinline__ float d4_norm(float s, float mu, float sd) { return (s - mu) / sd; }

template <typename S>
struct D4Vec4;  // four consecutive source samples in one load
template <>
struct D4Vec4<uint8_t> { typedef uchar4 type; };
template <>
struct D4Vec4<uint16_t> { typedef ushort4 type; };
template <>
struct D4Vec4<int16_t> { typedef short4 type; };
template <>
struct D4Vec4<float> { typedef float4 type; };

// the staged 64 x 64 source tile of class indices -> the destination tile, one byte per thread and step (a wave
// writes 64 consecutive bytes of a destination row); pitch: bytes between destination rows
__device__ __forceinline__ void d4_store_label_tile(const D4Map& m, const uint8_t* tile, uint8_t* __restrict__ dst,
                                                    int pitch) {
  for (int e = threadIdx.x; e < FFA_D4_LTS * FFA_D4_LTS; e += FFA_D4_THREADS) {
    const int li = e / FFA_D4_LTS, lj = e % FFA_D4_LTS;
    if (li >= m.th || lj >= m.tw) continue;
    int r, c;
    d4_local(m, li, lj, r, c);
    dst[(long long)(m.i0 + li) * pitch + m.j0 + lj] = tile[r * FFA_D4_LPITCH + c];
  }
}

// ---- the layout pass of one tile of one image, shared by d4_nchw_to_nhwc_kernel and gather_layout_kernel ----
// FFA_ELEV_* (flairhip_gather.h): how the C output channels are made of the stored ones of a 2-band elevation sample
template <typename S>
__device__ __forceinline__ float d4_sample(const S* __restrict__ img, long long hw, long long off, int c, int elev) {
  // output channel c of one source pixel: as stored, or built from the two elevation bands
  if (elev == FFA_ELEV_NONE) return (float)img[c * hw + off];
  const float z0 = (float)img[off];
  if (elev == FFA_ELEV_STACK && c == 0) return z0;
  return z0 - (float)img[hw + off];
}


// simg: the source image's planes (pitch hw = H * W samples, rows of W), dimg: the destination image [H][W][Cp]; the
// tile m of it.  Dynamic LDS: [min(C, 8)][FFA_D4_TS][FFA_D4_PITCH] floats.  Channels go through LDS eight at a time (one
// 16-byte bf16 piece per pixel); the pass that holds the last real channels also writes the all-zero pad groups, and a
// thread's piece index runs (pixel, group) with the group fastest, so for the few-channel inputs (C <= 8) a wave stores
// whole pixels back to back.  vec4: W % 4 == 0 and aligned planes, four samples per load (FFA_ELEV_NONE only).
template <typename S, typename T>
__device__ __forceinline__ void d4_layout_image(const D4Map& m, const S* __restrict__ simg, T* __restrict__ dimg, int C,
                                                int W, long long hw, int Cp, const float* __restrict__ mean,
                                                const float* __restrict__ stdv, int vec4, int elev) {
  extern __shared__ float d4_tile[];
  const int groups = Cp / 8;
  const int passes = C > 8 ? (C + 7) / 8 : 1;
  constexpr int PLANE = FFA_D4_TS * FFA_D4_PITCH;
  for (int p = 0; p < passes; ++p) {
    const int c0 = p * 8;
    const int nc = min(8, C - c0);
    if (p) __syncthreads();
    // ---- source tile -> LDS, normalised ----
    for (int c = 0; c < nc; ++c) {
      const bool norm = mean != nullptr;
      const float mu = norm ? mean[c0 + c] : 0.f, sd = norm ? stdv[c0 + c] : 1.f;
      float* t = d4_tile + c * PLANE;
      if (vec4 && elev == FFA_ELEV_NONE) {  // W % 4 == 0: tile origins and extents are multiples of 4
        const S* plane = simg + (c0 + c) * hw;
        const int r = threadIdx.x / (FFA_D4_TS / 4), q = (threadIdx.x % (FFA_D4_TS / 4)) * 4;
        if (r < m.srows && q < m.scols) {
          const typename D4Vec4<S>::type v = *reinterpret_cast<const typename D4Vec4<S>::type*>(
              plane + (long long)(m.si0 + r) * W + m.sj0 + q);
          float* o = t + r * FFA_D4_PITCH + q;
          if (norm) {
            o[0] = d4_norm((float)v.x, mu, sd);
            o[1] = d4_norm((float)v.y, mu, sd);
            o[2] = d4_norm((float)v.z, mu, sd);
            o[3] = d4_norm((float)v.w, mu, sd);
          } else {
            o[0] = (float)v.x;
            o[1] = (float)v.y;
            o[2] = (float)v.z;
            o[3] = (float)v.w;
          }
        }
      } else {
        for (int e = threadIdx.x; e < FFA_D4_TS * FFA_D4_TS; e += FFA_D4_THREADS) {
          const int r = e / FFA_D4_TS, q = e % FFA_D4_TS;
          if (r < m.srows && q < m.scols) {
            const float s = d4_sample<S>(simg, hw, (long long)(m.si0 + r) * W + m.sj0 + q, c0 + c, elev);
            t[r * FFA_D4_PITCH + q] = norm ? d4_norm(s, mu, sd) : s;
          }
        }
      }
    }
    __syncthreads();
    // ---- LDS -> destination pixels, 16-byte pieces in memory order ----
    const int g0 = p;                                    // the group of this pass's real channels ...
    const int ng = (p == passes - 1) ? groups - g0 : 1;  // ... and, with the last one, the pad groups behind it
    for (int e = threadIdx.x; e < FFA_D4_TS * FFA_D4_TS * ng; e += FFA_D4_THREADS) {
      const int pix = ng == 1 ? e : ng == 2 ? e >> 1 : e / ng;
      const int g = g0 + e - pix * ng;
      const int li = pix / FFA_D4_TS, lj = pix % FFA_D4_TS;
      if (li >= m.th || lj >= m.tw) continue;
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = 0.f;
      if (g == g0) {
        int r, c;
        d4_local(m, li, lj, r, c);
        const float* t = d4_tile + r * FFA_D4_PITCH + c;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < nc) v[k] = t[k * PLANE];
      }
      ffa_store8<T>(dimg + ((long long)(m.i0 + li) * W + m.j0 + lj) * Cp + g * 8, v);
    }
  }
}

