// Training augmentation inside the passes every input and label makes anyway: per-sample flips and rotations by
// k * 90 degrees (the reference's apply_numpy_augmentations, flair_hub/data/utils_data/augmentations.py:6-48) as a
// gather on the read side of the NCHW -> NHWC layout kernel, of the uint8 label copy and of the one-hot -> index
// reduction.  One uint8 code per sample, resident on the device (a captured training step replays with new codes):
//   bit 0 horizontal flip, bit 1 vertical flip, bits 2-3 k.  The reference flips axis -1, flips axis -2, then rot90(k);
// for a square n x n plane out[i, j] = in[si, sj] with (si, sj) = (i, j), k times (si, sj) <- (sj, n-1-si), then
// si <- n-1-si if vflip, sj <- n-1-sj if hflip.  In closed form: odd k swaps the roles of i and j, and each source
// coordinate is either the destination coordinate or its mirror image (d4_decode).
//
// A block works on one square pixel tile of one image, so the code and everything derived from it is wave-uniform.
// The source tile (the destination tile's pre-image: again an axis-aligned rectangle) is read row by row, coalesced,
// into LDS; the destination pixels are then written in memory order with 16-byte stores, reading LDS along a row
// (even k) or down a column (odd k: the pitch is odd in dwords, so a column falls on distinct banks).
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

// destination pixel (li, lj) of the tile -> its source pixel's position in the staged source tile
__device__ __forceinline__ void d4_local(const D4Map& m, int li, int lj, int& r, int& c) {
  const int a = m.swap ? lj : li, b = m.swap ? li : lj;
  r = m.fi ? m.srows - 1 - a : a;
  c = m.fj ? m.scols - 1 - b : b;
}

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

// grid: B * tiles blocks.  Channels go through LDS eight at a time (one 16-byte bf16 piece per pixel); the pass that
// holds the last real channels also writes the all-zero pad groups, and a thread's piece index runs (pixel, group) with
// the group fastest, so for the few-channel inputs (C <= 8) a wave stores whole pixels back to back.
template <typename S, typename T>
__global__ void __launch_bounds__(FFA_D4_THREADS)
d4_nchw_to_nhwc_kernel(const S* __restrict__ src, T* __restrict__ dst, int C, int n, int Cp,
                       const float* __restrict__ mean, const float* __restrict__ stdv,
                       const uint8_t* __restrict__ codes, int group, int vec4) {
  extern __shared__ float d4_tile[];  // [min(C, 8)][FFA_D4_TS][FFA_D4_PITCH]
  const int nt = (n + FFA_D4_TS - 1) / FFA_D4_TS;
  const int tiles = nt * nt;
  const int img = blockIdx.x / tiles;
  const D4Map m = d4_decode(codes[img / group] & 15, n, blockIdx.x % tiles, FFA_D4_TS);
  const long long hw = (long long)n * n;
  const int groups = Cp / 8;
  const int passes = C > 8 ? (C + 7) / 8 : 1;
  constexpr int PLANE = FFA_D4_TS * FFA_D4_PITCH;
  for (int p = 0; p < passes; ++p) {
    const int c0 = p * 8;
    const int nc = min(8, C - c0);
    if (p) __syncthreads();
    // ---- source tile -> LDS, normalised ----
    for (int c = 0; c < nc; ++c) {
      const S* plane = src + ((long long)img * C + c0 + c) * hw;
      const bool norm = mean != nullptr;
      const float mu = norm ? mean[c0 + c] : 0.f, sd = norm ? stdv[c0 + c] : 1.f;
      float* t = d4_tile + c * PLANE;
      if (vec4) {  // n % 4 == 0: tile origins and extents are multiples of 4, four samples per load
        const int r = threadIdx.x / (FFA_D4_TS / 4), q = (threadIdx.x % (FFA_D4_TS / 4)) * 4;
        if (r < m.srows && q < m.scols) {
          const typename D4Vec4<S>::type v = *reinterpret_cast<const typename D4Vec4<S>::type*>(
              plane + (long long)(m.si0 + r) * n + m.sj0 + q);
          float* o = t + r * FFA_D4_PITCH + q;
          if (norm) {
            o[0] = ((float)v.x - mu) / sd;
            o[1] = ((float)v.y - mu) / sd;
            o[2] = ((float)v.z - mu) / sd;
            o[3] = ((float)v.w - mu) / sd;
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
            const float s = (float)plane[(long long)(m.si0 + r) * n + m.sj0 + q];
            t[r * FFA_D4_PITCH + q] = norm ? (s - mu) / sd : s;
          }
        }
      }
    }
    __syncthreads();
    // ---- LDS -> destination pixels, 16-byte pieces in memory order ----
    const int g0 = p;                                    // the group of this pass's real channels ...
    const int ng = (p == passes - 1) ? groups - g0 : 1;  // ... and, with the last one, the pad groups behind it
    for (int e = threadIdx.x; e < FFA_D4_TS * FFA_D4_TS * ng; e += FFA_D4_THREADS) {
      // ng is block-uniform and 1 or 2 for every pitch in use (Cp 8, 16): no division there
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
      ffa_store8<T>(dst + ((long long)img * hw + (long long)(m.i0 + li) * n + m.j0 + lj) * Cp + g * 8, v);
    }
  }
}

template <typename S>
static int d4_layout_launch(int dtype, const void* src, void* dst, int B, int C, int n, int Cp, const float* mean,
                            const float* stdv, const uint8_t* codes, int group, hipStream_t stream) {
  const int nt = (n + FFA_D4_TS - 1) / FFA_D4_TS;
  const long long blocks = (long long)B * nt * nt;
  FFA_REQUIRE(blocks <= 0x7fffffffLL, "d4_nchw_to_nhwc: too many tiles");
  const int vec4 = (n % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % (4 * sizeof(S)) == 0);
  const size_t lds = (size_t)(C < 8 ? C : 8) * FFA_D4_TS * FFA_D4_PITCH * sizeof(float);
  if (dtype == FFA_BF16)
    hipLaunchKernelGGL((d4_nchw_to_nhwc_kernel<S, ffa_bf16>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)src, (ffa_bf16*)dst, C, n, Cp, mean, stdv, codes, group, vec4);
  else
    hipLaunchKernelGGL((d4_nchw_to_nhwc_kernel<S, float>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)src, (float*)dst, C, n, Cp, mean, stdv, codes, group, vec4);
  return ffa_check_launch("d4_nchw_to_nhwc");
}

extern "C" int ffa_d4_nchw_to_nhwc(int dtype, int src_kind, const void* src, void* dst, int B, int C, int H, int W,
                                   int Cp, const float* mean, const float* stdv, const uint8_t* codes, int group,
                                   hipStream_t stream) {
  FFA_REQUIRE(src && dst && codes && B >= 1 && C >= 1 && Cp % 8 == 0 && Cp >= C,
              "d4_nchw_to_nhwc: bad arguments (C=%d Cp=%d)", C, Cp);
  FFA_REQUIRE(H == W && H >= 1, "d4_nchw_to_nhwc: planes must be square, got %d x %d", H, W);
  FFA_REQUIRE((mean == nullptr) == (stdv == nullptr), "d4_nchw_to_nhwc: mean and std come together or not at all");
  FFA_REQUIRE(mean || src_kind == 3, "d4_nchw_to_nhwc: integer samples need mean / std");
  FFA_REQUIRE(group >= 1 && B % group == 0, "d4_nchw_to_nhwc: %d images do not split into groups of %d", B, group);
  switch (src_kind) {
    case 0: return d4_layout_launch<uint8_t>(dtype, src, dst, B, C, H, Cp, mean, stdv, codes, group, stream);
    case 1: return d4_layout_launch<uint16_t>(dtype, src, dst, B, C, H, Cp, mean, stdv, codes, group, stream);
    case 2: return d4_layout_launch<int16_t>(dtype, src, dst, B, C, H, Cp, mean, stdv, codes, group, stream);
    case 3: return d4_layout_launch<float>(dtype, src, dst, B, C, H, Cp, mean, stdv, codes, group, stream);
  }
  ffa_set_error("d4_nchw_to_nhwc: unknown source sample kind %d", src_kind);
  return FFA_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------
// labels: uint8 class-index maps, and the reference's f32 one-hot maps reduced to indices on the way

// the staged 64 x 64 source tile of class indices -> the destination tile, one byte per thread and step (a wave
// writes 64 consecutive bytes of a destination row)
__device__ __forceinline__ void d4_store_label_tile(const D4Map& m, const uint8_t* tile, uint8_t* __restrict__ dst,
                                                    int n) {
  for (int e = threadIdx.x; e < FFA_D4_LTS * FFA_D4_LTS; e += FFA_D4_THREADS) {
    const int li = e / FFA_D4_LTS, lj = e % FFA_D4_LTS;
    if (li >= m.th || lj >= m.tw) continue;
    int r, c;
    d4_local(m, li, lj, r, c);
    dst[(long long)(m.i0 + li) * n + m.j0 + lj] = tile[r * FFA_D4_LPITCH + c];
  }
}

__global__ void __launch_bounds__(FFA_D4_THREADS)
d4_labels_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n,
                    const uint8_t* __restrict__ codes) {
  __shared__ __align__(16) uint8_t tile[FFA_D4_LTS * FFA_D4_LPITCH];
  const int nt = (n + FFA_D4_LTS - 1) / FFA_D4_LTS;
  const int tiles = nt * nt;
  const int img = blockIdx.x / tiles;
  const D4Map m = d4_decode(codes[img] & 15, n, blockIdx.x % tiles, FFA_D4_LTS);
  const long long hw = (long long)n * n;
  const uint8_t* plane = src + img * hw;
  for (int e = threadIdx.x; e < FFA_D4_LTS * FFA_D4_LTS; e += FFA_D4_THREADS) {
    const int r = e / FFA_D4_LTS, q = e % FFA_D4_LTS;
    if (r < m.srows && q < m.scols) tile[r * FFA_D4_LPITCH + q] = plane[(long long)(m.si0 + r) * n + m.sj0 + q];
  }
  __syncthreads();
  d4_store_label_tile(m, tile, dst + img * hw, n);
}

__global__ void __launch_bounds__(FFA_D4_THREADS)
d4_onehot_to_index_kernel(const float* __restrict__ onehot, uint8_t* __restrict__ idx, int K, int n,
                          const uint8_t* __restrict__ codes) {
  // the first maximum over the K planes of every source pixel (ffa_onehot_to_index's rule), taken in source order so
  // that the K plane reads stay coalesced; the permutation happens on the one byte per pixel that is left
  __shared__ __align__(16) uint8_t tile[FFA_D4_LTS * FFA_D4_LPITCH];
  const int nt = (n + FFA_D4_LTS - 1) / FFA_D4_LTS;
  const int tiles = nt * nt;
  const int img = blockIdx.x / tiles;
  const D4Map m = d4_decode(codes[img] & 15, n, blockIdx.x % tiles, FFA_D4_LTS);
  const long long hw = (long long)n * n;
  for (int e = threadIdx.x; e < FFA_D4_LTS * FFA_D4_LTS; e += FFA_D4_THREADS) {
    const int r = e / FFA_D4_LTS, q = e % FFA_D4_LTS;
    if (r >= m.srows || q >= m.scols) continue;
    const float* px = onehot + (long long)img * K * hw + (long long)(m.si0 + r) * n + m.sj0 + q;
    float best = -INFINITY;
    int am = 0;
    for (int k = 0; k < K; ++k) {
      const float v = px[k * hw];
      if (v > best) {
        best = v;
        am = k;
      }
    }
    tile[r * FFA_D4_LPITCH + q] = (uint8_t)am;
  }
  __syncthreads();
  d4_store_label_tile(m, tile, idx + img * hw, n);
}

static int d4_label_blocks(int B, int n, unsigned* blocks) {
  const int nt = (n + FFA_D4_LTS - 1) / FFA_D4_LTS;
  const long long b = (long long)B * nt * nt;
  FFA_REQUIRE(b <= 0x7fffffffLL, "d4 labels: too many tiles");
  *blocks = (unsigned)b;
  return 0;
}

extern "C" int ffa_d4_labels_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const uint8_t* codes,
                                hipStream_t stream) {
  FFA_REQUIRE(src && dst && codes && B >= 1, "d4_labels_u8: bad arguments");
  FFA_REQUIRE(H == W && H >= 1, "d4_labels_u8: planes must be square, got %d x %d", H, W);
  unsigned blocks;
  if (int rc = d4_label_blocks(B, H, &blocks)) return rc;
  hipLaunchKernelGGL(d4_labels_u8_kernel, dim3(blocks), dim3(FFA_D4_THREADS), 0, stream, src, dst, H, codes);
  return ffa_check_launch("d4_labels_u8");
}

extern "C" int ffa_d4_onehot_to_index(const float* onehot, uint8_t* idx, int B, int K, int H, int W,
                                      const uint8_t* codes, hipStream_t stream) {
  FFA_REQUIRE(onehot && idx && codes && B >= 1 && K >= 1 && K <= 255, "d4_onehot_to_index: bad arguments");
  FFA_REQUIRE(H == W && H >= 1, "d4_onehot_to_index: planes must be square, got %d x %d", H, W);
  unsigned blocks;
  if (int rc = d4_label_blocks(B, H, &blocks)) return rc;
  hipLaunchKernelGGL(d4_onehot_to_index_kernel, dim3(blocks), dim3(FFA_D4_THREADS), 0, stream, onehot, idx, K, H,
                     codes);
  return ffa_check_launch("d4_onehot_to_index");
}
