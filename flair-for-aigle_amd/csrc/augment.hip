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
#include "ffa_d4.h"

// grid: B * tiles blocks, one tile of one image each: d4_layout_image (ffa_d4.h) on image img under its code
template <typename S, typename T>
__global__ void __launch_bounds__(FFA_D4_THREADS)
d4_nchw_to_nhwc_kernel(const S* __restrict__ src, T* __restrict__ dst, int C, int n, int Cp,
                       const float* __restrict__ mean, const float* __restrict__ stdv,
                       const uint8_t* __restrict__ codes, int group, int vec4) {
  const int nt = (n + FFA_D4_TS - 1) / FFA_D4_TS;
  const int tiles = nt * nt;
  const int img = blockIdx.x / tiles;
  const D4Map m = d4_decode(codes[img / group] & 15, n, blockIdx.x % tiles, FFA_D4_TS);
  const long long hw = (long long)n * n;
  d4_layout_image<S, T>(m, src + (long long)img * C * hw, dst + (long long)img * hw * Cp, C, n, hw, Cp, mean, stdv, vec4,
                        FFA_ELEV_NONE);
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
