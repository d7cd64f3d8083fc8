// A batch gathered from a device-resident sample store: image b of the output is image index[b] of a raw NCHW store
// [N, C_src, H, W] (uint8 / uint16 / int16 / float32, as decoded from the patch rasters), read through the D4 gather
// of augment.hip's layout kernel and normalised on the way, and label map b is label map index[b] of a uint8 store
// [N, H, W] reduced to class indices by the reference's rule.  index is int32 on the device, so a captured training
// step replays with new indices as it replays with new augmentation codes.
//
// The elevation pre-processing of the reference happens in the same pass (a 2-band DEM_ELEV patch: band 0 surface
// model, band 1 terrain model): FFA_ELEV_DIFF writes the one channel z0 - z1 (calc_elevation, elevation.py:11),
// FFA_ELEV_STACK the two channels (z0, z0 - z1) (calc_elevation_stack_dsm, dataloader.py:140-141); the difference is
// taken in f32 before the normalisation, and mean / stdv are indexed by output channel.
//
// Kernel shape: augment.hip's.  A block works on one pixel tile of one output image, so index[b], the code and all
// that follows from them are wave-uniform; the source tile is read row by row, coalesced, into LDS; the destination
// pixels are written in memory order with 16-byte stores.  An index outside [0, N) is the caller's error: the kernels
// clamp it, so nothing outside the store is ever read.
#include "ffa_d4.h"

// grid: B * tiles blocks; d4_nchw_to_nhwc_kernel's pass (d4_layout_image, ffa_d4.h) with the image taken from the store
// and C output channels made of C_src stored ones.  codes null: the identity on an H x W plane; otherwise H == W.
template <typename S, typename T>
__global__ void __launch_bounds__(FFA_D4_THREADS)
gather_layout_kernel(const S* __restrict__ store, const int* __restrict__ index, T* __restrict__ dst, int N, int C_src,
                     int C, int H, int W, int Cp, const float* __restrict__ mean, const float* __restrict__ stdv,
                     const uint8_t* __restrict__ codes, int group, int elev, int vec4) {
  const int tiles = ((H + FFA_D4_TS - 1) / FFA_D4_TS) * ((W + FFA_D4_TS - 1) / FFA_D4_TS);
  const int img = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const D4Map m = codes ? d4_decode(codes[img / group] & 15, H, tile, FFA_D4_TS) : d4_identity(H, W, tile, FFA_D4_TS);
  const int sample = min(max(index[img], 0), N - 1);
  const long long hw = (long long)H * W;
  d4_layout_image<S, T>(m, store + (long long)sample * C_src * hw, dst + (long long)img * hw * Cp, C, W, hw, Cp, mean,
                        stdv, vec4, elev);
}

template <typename S>
static int gather_layout_launch(int dtype, const void* store, const int* index, void* dst, int N, int B, int C_src,
                                int C, int H, int W, int Cp, const float* mean, const float* stdv,
                                const uint8_t* codes, int group, int elev, hipStream_t stream) {
  const long long blocks =
      (long long)B * ((H + FFA_D4_TS - 1) / FFA_D4_TS) * ((W + FFA_D4_TS - 1) / FFA_D4_TS);
  FFA_REQUIRE(blocks <= 0x7fffffffLL, "gather_layout: too many tiles");
  // every plane of the store starts on a 4-sample boundary when the store does and W % 4 == 0
  const int vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(store) % (4 * sizeof(S)) == 0);
  const size_t lds = (size_t)(C < 8 ? C : 8) * FFA_D4_TS * FFA_D4_PITCH * sizeof(float);
  if (dtype == FFA_BF16)
    hipLaunchKernelGGL((gather_layout_kernel<S, ffa_bf16>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)store, index, (ffa_bf16*)dst, N, C_src, C, H, W, Cp, mean, stdv, codes, group, elev,
                       vec4);
  else
    hipLaunchKernelGGL((gather_layout_kernel<S, float>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)store, index, (float*)dst, N, C_src, C, H, W, Cp, mean, stdv, codes, group, elev,
                       vec4);
  return ffa_check_launch("gather_layout");
}

extern "C" int ffa_gather_layout(int dtype, int src_kind, const void* store, const int* index, void* dst, int N, int B,
                                 int C_src, int H, int W, int Cp, const float* mean, const float* stdv,
                                 const uint8_t* codes, int group, int elevation, hipStream_t stream) {
  FFA_REQUIRE(store && index && dst && N >= 1 && B >= 1 && C_src >= 1 && H >= 1 && W >= 1,
              "gather_layout: bad arguments (N=%d B=%d C_src=%d H=%d W=%d)", N, B, C_src, H, W);
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "gather_layout: unknown output type %d", dtype);
  FFA_REQUIRE(elevation == FFA_ELEV_NONE || elevation == FFA_ELEV_DIFF || elevation == FFA_ELEV_STACK,
              "gather_layout: unknown elevation mode %d", elevation);
  FFA_REQUIRE(elevation == FFA_ELEV_NONE || C_src == 2, "gather_layout: the elevation modes need the 2 bands, got %d",
              C_src);
  const int C = elevation == FFA_ELEV_NONE ? C_src : elevation == FFA_ELEV_DIFF ? 1 : 2;
  FFA_REQUIRE(Cp % 8 == 0 && Cp >= C, "gather_layout: bad channel pitch (C=%d Cp=%d)", C, Cp);
  FFA_REQUIRE(!codes || H == W, "gather_layout: rotations need square planes, got %d x %d", H, W);
  FFA_REQUIRE((mean == nullptr) == (stdv == nullptr), "gather_layout: mean and std come together or not at all");
  FFA_REQUIRE(mean || src_kind == FFA_SRC_F32, "gather_layout: integer samples need mean / std");
  FFA_REQUIRE(group >= 1 && B % group == 0, "gather_layout: %d images do not split into groups of %d", B, group);
  switch (src_kind) {
    case FFA_SRC_U8:
      return gather_layout_launch<uint8_t>(dtype, store, index, dst, N, B, C_src, C, H, W, Cp, mean, stdv, codes, group,
                                           elevation, stream);
    case FFA_SRC_U16:
      return gather_layout_launch<uint16_t>(dtype, store, index, dst, N, B, C_src, C, H, W, Cp, mean, stdv, codes,
                                            group, elevation, stream);
    case FFA_SRC_I16:
      return gather_layout_launch<int16_t>(dtype, store, index, dst, N, B, C_src, C, H, W, Cp, mean, stdv, codes, group,
                                           elevation, stream);
    case FFA_SRC_F32:
      return gather_layout_launch<float>(dtype, store, index, dst, N, B, C_src, C, H, W, Cp, mean, stdv, codes, group,
                                         elevation, stream);
  }
  ffa_set_error("gather_layout: unknown source sample kind %d", src_kind);
  return FFA_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------
// labels: the raw label channel -> class indices.  The reference one-hot encodes the raster against range(K)
// (reshape_label_ohe, label.py:12-14) and takes the argmax (tasks_module.py:153): a value v < K stays v, and a value
// v >= K has an all-false one-hot whose argmax is 0 -- it becomes class 0, not an ignored pixel.

__global__ void __launch_bounds__(FFA_D4_THREADS)
gather_labels_u8_kernel(const uint8_t* __restrict__ store, const int* __restrict__ index, uint8_t* __restrict__ dst,
                        int N, int H, int W, int K, const uint8_t* __restrict__ codes) {
  __shared__ __align__(16) uint8_t tile[FFA_D4_LTS * FFA_D4_LPITCH];
  const int tiles = ((H + FFA_D4_LTS - 1) / FFA_D4_LTS) * ((W + FFA_D4_LTS - 1) / FFA_D4_LTS);
  const int img = blockIdx.x / tiles;
  const int t = blockIdx.x % tiles;
  const D4Map m = codes ? d4_decode(codes[img] & 15, H, t, FFA_D4_LTS) : d4_identity(H, W, t, FFA_D4_LTS);
  const int sample = min(max(index[img], 0), N - 1);
  const long long hw = (long long)H * W;
  const uint8_t* plane = store + sample * hw;
  for (int e = threadIdx.x; e < FFA_D4_LTS * FFA_D4_LTS; e += FFA_D4_THREADS) {
    const int r = e / FFA_D4_LTS, q = e % FFA_D4_LTS;
    if (r < m.srows && q < m.scols) {
      const int v = plane[(long long)(m.si0 + r) * W + m.sj0 + q];
      tile[r * FFA_D4_LPITCH + q] = (uint8_t)(v < K ? v : 0);
    }
  }
  __syncthreads();
  d4_store_label_tile(m, tile, dst + img * hw, W);
}

extern "C" int ffa_gather_labels_u8(const uint8_t* store, const int* index, uint8_t* dst, int N, int B, int H, int W,
                                    int num_classes, const uint8_t* codes, hipStream_t stream) {
  FFA_REQUIRE(store && index && dst && N >= 1 && B >= 1 && H >= 1 && W >= 1,
              "gather_labels_u8: bad arguments (N=%d B=%d H=%d W=%d)", N, B, H, W);
  FFA_REQUIRE(num_classes >= 1 && num_classes <= 256, "gather_labels_u8: %d classes do not fit a byte", num_classes);
  FFA_REQUIRE(!codes || H == W, "gather_labels_u8: rotations need square planes, got %d x %d", H, W);
  const long long blocks =
      (long long)B * ((H + FFA_D4_LTS - 1) / FFA_D4_LTS) * ((W + FFA_D4_LTS - 1) / FFA_D4_LTS);
  FFA_REQUIRE(blocks <= 0x7fffffffLL, "gather_labels_u8: too many tiles");
  hipLaunchKernelGGL(gather_labels_u8_kernel, dim3((unsigned)blocks), dim3(FFA_D4_THREADS), 0, stream, store, index,
                     dst, N, H, W, num_classes, codes);
  return ffa_check_launch("gather_labels_u8");
}
