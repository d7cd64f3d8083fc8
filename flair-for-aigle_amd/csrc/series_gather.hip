// The padded batch of a U-TAE branch gathered from a ragged, device-resident series store: data [D, C, H, W] holds the
// dates of all N samples back to back (uint8 / uint16 / int16 / float32, as the dataset yields them before the f32
// cast), offsets [N + 1] says where each sample's dates start, is_pad [D] which stored dates are constant at the model's
// pad value.  Image b * T + t of the NHWC output is date t of sample index[b], read through the D4 gather of codes[b];
// the dates past the sample's length are the constant `fill` pad_collate_flair pads with.  pad [B * T] is what
// detect_pad_images reports on the padded f32 batch.  No normalisation: the reference normalises no series.
//
// Kernel shape: sample_gather.hip's.  A block works on one pixel tile of one output image, so index[b], its offset, its
// length and its code are read once and stay wave-uniform, and whether the block copies a stored date or writes a padded
// one is a block-uniform branch.  A stored date goes through d4_layout_image (ffa_d4.h), the one definition of the
// layout pass, so the result equals d4_nchw_to_nhwc_kernel's on the padded batch by construction; a padded date is
// written with the same 16-byte pieces in memory order.  An index outside [0, N) is the caller's error and is clamped;
// a series longer than T loses its dates beyond T; nothing outside the store or the outputs is read or written.
#include "ffa_d4.h"

// grid: B * T * tiles blocks
template <typename S, typename T>
__global__ void __launch_bounds__(FFA_D4_THREADS)
gather_series_kernel(const S* __restrict__ data, const int* __restrict__ offsets, const uint8_t* __restrict__ is_pad,
                     const int* __restrict__ index, T* __restrict__ dst, uint8_t* __restrict__ pad, int N, int Tn,
                     int C, int H, int W, int Cp, float fill, int tail_is_pad, const uint8_t* __restrict__ codes,
                     int vec4) {
  const int tiles = ((H + FFA_D4_TS - 1) / FFA_D4_TS) * ((W + FFA_D4_TS - 1) / FFA_D4_TS);
  const int img = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int b = img / Tn, t = img % Tn;
  const D4Map m = codes ? d4_decode(codes[b] & 15, H, tile, FFA_D4_TS) : d4_identity(H, W, tile, FFA_D4_TS);
  const int sample = min(max(index[b], 0), N - 1);
  const int first = offsets[sample];
  const int len = offsets[sample + 1] - first;
  const long long hw = (long long)H * W;
  T* dimg = dst + (long long)img * hw * Cp;
  if (t < len) {  // block-uniform
    const long long date = (long long)first + t;
    if (tile == 0 && threadIdx.x == 0) pad[img] = is_pad[date];
    d4_layout_image<S, T>(m, data + date * C * hw, dimg, C, W, hw, Cp, nullptr, nullptr, vec4, FFA_ELEV_NONE);
    return;
  }
  if (tile == 0 && threadIdx.x == 0) pad[img] = (uint8_t)(tail_is_pad ? 1 : 0);
  const int groups = Cp / 8;
  for (int e = threadIdx.x; e < FFA_D4_TS * FFA_D4_TS * groups; e += FFA_D4_THREADS) {
    const int pix = e / groups;
    const int g = e - pix * groups;
    const int li = pix / FFA_D4_TS, lj = pix % FFA_D4_TS;
    if (li >= m.th || lj >= m.tw) continue;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = g * 8 + k < C ? fill : 0.f;
    ffa_store8<T>(dimg + ((long long)(m.i0 + li) * W + m.j0 + lj) * Cp + g * 8, v);
  }
}

template <typename S>
static int gather_series_launch(int dtype, const void* data, const int* offsets, const uint8_t* is_pad,
                                const int* index, void* dst, uint8_t* pad, int N, int B, int T, int C, int H, int W,
                                int Cp, float fill, int tail_is_pad, const uint8_t* codes, hipStream_t stream) {
  const long long blocks =
      (long long)B * T * ((H + FFA_D4_TS - 1) / FFA_D4_TS) * ((W + FFA_D4_TS - 1) / FFA_D4_TS);
  FFA_REQUIRE(blocks <= 0x7fffffffLL, "gather_series: too many tiles");
  // every plane of the store starts on a 4-sample boundary when the store does and W % 4 == 0
  const int vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(data) % (4 * sizeof(S)) == 0);
  const size_t lds = (size_t)(C < 8 ? C : 8) * FFA_D4_TS * FFA_D4_PITCH * sizeof(float);
  if (dtype == FFA_BF16)
    hipLaunchKernelGGL((gather_series_kernel<S, ffa_bf16>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)data, offsets, is_pad, index, (ffa_bf16*)dst, pad, N, T, C, H, W, Cp, fill,
                       tail_is_pad, codes, vec4);
  else
    hipLaunchKernelGGL((gather_series_kernel<S, float>), dim3((unsigned)blocks), dim3(FFA_D4_THREADS), lds, stream,
                       (const S*)data, offsets, is_pad, index, (float*)dst, pad, N, T, C, H, W, Cp, fill, tail_is_pad,
                       codes, vec4);
  return ffa_check_launch("gather_series");
}

extern "C" int ffa_gather_series(int dtype, int src_kind, const void* data, const int* offsets, const uint8_t* is_pad,
                                 const int* index, void* dst, uint8_t* pad, int N, int B, int T, int C, int H, int W,
                                 int Cp, float fill, int tail_is_pad, const uint8_t* codes, hipStream_t stream) {
  FFA_REQUIRE(data && offsets && is_pad && index && dst && pad, "gather_series: null pointer");
  FFA_REQUIRE(N >= 1 && B >= 1 && T >= 1 && C >= 1 && H >= 1 && W >= 1,
              "gather_series: bad arguments (N=%d B=%d T=%d C=%d H=%d W=%d)", N, B, T, C, H, W);
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "gather_series: unknown output type %d", dtype);
  FFA_REQUIRE(Cp % 8 == 0 && Cp >= C, "gather_series: bad channel pitch (C=%d Cp=%d)", C, Cp);
  FFA_REQUIRE(!codes || H == W, "gather_series: rotations need square planes, got %d x %d", H, W);
  switch (src_kind) {
    case FFA_SRC_U8:
      return gather_series_launch<uint8_t>(dtype, data, offsets, is_pad, index, dst, pad, N, B, T, C, H, W, Cp, fill,
                                           tail_is_pad, codes, stream);
    case FFA_SRC_U16:
      return gather_series_launch<uint16_t>(dtype, data, offsets, is_pad, index, dst, pad, N, B, T, C, H, W, Cp, fill,
                                            tail_is_pad, codes, stream);
    case FFA_SRC_I16:
      return gather_series_launch<int16_t>(dtype, data, offsets, is_pad, index, dst, pad, N, B, T, C, H, W, Cp, fill,
                                           tail_is_pad, codes, stream);
    case FFA_SRC_F32:
      return gather_series_launch<float>(dtype, data, offsets, is_pad, index, dst, pad, N, B, T, C, H, W, Cp, fill,
                                         tail_is_pad, codes, stream);
  }
  ffa_set_error("gather_series: unknown source sample kind %d", src_kind);
  return FFA_ERR_ARG;
}
