// Change codes: two uint8 class rasters on one grid -> one uint8 raster of codes through a table,
// out[i] = lut[min(before[i], K) * (K + 1) + min(after[i], K)].  include/flairhip_change.h holds the normative
// definition.  An HBM streaming pass: two bytes read and one written per pixel.
//
// The table ((K + 1)^2 <= 1089 bytes) is staged once per block in LDS.  A lane takes 16 bytes of each input per trip
// (one 16-byte load each, any alignment: the callers hand views in), looks the 16 codes up and stores 16 bytes; the last
// n % 16 bytes go byte by byte in block 0.  A lane reads its bytes of both inputs before it writes the same bytes of out,
// and no other lane touches them, so out may be one of the inputs; the pointers carry no __restrict__ for that reason.
#include "ffa_common.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxK = FFA_CHANGE_MAX_CLASSES;
constexpr int kTab = (kMaxK + 1) * (kMaxK + 1);

__device__ __forceinline__ unsigned int code_of(const uint8_t* s_lut, unsigned int a, unsigned int b, int K) {
  const int x = min((int)a, K), y = min((int)b, K);
  return s_lut[x * (K + 1) + y];
}

__global__ __launch_bounds__(kT) void change_code_kernel(const uint8_t* before, const uint8_t* after, long long n, int K,
                                                         const uint8_t* lut, uint8_t* out) {
  __shared__ uint8_t s_lut[kTab];
  const int tab = (K + 1) * (K + 1);  // <= kTab: the entry point checked K
  for (int i = threadIdx.x; i < tab; i += kT) s_lut[i] = lut[i];
  __syncthreads();
  const long long groups = n >> 4;
  const long long stride = (long long)gridDim.x * kT;
  for (long long g = (long long)blockIdx.x * kT + threadIdx.x; g < groups; g += stride) {
    uint4 a, b;
    __builtin_memcpy(&a, before + 16 * g, 16);
    __builtin_memcpy(&b, after + 16 * g, 16);
    const unsigned int av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    unsigned int ov[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned int w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        w |= code_of(s_lut, (av[d] >> (8 * j)) & 255u, (bv[d] >> (8 * j)) & 255u, K) << (8 * j);
      ov[d] = w;
    }
    const uint4 o = make_uint4(ov[0], ov[1], ov[2], ov[3]);
    __builtin_memcpy(out + 16 * g, &o, 16);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 15)) {  // the tail
    const long long i = 16 * groups + threadIdx.x;
    const unsigned int a = before[i], b = after[i];
    out[i] = (uint8_t)code_of(s_lut, a, b, K);
  }
}

}  // namespace

extern "C" int ffa_change_code_u8(const uint8_t* before, const uint8_t* after, long long n, int K, const uint8_t* lut,
                                  uint8_t* out, hipStream_t st) {
  FFA_REQUIRE(K >= 1 && K <= kMaxK, "change_code: %d classes outside 1..%d", K, kMaxK);
  FFA_REQUIRE(n >= 0, "change_code: %lld bytes", n);
  if (n == 0) return FFA_OK;
  FFA_REQUIRE(before && after && lut && out, "change_code: null raster, table or output");
  const long long blocks = ((n >> 4) + kT - 1) / kT;
  // 8 blocks per CU walk the raster with a grid stride; one block at least, for the tail
  const dim3 grid((unsigned int)(blocks < 1 ? 1 : (blocks < 2048 ? blocks : 2048)));
  hipLaunchKernelGGL(change_code_kernel, grid, dim3(kT), 0, st, before, after, n, K, lut, out);
  return ffa_check_launch("change_code");
}
