// Overview pyramid of a uint8 raster (the reduced-resolution images of a cloud-optimised GeoTIFF): every level halves
// the one before, by nearest / mode / average over 2 x 2 blocks.  include/flairhip.h holds the normative definition.
//
// overview_kernel<method>: one block per 64-row x 256-column tile of the source level and per band; one launch writes
// up to four levels from one read of the source.
//   1. load     the tile goes to LDS in 16-byte pieces, lane i on piece i of a row (a wave covers four full rows).
//               Rows of a raster whose width is no multiple of 16 start at any byte: the piece is then cut out of the
//               two aligned 16-byte loads that cover it.  Pieces those loads would take outside the raster (its first
//               and last bytes) and pieces past the row end are read byte by byte.
//   2. reduce   128 x 32 from the tile (16 pixels per thread, 16-byte LDS reads), then 64 x 16, 32 x 8 and 16 x 4 from
//               the level before, all in LDS.  A block on the raster's last row or column reads its missing pixels
//               from the row / column before (clamped indices): every count of the vote doubles and so does the sum and
//               the divisor of the mean, which gives the definition's n = 1 and n = 2 results.
//   3. store    every level's part of the tile: 16-byte stores on the aligned groups of each destination row (cut out
//               of LDS dwords, since the row's first pixel is rarely on a 16-byte address), single bytes at its ends.
// Tile origins are multiples of 64 rows and 256 columns, so the 2 x 2 blocks of all four levels lie inside one tile and
// the bytes equal those of a level-by-level chain.  Levels beyond four come from further launches on the last level.
#include "ffa_common.h"

namespace {

constexpr int kT = 256;
constexpr int kTileH = 64, kTileW = 256;
constexpr int kMaxFused = 4;
// byte offsets of the tile and of levels 1..4 in the LDS image; 32 spare bytes: the store pass reads 5 dwords a group
constexpr int kOff0 = 0, kOff1 = kTileH * kTileW, kOff2 = kOff1 + 32 * 128, kOff3 = kOff2 + 16 * 64,
              kOff4 = kOff3 + 8 * 32, kLdsBytes = kOff4 + 4 * 16 + 32;

struct Level {
  uint8_t* ptr;  // [bands][H][W]
  int H, W;
};

struct Args {
  const uint8_t* src;  // [bands][H][W]
  int H, W, bands, n;  // n = levels this launch writes, 1..4
  int tiles_x, tiles_y;
  int ignore;
  Level out[kMaxFused];
};

template <int M>
__device__ __forceinline__ unsigned int combine(unsigned int a, unsigned int b, unsigned int c, unsigned int d,
                                                int ignore) {
  if (M == 0) return a;
  if (M == 2) return (a + b + c + d + 2u) >> 2;
  // mode: most votes, then the smaller value; key = votes * 256 + (255 - value), -1 while nothing has voted
  const unsigned int v[4] = {a, b, c, d};
  int best = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += v[j] == v[i];
    const int key = (int)v[i] == ignore ? -1 : cnt * 256 + 255 - (int)v[i];
    best = key > best ? key : best;
  }
  return best < 0 ? (unsigned int)ignore : 255u - ((unsigned int)best & 255u);
}

__device__ __forceinline__ unsigned int funnel(unsigned int lo, unsigned int hi, int byte_shift) {
  return (unsigned int)((((unsigned long long)hi << 32) | lo) >> (8 * byte_shift));
}

// 16 bytes starting `d` dwords and `sh` bytes into w[0..7]
__device__ __forceinline__ uint4 cut16(const unsigned int (&w)[8], int d, int sh) {
  unsigned int x[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) x[m] = d == 0 ? w[m] : d == 1 ? w[m + 1] : d == 2 ? w[m + 2] : w[m + 3];
  return make_uint4(funnel(x[0], x[1], sh), funnel(x[1], x[2], sh), funnel(x[2], x[3], sh), funnel(x[3], x[4], sh));
}

// one pixel of a level from the LDS image of the level before (pitch pw, valid extent ph x pw_valid)
template <int M>
__device__ __forceinline__ uint8_t reduce_px(const uint8_t* prev, int pitch, int ph, int pwv, int r, int c, int ignore) {
  const int r0 = 2 * r, r1 = min(2 * r + 1, ph - 1), c0 = 2 * c, c1 = min(2 * c + 1, pwv - 1);
  return (uint8_t)combine<M>(prev[r0 * pitch + c0], prev[r0 * pitch + c1], prev[r1 * pitch + c0], prev[r1 * pitch + c1],
                             ignore);
}

template <int M>
__global__ __launch_bounds__(kT) void overview_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) unsigned int s_words[kLdsBytes / 4];
  uint8_t* const lds = reinterpret_cast<uint8_t*>(s_words);
  const int tid = threadIdx.x;
  long long blk = blockIdx.x;
  const int tx = (int)(blk % a.tiles_x);
  blk /= a.tiles_x;
  const int ty = (int)(blk % a.tiles_y);
  const int band = (int)(blk / a.tiles_y);
  const int r0 = ty * kTileH, c0 = tx * kTileW;
  const int hv0 = min(kTileH, a.H - r0), wv0 = min(kTileW, a.W - c0);  // >= 1: the grid covers the raster only

  // ---- 1. load: thread = piece k of the rows r, r + 16, r + 32, r + 48; every load is issued before the first use ----
  {
    const uintptr_t t0 = (uintptr_t)a.src, t1 = t0 + (uintptr_t)((long long)a.bands * a.H * a.W);
    const uint8_t* plane = a.src + (long long)band * a.H * a.W;
    const int k = tid & 15, rbase = tid >> 4;
    const bool piece = 16 * k < wv0;  // else nothing of this piece is ever read
    // every row of the tile starts on a 16-byte address and this piece lies inside the row: one load per piece
    const bool aligned = (((uintptr_t)plane + (uintptr_t)c0) & 15) == 0 && (a.W & 15) == 0 && 16 * k + 16 <= wv0;
    const uint8_t* g[4];
    uint4 lo[4], hi[4];
    int mode[4];  // 0: skip, 1: one aligned load, 2: cut out of two aligned loads, 3: byte by byte
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rbase + 16 * j;
      g[j] = plane + (long long)(r0 + row) * a.W + c0 + 16 * k;
      const uint8_t* q = g[j] - ((uintptr_t)g[j] & 15);  // the aligned 16 bytes that hold the piece's first byte
      const uintptr_t p0 = (uintptr_t)q;
      // both aligned loads must lie inside the raster; bytes past the row end belong to the next row and are not used
      mode[j] = !(piece && row < hv0) ? 0 : aligned ? 1 : (p0 >= t0 && p0 + 32 <= t1) ? 2 : 3;
      if (mode[j] == 1 || mode[j] == 2) lo[j] = *reinterpret_cast<const uint4*>(q);
      if (mode[j] == 2) hi[j] = *reinterpret_cast<const uint4*>(q + 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mode[j] == 0) continue;
      uint4 v;
      if (mode[j] == 1) {
        v = lo[j];
      } else if (mode[j] == 2) {
        const int head = (int)((uintptr_t)g[j] & 15);
        const unsigned int w[8] = {lo[j].x, lo[j].y, lo[j].z, lo[j].w, hi[j].x, hi[j].y, hi[j].z, hi[j].w};
        v = cut16(w, head >> 2, head & 3);
      } else {
        union { uint4 q; uint8_t b[16]; } u;
        u.q = make_uint4(0, 0, 0, 0);
        for (int i = 0; i < 16; ++i)
          if (16 * k + i < wv0) u.b[i] = g[j][i];
        v = u.q;
      }
      *reinterpret_cast<uint4*>(lds + kOff0 + (rbase + 16 * j) * kTileW + 16 * k) = v;
    }
  }
  __syncthreads();

  // ---- 2. reduce ----
  const int hv1 = (hv0 + 1) >> 1, wv1 = (wv0 + 1) >> 1;
  {  // level 1: thread = one row, 16 columns
    const int r = tid >> 3, cb = (tid & 7) * 16;
    if (r < hv1 && cb < wv1) {
      const int ra = 2 * r, rb = min(2 * r + 1, hv0 - 1);
      union { uint4 q[2]; uint8_t b[32]; } top, bot;
      union { uint4 q; uint8_t b[16]; } o;
      const uint4* pa = reinterpret_cast<const uint4*>(lds + kOff0 + ra * kTileW + 2 * cb);
      const uint4* pb = reinterpret_cast<const uint4*>(lds + kOff0 + rb * kTileW + 2 * cb);
      top.q[0] = pa[0];
      top.q[1] = pa[1];
      bot.q[0] = pb[0];
      bot.q[1] = pb[1];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool right = 2 * (cb + i) + 1 < wv0;
        const unsigned int p = top.b[2 * i], q = bot.b[2 * i];
        o.b[i] = (uint8_t)combine<M>(p, right ? top.b[2 * i + 1] : p, q, right ? bot.b[2 * i + 1] : q, a.ignore);
      }
      *reinterpret_cast<uint4*>(lds + kOff1 + r * 128 + cb) = o.q;
    }
  }
  __syncthreads();
  const int hv2 = (hv1 + 1) >> 1, wv2 = (wv1 + 1) >> 1;
  if (a.n >= 2) {  // 16 x 64, 4 pixels per thread
    const int r = tid >> 4, cb = (tid & 15) * 4;
    if (r < hv2)
      for (int c = cb; c < min(cb + 4, wv2); ++c)
        lds[kOff2 + r * 64 + c] = reduce_px<M>(lds + kOff1, 128, hv1, wv1, r, c, a.ignore);
  }
  __syncthreads();
  const int hv3 = (hv2 + 1) >> 1, wv3 = (wv2 + 1) >> 1;
  if (a.n >= 3) {  // 8 x 32
    const int r = tid >> 5, c = tid & 31;
    if (r < hv3 && c < wv3) lds[kOff3 + r * 32 + c] = reduce_px<M>(lds + kOff2, 64, hv2, wv2, r, c, a.ignore);
  }
  __syncthreads();
  const int hv4 = (hv3 + 1) >> 1, wv4 = (wv3 + 1) >> 1;
  if (a.n >= 4 && tid < 64) {  // 4 x 16
    const int r = tid >> 4, c = tid & 15;
    if (r < hv4 && c < wv4) lds[kOff4 + r * 16 + c] = reduce_px<M>(lds + kOff3, 32, hv3, wv3, r, c, a.ignore);
  }
  __syncthreads();

  // ---- 3. store: items = (level, row, 16-byte group of the destination row) ----
  constexpr int kItems1 = 32 * 9, kItems2 = 16 * 5, kItems3 = 8 * 3, kItems4 = 4 * 2;
  for (int i = tid; i < kItems1 + kItems2 + kItems3 + kItems4; i += kT) {
    int l, j, off, hv, wv;
    if (i < kItems1) {
      l = 1, j = i, off = kOff1, hv = hv1, wv = wv1;
    } else if (i < kItems1 + kItems2) {
      l = 2, j = i - kItems1, off = kOff2, hv = hv2, wv = wv2;
    } else if (i < kItems1 + kItems2 + kItems3) {
      l = 3, j = i - kItems1 - kItems2, off = kOff3, hv = hv3, wv = wv3;
    } else {
      l = 4, j = i - kItems1 - kItems2 - kItems3, off = kOff4, hv = hv4, wv = wv4;
    }
    if (l > a.n) continue;
    const int tw = kTileW >> l, nq = tw / 16 + 1;
    const int r = j / nq, q = j - r * nq;
    if (r >= hv) continue;
    const Level& lv = a.out[l - 1];
    uint8_t* row = lv.ptr + ((long long)band * lv.H + (r0 >> l) + r) * lv.W + (c0 >> l);  // wv valid pixels from here
    const int head = (int)((uintptr_t)row & 15);
    const int o = 16 * q - head;  // tile column of the group's first byte; row + o is 16-byte aligned
    if (o >= wv) continue;
    const int idx = off + r * tw + o;
    if (o >= 0 && o + 16 <= wv) {
      const unsigned int* w = s_words + (idx >> 2);
      const int sh = idx & 3;
      const unsigned int x0 = w[0], x1 = w[1], x2 = w[2], x3 = w[3], x4 = w[4];
      *reinterpret_cast<uint4*>(row + o) =
          make_uint4(funnel(x0, x1, sh), funnel(x1, x2, sh), funnel(x2, x3, sh), funnel(x3, x4, sh));
    } else {
      for (int b = 0; b < 16; ++b)
        if (o + b >= 0 && o + b < wv) row[o + b] = lds[idx + b];
    }
  }
}

inline int half_up(int v, int l) { return (int)(((long long)v + (1ll << l) - 1) >> l); }

bool shape_ok(int bands, int H, int W, int levels) {
  return bands >= 1 && H >= 1 && W >= 1 && levels >= 0 && levels <= 30 && (long long)bands * H * W < (1ll << 31);
}

}  // namespace

extern "C" int ffa_overview_levels(int H, int W, int block) {
  FFA_REQUIRE(H >= 1 && W >= 1 && block >= 1, "overview_levels: raster %d x %d, block %d outside 1 <= H, W, block", H,
              W, block);
  int L = 0;
  while (half_up(H, L) > block || half_up(W, L) > block) ++L;
  return L;
}

extern "C" long long ffa_overview_pyramid_bytes(int bands, int H, int W, int levels) {
  if (!shape_ok(bands, H, W, levels)) {
    ffa_set_error("overview_pyramid_bytes: %d bands of %d x %d, %d levels outside 1 <= bands, H, W, bands * H * W < "
                  "2^31 and 0 <= levels <= 30", bands, H, W, levels);
    return FFA_ERR_ARG;
  }
  long long total = 0;
  for (int l = 1; l <= levels; ++l) total += (long long)bands * half_up(H, l) * half_up(W, l);
  return total;
}

extern "C" int ffa_overview_pyramid_u8(const uint8_t* base, uint8_t* pyr, int bands, int H, int W, int levels,
                                       int method, int ignore, hipStream_t st) {
  FFA_REQUIRE(shape_ok(bands, H, W, levels),
              "overview_pyramid: %d bands of %d x %d, %d levels outside 1 <= bands, H, W, bands * H * W < 2^31 and "
              "0 <= levels <= 30", bands, H, W, levels);
  FFA_REQUIRE(method >= 0 && method <= 2, "overview_pyramid: method %d is not 0 (nearest), 1 (mode) or 2 (average)",
              method);
  FFA_REQUIRE(ignore >= -1 && ignore <= 255, "overview_pyramid: ignore %d is neither -1 nor a uint8 value", ignore);
  FFA_REQUIRE(method != 2 || ignore == -1, "overview_pyramid: the average has no ignore value (got %d)", ignore);
  if (levels == 0) return FFA_OK;
  FFA_REQUIRE(base && pyr, "overview_pyramid: null pointer");
  const uint8_t* src = base;
  int sh = H, sw = W;
  uint8_t* next = pyr;
  for (int done = 0; done < levels;) {
    Args a = {};
    a.src = src;
    a.H = sh;
    a.W = sw;
    a.bands = bands;
    a.n = levels - done < kMaxFused ? levels - done : kMaxFused;
    a.tiles_x = ffa_cdiv(sw, kTileW);
    a.tiles_y = ffa_cdiv(sh, kTileH);
    a.ignore = method == 1 ? ignore : -1;
    for (int k = 0; k < a.n; ++k) {
      a.out[k].ptr = next;
      a.out[k].H = half_up(H, done + k + 1);
      a.out[k].W = half_up(W, done + k + 1);
      next += (long long)bands * a.out[k].H * a.out[k].W;
    }
    const dim3 grid((unsigned int)((long long)a.tiles_x * a.tiles_y * bands));  // < 2^31 / (64 * 256) + edge tiles
    if (method == 0)
      hipLaunchKernelGGL(overview_kernel<0>, grid, dim3(kT), 0, st, a);
    else if (method == 1)
      hipLaunchKernelGGL(overview_kernel<1>, grid, dim3(kT), 0, st, a);
    else
      hipLaunchKernelGGL(overview_kernel<2>, grid, dim3(kT), 0, st, a);
    src = a.out[a.n - 1].ptr;
    sh = a.out[a.n - 1].H;
    sw = a.out[a.n - 1].W;
    done += a.n;
  }
  return ffa_check_launch("overview_pyramid");
}
