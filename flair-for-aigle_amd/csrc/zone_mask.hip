// Geozone clipping on the pixel grid: rasterise polygon rings into a uint8 inside mask, clip / class-filter a class
// raster with it, count mask pixels in rectangles (tile skipping).  include/flairhip.h holds the normative definition.
//
// ffa_zone_mask_u8 (separate launches, no grid-wide barrier):
//   1. spans    zone_span_kernel: one block walks the edges (vertex v -> next vertex of its ring, the last one back to
//               the first) and writes, per edge, the first pixel row its y range can cross, a conservative row count
//               and the exclusive scan of those counts.  The scan balances the next pass: a contour of 50 000 short
//               edges and a box of 4 long ones both become a flat list of (edge, row) items.
//   2. toggles  zone_toggle_kernel: one work item per (edge, row); the exact crossing predicate and the crossing column
//               in separately rounded float64 (contraction is off for this file), then one atomicXor of one bit in the
//               bit-packed plane uint32 [H][ceil(W / 32)].  XOR commutes: the plane does not depend on the schedule.
//   3. row scan zone_row_scan_kernel: a wave per row; prefix XOR inside each word by shift-XOR steps, carry across
//               words = parity of the popcounts before (ballot), running carry when a row has more than 64 words.
//               In place: the plane then holds inside bits.
//   4. expand   zone_expand_kernel: 16 mask bytes per lane from 16 plane bits, 16-byte stores aligned on the mask
//               pointer; with accumulate the bytes are ORed into the mask.
// The plane is cleared at the head of every call (hipMemsetAsync), so the workspace may hold anything.
#include "ffa_common.h"
#include "ffa_zone.h"  // the crossing predicate and column, shared with zone_stats.hip

// xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) must round every operation separately: no a * b + c -> fma
#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kScanT = 1024;
constexpr long long kAlign = 256;

inline long long align_up(long long v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Layout {
  long long tog, offs, rfirst, nxt, total;
  int WW;
};

Layout make_layout(int H, int W, long long n) {
  Layout lo;
  lo.WW = (W + 31) / 32;
  lo.tog = 0;
  lo.offs = align_up(4ll * H * lo.WW);  // int64 [n + 1], then the two int32 [n] arrays: 16 n + 8 bytes
  lo.rfirst = lo.offs + 8 * (n + 1);
  lo.nxt = lo.rfirst + 4 * n;
  lo.total = lo.nxt + 4 * n;
  return lo;
}

template <typename T>
__host__ __device__ inline T* at(void* ws, long long off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// number of vertices = ring_offsets[n_rings], never more than the workspace was sized for
__device__ __forceinline__ int vertex_count(const int* ro, int n_rings, int nmax) {
  const int n = ro[n_rings];
  return n < 0 ? 0 : (n > nmax ? nmax : n);
}

// ---- 1. per-edge row spans and their exclusive scan ---------------------------------------------------------------

__global__ __launch_bounds__(kScanT) void zone_span_kernel(const double* __restrict__ xy, const int* __restrict__ ro,
                                                           int n_rings, int nmax, int H, int* __restrict__ rfirst,
                                                           int* __restrict__ nxt, long long* __restrict__ offs) {
  __shared__ long long s_wave[kScanT / 64];
  __shared__ long long s_carry;
  const int n = vertex_count(ro, n_rings, nmax);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kScanT) {
    const int e = base + tid;
    long long span = 0;
    if (e < n) {
      // ring k with ro[k] <= e < ro[k + 1]: the last k whose start is <= e (empty rings are stepped over)
      int lo = 0, hi = n_rings;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ro[mid] <= e) lo = mid; else hi = mid;
      }
      int nx = e + 1 == ro[lo + 1] ? ro[lo] : e + 1;
      nx = nx < 0 ? 0 : (nx >= n ? n - 1 : nx);  // malformed offsets must not index outside xy
      const double x0 = xy[2ll * e], y0 = xy[2ll * e + 1], x1 = xy[2ll * nx], y1 = xy[2ll * nx + 1];
      int first = 0;
      if (y0 != y1 && isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1)) {
        // rows r with min <= r + 0.5 < max, widened by a row on either side: the toggle pass tests the exact predicate
        double a = floor(fmin(y0, y1) - 0.5), b = ceil(fmax(y0, y1) - 0.5) + 1.0;
        a = fmax(a, 0.0);
        b = fmin(b, (double)H);
        if (b > a) {
          first = (int)a;
          span = (long long)(b - a);
        }
      }
      rfirst[e] = first;
      nxt[e] = nx;
    }
    // block-wide exclusive scan: wave scan by shuffles, wave totals through LDS
    long long incl = span;
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (e < n) offs[e] = before + incl - span;
    __syncthreads();
    if (tid == kScanT - 1) s_carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) offs[n] = s_carry;
}

// ---- 2. toggles ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void zone_toggle_kernel(const double* __restrict__ xy, const int* __restrict__ ro,
                                                         int n_rings, int nmax, int H, int W, int WW,
                                                         const int* __restrict__ rfirst, const int* __restrict__ nxt,
                                                         const long long* __restrict__ offs,
                                                         unsigned int* __restrict__ tog) {
  const int n = vertex_count(ro, n_rings, nmax);
  if (n == 0) return;
  const long long total = offs[n];
  const long long stride = (long long)gridDim.x * kT;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += stride) {
    // edge e with offs[e] <= i < offs[e + 1]
    int lo = 0, hi = n;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    const int e = lo, nx = nxt[e];
    const int r = rfirst[e] + (int)(i - offs[e]);
    if (r < 0 || r >= H) continue;
    const double x0 = xy[2ll * e], y0 = xy[2ll * e + 1], x1 = xy[2ll * nx], y1 = xy[2ll * nx + 1];
    int c;
    if (!ffa_zone_crossing(x0, y0, x1, y1, r, W, &c)) continue;
    if (c < W) atomicXor(&tog[(long long)r * WW + (c >> 5)], 1u << (c & 31));
  }
}

// ---- 3. row scan: toggle bits -> inside bits, in place --------------------------------------------------------------

__global__ __launch_bounds__(kT) void zone_row_scan_kernel(int H, int WW, unsigned int* __restrict__ tog) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if (row >= H) return;  // whole waves leave; there is no block-wide barrier below
  unsigned int* bits = tog + row * WW;
  unsigned int carry = 0;  // wave-uniform: parity of all toggles of the row in the words already done
  for (int w0 = 0; w0 < WW; w0 += 64) {
    const int w = w0 + lane;
    unsigned int p = w < WW ? bits[w] : 0u;
    p = ffa_zone_prefix_xor(p);  // bit k = XOR of the word's toggles at bits <= k; bit 31 = parity of the word
    const unsigned long long odd = __ballot((p >> 31) != 0);
    const unsigned int in = (unsigned int)(__popcll(odd & ((1ull << lane) - 1ull)) & 1) ^ carry;
    if (in) p = ~p;
    if (w < WW) bits[w] = p;
    carry ^= (unsigned int)(__popcll(odd) & 1);
  }
}

// ---- 4. expand bits to bytes ----------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned int spread4(unsigned int nib) {
  return (nib * 0x00204081u) & 0x01010101u;  // bit i of the nibble -> byte i (the 16 partial products do not collide)
}

__global__ __launch_bounds__(kT) void zone_expand_kernel(const unsigned int* __restrict__ bits, int W, int WW,
                                                         long long N, int head, long long groups, int accumulate,
                                                         uint8_t* __restrict__ mask) {
  const long long stride = (long long)gridDim.x * kT;
  for (long long g = (long long)blockIdx.x * kT + threadIdx.x; g < groups; g += stride) {
    const long long i0 = 16 * g - head;  // mask + i0 is 16-byte aligned
    const long long row = i0 >= 0 ? i0 / W : 0;
    const int col = (int)(i0 - row * W);
    if (i0 >= 0 && i0 + 16 <= N && col + 16 <= W) {
      const unsigned int* rb = bits + row * WW;
      const int wi = col >> 5, sh = col & 31;
      const unsigned long long two = (unsigned long long)rb[wi] | ((unsigned long long)(wi + 1 < WW ? rb[wi + 1] : 0u) << 32);
      const unsigned int v = (unsigned int)(two >> sh) & 0xffffu;
      uint4 o = make_uint4(spread4(v & 15u), spread4((v >> 4) & 15u), spread4((v >> 8) & 15u), spread4(v >> 12));
      uint4* dst = reinterpret_cast<uint4*>(mask + i0);
      if (accumulate) {
        const uint4 old = *dst;
        o.x |= old.x;
        o.y |= old.y;
        o.z |= old.z;
        o.w |= old.w;
      }
      *dst = o;
    } else {  // the group straddles a row end or an end of the mask: byte by byte
      for (int k = 0; k < 16; ++k) {
        const long long i = i0 + k;
        if (i < 0 || i >= N) continue;
        const long long r = i / W;
        const int c = (int)(i - r * W);
        const uint8_t b = (uint8_t)((bits[r * WW + (c >> 5)] >> (c & 31)) & 1u);
        mask[i] = accumulate ? (uint8_t)(mask[i] | b) : b;
      }
    }
  }
}

// ---- clip: out = mask ? lut[class] : fill ---------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void zone_clip_kernel(uint8_t* __restrict__ cls, const uint8_t* __restrict__ mask,
                                                       const uint8_t* __restrict__ lut, long long n, int head,
                                                       long long groups, int fill) {
  __shared__ uint8_t s_lut[256];
  s_lut[threadIdx.x] = lut ? lut[threadIdx.x] : (uint8_t)threadIdx.x;  // kT == 256
  __syncthreads();
  const uint8_t f = (uint8_t)fill;
  const bool mask_vec = mask && (((uintptr_t)mask - (uintptr_t)head) & 15) == 0;  // mask + i0 aligned like cls + i0
  const long long stride = (long long)gridDim.x * kT;
  for (long long g = (long long)blockIdx.x * kT + threadIdx.x; g < groups; g += stride) {
    const long long i0 = 16 * g - head;  // cls + i0 is 16-byte aligned
    if (i0 >= 0 && i0 + 16 <= n) {
      union { uint4 v; uint8_t b[16]; } c, m;
      c.v = *reinterpret_cast<const uint4*>(cls + i0);
      if (!mask) {
        m.v = make_uint4(~0u, ~0u, ~0u, ~0u);
      } else if (mask_vec) {
        m.v = *reinterpret_cast<const uint4*>(mask + i0);
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) m.b[k] = mask[i0 + k];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) c.b[k] = m.b[k] ? s_lut[c.b[k]] : f;
      *reinterpret_cast<uint4*>(cls + i0) = c.v;
    } else {
      for (int k = 0; k < 16; ++k) {
        const long long i = i0 + k;
        if (i < 0 || i >= n) continue;
        cls[i] = (!mask || mask[i]) ? s_lut[cls[i]] : f;
      }
    }
  }
}

// ---- window counts: one block per rectangle -------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void zone_window_count_kernel(const uint8_t* __restrict__ mask, int H, int W,
                                                               const int* __restrict__ win,
                                                               long long* __restrict__ counts) {
  __shared__ long long s_part[kT / 64];
  const int* q = win + 4ll * blockIdx.x;
  const int r0 = max(q[0], 0), c0 = max(q[1], 0), r1 = min(q[2], H), c1 = min(q[3], W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long acc = 0;
  if (r1 > r0 && c1 > c0) {
    for (int r = r0 + wave; r < r1; r += kT / 64) {  // a wave per row, lanes along the columns
      const uint8_t* p = mask + (long long)r * W;
      for (int c = c0 + lane; c < c1; c += 64) acc += p[c] != 0;
    }
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int w = 0; w < kT / 64; ++w) s += s_part[w];
    counts[blockIdx.x] = s;  // the only writer of this entry: integer sums, exact and deterministic
  }
}

unsigned int grid_stride_blocks(long long items) {
  const long long b = (items + kT - 1) / kT;
  return (unsigned int)(b < 1 ? 1 : (b > (1 << 16) ? (1 << 16) : b));
}

}  // namespace

extern "C" long long ffa_zone_mask_workspace_bytes(int H, int W, long long n_vertices) {
  if (H < 1 || W < 1 || n_vertices < 0 || n_vertices >= (1ll << 31) - 1) {
    ffa_set_error("zone_mask: raster %d x %d, %lld vertices outside 1 <= H, W and 0 <= vertices < 2^31 - 1", H, W,
                  n_vertices);
    return FFA_ERR_ARG;
  }
  return make_layout(H, W, n_vertices < 1 ? 1 : n_vertices).total;
}

extern "C" int ffa_zone_mask_u8(const double* xy_pix, const int32_t* ring_offsets, int n_rings, int H, int W,
                                uint8_t* mask, int accumulate, void* ws, long long ws_bytes, hipStream_t st) {
  FFA_REQUIRE(H >= 1 && W >= 1, "zone_mask: raster %d x %d outside 1 <= H, W", H, W);
  FFA_REQUIRE(n_rings >= 0 && mask, "zone_mask: %d rings, mask %p", n_rings, (void*)mask);
  const long long N = (long long)H * W;
  if (n_rings == 0) {  // nothing is inside
    if (!accumulate) (void)hipMemsetAsync(mask, 0, N, st);
    return ffa_check_launch("zone_mask");
  }
  FFA_REQUIRE(xy_pix && ring_offsets && ws, "zone_mask: null pointer");
  // the vertex count ring_offsets[n_rings] lives on the device: the workspace size bounds what the kernels touch
  const Layout fixed = make_layout(H, W, 1);
  const long long nmax_ll = (ws_bytes - fixed.offs - 8) / 16;
  if (ws_bytes < fixed.total || nmax_ll < 1) {
    ffa_set_error("zone_mask: workspace %lld bytes < %lld", ws_bytes, fixed.total);
    return FFA_ERR_WORKSPACE;
  }
  const int nmax = (int)(nmax_ll > (1ll << 31) - 2 ? (1ll << 31) - 2 : nmax_ll);
  const Layout lo = make_layout(H, W, nmax);
  unsigned int* tog = at<unsigned int>(ws, lo.tog);
  long long* offs = at<long long>(ws, lo.offs);
  int* rfirst = at<int>(ws, lo.rfirst);
  int* nxt = at<int>(ws, lo.nxt);

  (void)hipMemsetAsync(tog, 0, 4ll * H * lo.WW, st);
  hipLaunchKernelGGL(zone_span_kernel, dim3(1), dim3(kScanT), 0, st, xy_pix, ring_offsets, n_rings, nmax, H, rfirst,
                     nxt, offs);
  // the item count is on the device too: a fixed grid walks it with a grid stride (8 blocks per CU)
  hipLaunchKernelGGL(zone_toggle_kernel, dim3(2048), dim3(kT), 0, st, xy_pix, ring_offsets, n_rings, nmax, H, W, lo.WW,
                     rfirst, nxt, offs, tog);
  hipLaunchKernelGGL(zone_row_scan_kernel, dim3((unsigned int)((H + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, H,
                     lo.WW, tog);
  const int head = (int)((uintptr_t)mask & 15);
  const long long groups = (N + head + 15) / 16;
  hipLaunchKernelGGL(zone_expand_kernel, dim3(grid_stride_blocks(groups)), dim3(kT), 0, st, tog, W, lo.WW, N, head,
                     groups, accumulate != 0, mask);
  return ffa_check_launch("zone_mask");
}

extern "C" int ffa_zone_clip_u8(uint8_t* classes, const uint8_t* mask, const uint8_t* lut256, long long n, int fill,
                                hipStream_t st) {
  FFA_REQUIRE(n >= 0 && (classes || n == 0), "zone_clip: null class raster");
  FFA_REQUIRE(fill >= 0 && fill <= 255, "zone_clip: fill %d is not a uint8 value", fill);
  if (n == 0) return FFA_OK;
  const int head = (int)((uintptr_t)classes & 15);
  const long long groups = (n + head + 15) / 16;
  hipLaunchKernelGGL(zone_clip_kernel, dim3(grid_stride_blocks(groups)), dim3(kT), 0, st, classes, mask, lut256, n,
                     head, groups, fill);
  return ffa_check_launch("zone_clip");
}

extern "C" int ffa_zone_window_counts(const uint8_t* mask, int H, int W, const int32_t* windows, int n_windows,
                                      int64_t* counts, hipStream_t st) {
  FFA_REQUIRE(H >= 1 && W >= 1 && n_windows >= 0, "zone_window_counts: raster %d x %d, %d windows", H, W, n_windows);
  if (n_windows == 0) return FFA_OK;
  FFA_REQUIRE(mask && windows && counts, "zone_window_counts: null pointer");
  hipLaunchKernelGGL(zone_window_count_kernel, dim3((unsigned int)n_windows), dim3(kT), 0, st, mask, H, W, windows,
                     reinterpret_cast<long long*>(counts));
  return ffa_check_launch("zone_window_counts");
}
