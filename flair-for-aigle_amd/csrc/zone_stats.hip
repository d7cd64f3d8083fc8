// Zonal statistics: for Z zones (rings in pixel coordinates) over a uint8 class raster, the pixel count per (zone,
// class) and the sum of a uint8 confidence raster over the same pixels.  include/flairhip_zonestats.h holds the
// normative definition and the tables the host provides.
//
// The full-raster XOR plane of zone_mask.hip does not generalise to many zones: here each zone has its own bit plane
// over its own window (r0, c0, r1, c1), c0 a multiple of 32, all planes packed in one workspace array.
//
// ffa_zone_stats_u8 (separate launches, no grid-wide barrier):
//   1. spans    zstat_span_kernel: per edge its ring (binary search in ring_offsets), the ring's zone (binary search in
//               zone_ring_offsets), the first row of the zone's window its y range can cross and a conservative row
//               count; zstat_scan_kernel: the exclusive scan of those counts, one block (10^5 parcels have 4 * 10^5
//               edges: the searches are kept out of the serial part).
//   2. toggles  zstat_toggle_kernel: one item per (edge, row); the crossing predicate and column of ffa_zone.h, then one
//               atomicXor of one bit into the zone's plane.  A crossing left of c0 toggles local column 0, one at or
//               beyond c1 has no effect.
//   3. row scan zstat_row_scan_kernel: a wave per work item.  Narrow windows (parcels, <= 8 words per row): a lane per
//               row, 64 rows per item, the carry from word to word in a register.  Wide windows: a wave per row, carry
//               across words by ballot and a running carry beyond 64 words, as zone_row_scan_kernel has.
//   4. tabulate zstat_tabulate_kernel (the hot pass): a wave per chunk (zone, first word, words).  A lane skips zero
//               words; since c0 is a multiple of 32, a plane word covers 32 consecutive class bytes, fetched as two
//               16-byte loads (and the confidence bytes likewise).  Runs of one class inside a word are summed in
//               registers, then added to a per-wave LDS table uint32 [K + 1] (a second one for the confidence sums);
//               non-zero entries are flushed with 64-bit integer atomicAdd.  No floating point in this pass.
// The planes are cleared at the head of every call and the outputs too, so the workspace may hold anything.
//
// ffa_zone_change_u8 (include/flairhip_change.h) tabulates two rasters over the same zones: stages 1 - 3 are the one
// host function zstat_build_planes for both entry points, stage 4 is zchange_tabulate_kernel, a transition matrix
// uint32 [K + 1][K + 1] per wave in place of the class table.
#include "ffa_common.h"
#include "ffa_zone.h"  // the crossing predicate and column, shared with zone_mask.hip

// the crossing column must round every operation separately (ffa_zone.h)
#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kScanT = 1024;
constexpr long long kAlign = 256;
constexpr int kMaxK = 256;
constexpr int kNarrow = FFA_ZONE_STATS_NARROW_WORDS;
constexpr int kChunkWords = FFA_ZONE_STATS_CHUNK_WORDS;
static_assert(255ll * 32 * kChunkWords < (1ll << 32), "a per-wave 32-bit confidence sum must not overflow");
constexpr int kChangeMaxK = FFA_CHANGE_MAX_CLASSES;
constexpr int kChangeTab = (kChangeMaxK + 1) * (kChangeMaxK + 1);  // entries of one per-wave transition table
static_assert(2 * kWaves * kChangeTab * 4 <= 48 * 1024, "the transition tables of a block must fit static LDS");
static_assert(kChangeMaxK < 64, "a lane per column and a 64-bit row mask in the flush");

inline long long align_up(long long v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Layout {
  long long planes, offs, rfirst, nxt, ezone, total;
};

Layout make_layout(long long plane_words, long long n) {
  Layout lo;
  lo.planes = 0;
  lo.offs = align_up(4 * plane_words);  // int64 [n + 1], then three int32 [n] arrays
  lo.rfirst = lo.offs + 8 * (n + 1);
  lo.nxt = lo.rfirst + 4 * n;
  lo.ezone = lo.nxt + 4 * n;
  lo.total = lo.ezone + 4 * n;
  return lo;
}

template <typename T>
inline T* at(void* ws, long long off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// A zone's window as the kernels use it: clamped to the raster whatever the table says, c0 rounded down to 32.
struct Win {
  int r0, c0, r1, c1, ww;
};

__device__ __forceinline__ Win load_window(const int* __restrict__ win, int z, int H, int W) {
  const int* q = win + 4ll * z;
  Win w;
  w.r0 = max(q[0], 0);
  w.c0 = max(q[1], 0) & ~31;
  w.r1 = min(q[2], H);
  w.c1 = min(q[3], W);
  w.ww = (w.r1 > w.r0 && w.c1 > w.c0) ? (w.c1 - w.c0 + 31) >> 5 : 0;  // 0: the zone has no plane
  return w;
}

// last k in [0, n) with t[k] <= v (tables that rise; equal entries = empty rings / zones are stepped over)
template <typename T>
__device__ __forceinline__ int last_not_above(const T* __restrict__ t, int n, T v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (t[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- 1. per-edge row spans and their exclusive scan ---------------------------------------------------------------

__global__ __launch_bounds__(kT) void zstat_span_kernel(const double* __restrict__ xy, int n,
                                                        const int* __restrict__ ro, int n_rings,
                                                        const int* __restrict__ zro, int Z,
                                                        const int* __restrict__ win, int H, int W,
                                                        int* __restrict__ rfirst, int* __restrict__ nxt,
                                                        int* __restrict__ ezone, long long* __restrict__ offs) {
  const long long stride = (long long)gridDim.x * kT;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += stride) {
    const int e = (int)i;
    const int ring = last_not_above(ro, n_rings, e);
    int nx = e + 1 == ro[ring + 1] ? ro[ring] : e + 1;
    nx = nx < 0 ? 0 : (nx >= n ? n - 1 : nx);  // malformed offsets must not index outside xy
    const int z = last_not_above(zro, Z, ring);
    const Win w = load_window(win, z, H, W);
    const double x0 = xy[2ll * e], y0 = xy[2ll * e + 1], x1 = xy[2ll * nx], y1 = xy[2ll * nx + 1];
    int first = 0;
    long long span = 0;
    if (w.ww > 0 && y0 != y1 && isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1)) {
      // rows r with min <= r + 0.5 < max, widened by a row on either side: the toggle pass tests the exact predicate
      double a = floor(fmin(y0, y1) - 0.5), b = ceil(fmax(y0, y1) - 0.5) + 1.0;
      a = fmax(a, (double)w.r0);
      b = fmin(b, (double)w.r1);
      if (b > a) {
        first = (int)a;
        span = (long long)(b - a);
      }
    }
    rfirst[e] = first;
    nxt[e] = nx;
    ezone[e] = z;
    offs[e] = span;  // the scan below turns the counts into offsets
  }
}

// offs[0 .. n) (row counts) -> their exclusive scan in place, offs[n] = the total.  One block: 4 entries a thread per
// step, wave scan by shuffles, wave totals through LDS.  The searches and the coordinate loads stay in the parallel
// kernel above, so a step here is one load, one store and two barriers.
__global__ __launch_bounds__(kScanT) void zstat_scan_kernel(int n, long long* __restrict__ offs) {
  constexpr int kPer = 4;
  __shared__ long long s_wave[kScanT / 64];
  __shared__ long long s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += kScanT * kPer) {
    const long long e0 = base + (long long)tid * kPer;
    long long v[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      v[k] = e0 + k < n ? offs[e0 + k] : 0;
      sum += v[k];
    }
    long long incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long before = s_carry;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    long long run = before + incl - sum;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (e0 + k < n) offs[e0 + k] = run;
      run += v[k];
    }
    __syncthreads();
    if (tid == kScanT - 1) s_carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) offs[n] = s_carry;
}

// ---- 2. toggles ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void zstat_toggle_kernel(const double* __restrict__ xy, int n,
                                                          const int* __restrict__ win,
                                                          const long long* __restrict__ plane_off, long long plane_words,
                                                          int H, int W, const int* __restrict__ rfirst,
                                                          const int* __restrict__ nxt, const int* __restrict__ ezone,
                                                          const long long* __restrict__ offs,
                                                          unsigned int* __restrict__ planes) {
  const long long total = offs[n];
  const long long stride = (long long)gridDim.x * kT;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += stride) {
    const int e = last_not_above(offs, n, i);  // edge e with offs[e] <= i < offs[e + 1]
    const int nx = nxt[e], z = ezone[e];
    const Win w = load_window(win, z, H, W);
    const int r = rfirst[e] + (int)(i - offs[e]);
    if (r < w.r0 || r >= w.r1) continue;
    const double x0 = xy[2ll * e], y0 = xy[2ll * e + 1], x1 = xy[2ll * nx], y1 = xy[2ll * nx + 1];
    int c;
    if (!ffa_zone_crossing(x0, y0, x1, y1, r, W, &c)) continue;
    if (c >= w.c1) continue;                 // at or beyond the window's right end: no effect
    const int lc = c > w.c0 ? c - w.c0 : 0;  // left of the window: the whole row of the window is on its right
    const long long word = plane_off[z] + (long long)(r - w.r0) * w.ww + (lc >> 5);
    if (word >= 0 && word < plane_words) atomicXor(&planes[word], 1u << (lc & 31));
  }
}

// ---- 3. row scan: toggle bits -> inside bits, in place --------------------------------------------------------------

__global__ __launch_bounds__(kT) void zstat_row_scan_kernel(const int* __restrict__ win,
                                                            const long long* __restrict__ plane_off,
                                                            long long plane_words,
                                                            const long long* __restrict__ scan_starts, int Z,
                                                            long long items, int H, int W,
                                                            unsigned int* __restrict__ planes) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (item >= items) return;  // whole waves leave; there is no block-wide barrier below
  const int z = last_not_above(scan_starts, Z, item);
  const Win w = load_window(win, z, H, W);
  const long long idx = item - scan_starts[z];
  const long long rows = w.r1 - w.r0;
  if (w.ww == 0 || idx < 0) return;
  const long long base = plane_off[z];
  if (w.ww <= kNarrow) {  // a lane per row: the carry from word to word stays in a register
    const long long row = idx * 64 + lane;
    const long long p0 = base + row * w.ww;
    if (row >= rows || p0 < 0 || p0 + w.ww > plane_words) return;
    unsigned int carry = 0;
    for (int k = 0; k < w.ww; ++k) {
      unsigned int p = ffa_zone_prefix_xor(planes[p0 + k]);
      if (carry) p = ~p;
      planes[p0 + k] = p;
      carry = p >> 31;  // inside at the word's last column = inside on entry to the next word
    }
    return;
  }
  if (idx >= rows) return;
  const long long p0 = base + idx * w.ww;
  if (p0 < 0 || p0 + w.ww > plane_words) return;
  unsigned int* bits = planes + p0;
  unsigned int carry = 0;  // wave-uniform: parity of all toggles of the row in the words already done
  for (int w0 = 0; w0 < w.ww; w0 += 64) {
    const int k = w0 + lane;
    unsigned int p = k < w.ww ? bits[k] : 0u;
    p = ffa_zone_prefix_xor(p);
    const unsigned long long odd = __ballot((p >> 31) != 0);
    const unsigned int in = (unsigned int)(__popcll(odd & ((1ull << lane) - 1ull)) & 1) ^ carry;
    if (in) p = ~p;
    if (k < w.ww) bits[k] = p;
    carry ^= (unsigned int)(__popcll(odd) & 1);
  }
}

// ---- 4. tabulate ----------------------------------------------------------------------------------------------------

// 32 raster bytes from byte offset off (any alignment) as 8 dwords; bytes at or beyond n read as 0
__device__ __forceinline__ void load32(const uint8_t* __restrict__ p, long long off, long long n, unsigned int (&v)[8]) {
  if (off + 32 <= n) {
    uint4 a, b;
    __builtin_memcpy(&a, p + off, 16);
    __builtin_memcpy(&b, p + off + 16, 16);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {  // the tail of the raster's last row
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      unsigned int d = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = off + 4 * k + j;
        if (i < n) d |= (unsigned int)p[i] << (8 * j);
      }
      v[k] = d;
    }
  }
}

template <bool kConf>
__global__ __launch_bounds__(kT) void zstat_tabulate_kernel(const uint8_t* __restrict__ cls,
                                                            const uint8_t* __restrict__ conf, int H, int W, int K,
                                                            const int* __restrict__ win,
                                                            const long long* __restrict__ plane_off,
                                                            long long plane_words, int Z,
                                                            const int* __restrict__ chunks, long long n_chunks,
                                                            const unsigned int* __restrict__ planes,
                                                            unsigned long long* __restrict__ counts,
                                                            unsigned long long* __restrict__ sums) {
  __shared__ unsigned int s_cnt[kWaves][kMaxK + 1];
  __shared__ unsigned int s_sum[kConf ? kWaves : 1][kMaxK + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int* cnt = s_cnt[wave];
  unsigned int* sum = s_sum[kConf ? wave : 0];
  for (int k = lane; k <= K; k += 64) {
    cnt[k] = 0;
    if (kConf) sum[k] = 0;
  }
  __syncthreads();  // every thread of the block reaches both barriers: waves without a chunk only skip the work between

  const long long chunk = (long long)blockIdx.x * kWaves + wave;
  int z = -1;
  if (chunk < n_chunks) {
    const int* q = chunks + 3 * chunk;
    z = q[0];
    const int first = q[1];
    const int nw = min(q[2], kChunkWords);  // more would overflow the 32-bit partial sums
    if (z >= 0 && z < Z && first >= 0) {
      const Win w = load_window(win, z, H, W);
      const long long base = plane_off[z];
      const long long zone_words = (long long)(w.r1 - w.r0) * w.ww;
      const long long N = (long long)H * W;
      for (int j = lane; j < nw; j += 64) {
        const long long wi = (long long)first + j;
        if (w.ww == 0 || wi >= zone_words || base + wi < 0 || base + wi >= plane_words) break;  // j only rises
        unsigned int bits = planes[base + wi];
        const int r = w.r0 + (int)(wi / w.ww);
        const int col = w.c0 + 32 * (int)(wi % w.ww);
        const int valid = w.c1 - col;  // >= 1: col < c0 + 32 ww - 31 <= c1
        if (valid < 32) bits &= (1u << valid) - 1u;  // the scan runs to the word's end, the window does not
        if (bits == 0) continue;
        const long long off = (long long)r * W + col;
        unsigned int cv[8], fv[8];
        load32(cls, off, N, cv);
        if (kConf) load32(conf, off, N, fv);
        // runs of one class are summed in registers: a uniform field costs one LDS atomic per word, not 32
        int cur = 0;
        unsigned int run = 0, rsum = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          if ((bits >> k) & 1u) {
            int c = (int)((cv[k >> 2] >> (8 * (k & 3))) & 255u);
            c = c < K ? c : K;
            if (c != cur && run) {
              atomicAdd(&cnt[cur], run);
              if (kConf) atomicAdd(&sum[cur], rsum);
              run = 0;
              rsum = 0;
            }
            cur = c;
            run += 1;
            if (kConf) rsum += (fv[k >> 2] >> (8 * (k & 3))) & 255u;
          }
        }
        atomicAdd(&cnt[cur], run);  // bits != 0: the last run is never empty
        if (kConf) atomicAdd(&sum[cur], rsum);
      }
    } else {
      z = -1;
    }
  }
  __syncthreads();
  if (z < 0) return;
  for (int k = lane; k <= K; k += 64) {
    const unsigned int c = cnt[k];
    if (c) atomicAdd(&counts[(long long)z * (K + 1) + k], (unsigned long long)c);
    if (kConf) {
      const unsigned int s = sum[k];
      if (s) atomicAdd(&sums[(long long)z * (K + 1) + k], (unsigned long long)s);
    }
  }
}

// ---- 4b. tabulate two rasters: transition matrices --------------------------------------------------------------------

// The sibling of zstat_tabulate_kernel for ffa_zone_change_u8: the key of a member pixel is a * (K + 1) + b with
// a = min(before, K), b = min(after, K), the per-wave tables hold (K + 1)^2 entries.  Clearing and flushing 1089 entries
// per chunk would cost a parcel of a few words more than its pixels do, so the tables are cleared once per block, the
// blocks walk the chunk list with a stride, and a wave flushes and re-clears only the rows a its chunk touched (a
// 64-bit mask per lane, OR-ed over the wave): 2 LDS reads per touched row, lane b taking column b.  Every wave of a block
// makes the same number of trips (the bound depends on blockIdx alone), so the barriers are reached by all of them.
template <bool kConf>
__global__ __launch_bounds__(kT) void zchange_tabulate_kernel(const uint8_t* __restrict__ before,
                                                              const uint8_t* __restrict__ after,
                                                              const uint8_t* __restrict__ conf, int H, int W, int K,
                                                              const int* __restrict__ win,
                                                              const long long* __restrict__ plane_off,
                                                              long long plane_words, int Z,
                                                              const int* __restrict__ chunks, long long n_chunks,
                                                              const unsigned int* __restrict__ planes,
                                                              unsigned long long* __restrict__ counts,
                                                              unsigned long long* __restrict__ sums) {
  __shared__ unsigned int s_cnt[kWaves * kChangeTab];
  __shared__ unsigned int s_sum[kConf ? kWaves * kChangeTab : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < kWaves * kChangeTab; k += kT) {
    s_cnt[k] = 0;
    if (kConf) s_sum[k] = 0;
  }
  __syncthreads();
  unsigned int* cnt = s_cnt + wave * kChangeTab;
  unsigned int* sum = s_sum + (kConf ? wave * kChangeTab : 0);
  const int K1 = K + 1;
  const long long N = (long long)H * W;

  for (long long first_chunk = (long long)blockIdx.x * kWaves; first_chunk < n_chunks;
       first_chunk += (long long)gridDim.x * kWaves) {
    const long long chunk = first_chunk + wave;
    int z = -1;
    unsigned long long rows = 0;  // bit a: this lane added to row a of the wave's tables
    if (chunk < n_chunks) {
      const int* q = chunks + 3 * chunk;
      z = q[0];
      const int first = q[1];
      const int nw = min(q[2], kChunkWords);  // more would overflow the 32-bit partial sums
      if (z >= 0 && z < Z && first >= 0) {
        const Win w = load_window(win, z, H, W);
        const long long base = plane_off[z];
        const long long zone_words = (long long)(w.r1 - w.r0) * w.ww;
        for (int j = lane; j < nw; j += 64) {
          const long long wi = (long long)first + j;
          if (w.ww == 0 || wi >= zone_words || base + wi < 0 || base + wi >= plane_words) break;  // j only rises
          unsigned int bits = planes[base + wi];
          const int r = w.r0 + (int)(wi / w.ww);
          const int col = w.c0 + 32 * (int)(wi % w.ww);
          const int valid = w.c1 - col;  // >= 1, as in zstat_tabulate_kernel
          if (valid < 32) bits &= (1u << valid) - 1u;
          if (bits == 0) continue;
          const long long off = (long long)r * W + col;
          unsigned int av[8], bv[8], fv[8];
          load32(before, off, N, av);
          load32(after, off, N, bv);
          if (kConf) load32(conf, off, N, fv);
          // runs of one key are summed in registers: an unchanged uniform field costs one LDS atomic per word
          int cur = 0;
          unsigned int run = 0, rsum = 0;
#pragma unroll
          for (int k = 0; k < 32; ++k) {
            if ((bits >> k) & 1u) {
              const int sh = 8 * (k & 3);
              const int a = min((int)((av[k >> 2] >> sh) & 255u), K);
              const int b = min((int)((bv[k >> 2] >> sh) & 255u), K);
              const int key = a * K1 + b;  // < (K + 1)^2 <= kChangeTab
              if (key != cur && run) {
                atomicAdd(&cnt[cur], run);
                if (kConf) atomicAdd(&sum[cur], rsum);
                run = 0;
                rsum = 0;
              }
              if (run == 0) rows |= 1ull << a;
              cur = key;
              run += 1;
              if (kConf) rsum += (fv[k >> 2] >> sh) & 255u;
            }
          }
          atomicAdd(&cnt[cur], run);  // bits != 0: the last run is never empty
          if (kConf) atomicAdd(&sum[cur], rsum);
        }
      } else {
        z = -1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows |= __shfl_xor(rows, o, 64);  // wave-uniform from here
    if (z >= 0) {
      const long long out0 = (long long)z * K1 * K1;
      while (rows) {
        const int a = __builtin_ctzll(rows);  // <= K: only clamped classes set a bit
        rows &= rows - 1;
        if (lane <= K) {
          const int key = a * K1 + lane;
          const unsigned int c = cnt[key];
          if (c) {
            atomicAdd(&counts[out0 + key], (unsigned long long)c);
            cnt[key] = 0;
          }
          if (kConf) {
            const unsigned int s = sum[key];
            if (s) {
              atomicAdd(&sums[out0 + key], (unsigned long long)s);
              sum[key] = 0;
            }
          }
        }
      }
    }
    __syncthreads();  // the tables are clear again before the next chunk's adds
  }
}

}  // namespace

extern "C" long long ffa_zone_stats_workspace_bytes(long long n_vertices, long long plane_words, long long n_chunks) {
  if (n_vertices < 0 || n_vertices >= (1ll << 31) - 1 || plane_words < 0 || plane_words > (1ll << 40) || n_chunks < 0 ||
      n_chunks > (1ll << 31) - 1) {
    ffa_set_error("zone_stats: %lld vertices, %lld plane words, %lld chunks outside 0 <= vertices < 2^31 - 1, "
                  "0 <= plane words <= 2^40, 0 <= chunks < 2^31", n_vertices, plane_words, n_chunks);
    return FFA_ERR_ARG;
  }
  return make_layout(plane_words, n_vertices < 1 ? 1 : n_vertices).total;
}

namespace {

// The argument ranges both entry points accept (their K ranges differ: max_k).
int zstat_check_args(const char* what, int H, int W, int K, int max_k, int n_zones, int n_rings, long long n_vertices,
                     long long plane_words, long long n_scan_items, long long n_chunks) {
  FFA_REQUIRE(H >= 1 && W >= 1, "%s: raster %d x %d outside 1 <= H, W", what, H, W);
  FFA_REQUIRE(K >= 1 && K <= max_k, "%s: %d classes outside 1..%d", what, K, max_k);
  FFA_REQUIRE(n_zones >= 0 && n_rings >= 0 && n_vertices >= 0 && n_vertices < (1ll << 31) - 1,
              "%s: %d zones, %d rings, %lld vertices outside 0 <= zones, rings and 0 <= vertices < 2^31 - 1", what,
              n_zones, n_rings, n_vertices);
  FFA_REQUIRE(plane_words >= 0 && plane_words <= (1ll << 40) && n_scan_items >= 0 && n_chunks >= 0 &&
                  n_scan_items <= kWaves * ((1ll << 31) - 1) && n_chunks <= (1ll << 31) - 1,
              "%s: %lld plane words, %lld scan items, %lld chunks out of range", what, plane_words, n_scan_items,
              n_chunks);
  return FFA_OK;
}

// Stages 1 - 3 for both entry points: the planes of all zones in the workspace, cleared, toggled and scanned, so that
// bit b of word w of a row of zone z's plane says whether column c0 + 32 w + b of that row is inside.  One function:
// the member pixels of ffa_zone_change_u8 are those of ffa_zone_stats_u8 because the same launches made them.
int zstat_build_planes(const char* what, int H, int W, const double* xy_pix, long long n_vertices,
                       const int32_t* ring_offsets, int n_rings, const int32_t* zone_ring_offsets, int n_zones,
                       const int32_t* windows, const int64_t* plane_offsets, long long plane_words,
                       const int64_t* scan_starts, long long n_scan_items, const int32_t* chunks, void* ws,
                       long long ws_bytes, hipStream_t st, unsigned int** planes_out) {
  FFA_REQUIRE(windows && plane_offsets && scan_starts && chunks && ws, "%s: null table or workspace", what);
  FFA_REQUIRE(n_vertices == 0 || (xy_pix && ring_offsets && zone_ring_offsets && n_rings >= 1),
              "%s: vertices without rings", what);
  const long long n = n_vertices;
  const Layout lo = make_layout(plane_words, n < 1 ? 1 : n);
  if (ws_bytes < lo.total) {
    ffa_set_error("%s: workspace %lld bytes < %lld", what, ws_bytes, lo.total);
    return FFA_ERR_WORKSPACE;
  }
  unsigned int* planes = at<unsigned int>(ws, lo.planes);
  (void)hipMemsetAsync(planes, 0, 4 * plane_words, st);
  if (n > 0) {
    long long* offs = at<long long>(ws, lo.offs);
    int* rfirst = at<int>(ws, lo.rfirst);
    int* nxt = at<int>(ws, lo.nxt);
    int* ezone = at<int>(ws, lo.ezone);
    const unsigned int span_blocks = (unsigned int)(n + kT - 1) / kT;
    hipLaunchKernelGGL(zstat_span_kernel, dim3(span_blocks < 2048 ? span_blocks : 2048), dim3(kT), 0, st, xy_pix,
                       (int)n, ring_offsets, n_rings, zone_ring_offsets, n_zones, windows, H, W, rfirst, nxt, ezone,
                       offs);
    hipLaunchKernelGGL(zstat_scan_kernel, dim3(1), dim3(kScanT), 0, st, (int)n, offs);
    // the item count is on the device: a fixed grid walks it with a grid stride (8 blocks per CU)
    hipLaunchKernelGGL(zstat_toggle_kernel, dim3(2048), dim3(kT), 0, st, xy_pix, (int)n, windows,
                       reinterpret_cast<const long long*>(plane_offsets), plane_words, H, W, rfirst, nxt, ezone, offs,
                       planes);
    if (n_scan_items > 0)
      hipLaunchKernelGGL(zstat_row_scan_kernel, dim3((unsigned int)((n_scan_items + kWaves - 1) / kWaves)), dim3(kT),
                         0, st, windows, reinterpret_cast<const long long*>(plane_offsets), plane_words,
                         reinterpret_cast<const long long*>(scan_starts), n_zones, n_scan_items, H, W, planes);
  }
  *planes_out = planes;
  return FFA_OK;
}

}  // namespace

extern "C" int ffa_zone_stats_u8(const uint8_t* cls, const uint8_t* conf, int H, int W, int K, const double* xy_pix,
                                 long long n_vertices, const int32_t* ring_offsets, int n_rings,
                                 const int32_t* zone_ring_offsets, int n_zones, const int32_t* windows,
                                 const int64_t* plane_offsets, long long plane_words, const int64_t* scan_starts,
                                 long long n_scan_items, const int32_t* chunks, long long n_chunks, int64_t* counts,
                                 int64_t* conf_sums, void* ws, long long ws_bytes, hipStream_t st) {
  int rc = zstat_check_args("zone_stats", H, W, K, kMaxK, n_zones, n_rings, n_vertices, plane_words, n_scan_items,
                            n_chunks);
  if (rc != FFA_OK) return rc;
  if (n_zones == 0) return FFA_OK;
  FFA_REQUIRE(cls && counts && (!conf || conf_sums), "zone_stats: null raster or output");
  const long long out_bytes = 8ll * n_zones * (K + 1);
  (void)hipMemsetAsync(counts, 0, out_bytes, st);
  if (conf) (void)hipMemsetAsync(conf_sums, 0, out_bytes, st);
  if (plane_words == 0 || n_chunks == 0) return ffa_check_launch("zone_stats");  // no zone reaches the raster
  unsigned int* planes = nullptr;
  rc = zstat_build_planes("zone_stats", H, W, xy_pix, n_vertices, ring_offsets, n_rings, zone_ring_offsets, n_zones,
                          windows, plane_offsets, plane_words, scan_starts, n_scan_items, chunks, ws, ws_bytes, st,
                          &planes);
  if (rc != FFA_OK) return rc;
  const dim3 grid((unsigned int)((n_chunks + kWaves - 1) / kWaves));
  auto* c64 = reinterpret_cast<unsigned long long*>(counts);
  auto* s64 = reinterpret_cast<unsigned long long*>(conf_sums);
  const auto* po = reinterpret_cast<const long long*>(plane_offsets);
  if (conf)
    hipLaunchKernelGGL(zstat_tabulate_kernel<true>, grid, dim3(kT), 0, st, cls, conf, H, W, K, windows, po,
                       plane_words, n_zones, chunks, n_chunks, planes, c64, s64);
  else
    hipLaunchKernelGGL(zstat_tabulate_kernel<false>, grid, dim3(kT), 0, st, cls, conf, H, W, K, windows, po,
                       plane_words, n_zones, chunks, n_chunks, planes, c64, s64);
  return ffa_check_launch("zone_stats");
}

extern "C" int ffa_zone_change_u8(const uint8_t* before, const uint8_t* after, const uint8_t* conf, int H, int W, int K,
                                  const double* xy_pix, long long n_vertices, const int32_t* ring_offsets, int n_rings,
                                  const int32_t* zone_ring_offsets, int n_zones, const int32_t* windows,
                                  const int64_t* plane_offsets, long long plane_words, const int64_t* scan_starts,
                                  long long n_scan_items, const int32_t* chunks, long long n_chunks, int64_t* counts,
                                  int64_t* conf_sums, void* ws, long long ws_bytes, hipStream_t st) {
  int rc = zstat_check_args("zone_change", H, W, K, kChangeMaxK, n_zones, n_rings, n_vertices, plane_words,
                            n_scan_items, n_chunks);
  if (rc != FFA_OK) return rc;
  if (n_zones == 0) return FFA_OK;
  FFA_REQUIRE(before && after && counts && (!conf || conf_sums), "zone_change: null raster or output");
  const long long out_bytes = 8ll * n_zones * (K + 1) * (K + 1);
  (void)hipMemsetAsync(counts, 0, out_bytes, st);
  if (conf) (void)hipMemsetAsync(conf_sums, 0, out_bytes, st);
  if (plane_words == 0 || n_chunks == 0) return ffa_check_launch("zone_change");  // no zone reaches the raster
  unsigned int* planes = nullptr;
  rc = zstat_build_planes("zone_change", H, W, xy_pix, n_vertices, ring_offsets, n_rings, zone_ring_offsets, n_zones,
                          windows, plane_offsets, plane_words, scan_starts, n_scan_items, chunks, ws, ws_bytes, st,
                          &planes);
  if (rc != FFA_OK) return rc;
  // the tables take 34848 bytes of LDS: 4 blocks fit a CU (160 KB), and the blocks stride over the chunk list
  const long long blocks = (n_chunks + kWaves - 1) / kWaves;
  const dim3 grid((unsigned int)(blocks < 1024 ? blocks : 1024));
  auto* c64 = reinterpret_cast<unsigned long long*>(counts);
  auto* s64 = reinterpret_cast<unsigned long long*>(conf_sums);
  const auto* po = reinterpret_cast<const long long*>(plane_offsets);
  if (conf)
    hipLaunchKernelGGL(zchange_tabulate_kernel<true>, grid, dim3(kT), 0, st, before, after, conf, H, W, K, windows, po,
                       plane_words, n_zones, chunks, n_chunks, planes, c64, s64);
  else
    hipLaunchKernelGGL(zchange_tabulate_kernel<false>, grid, dim3(kT), 0, st, before, after, conf, H, W, K, windows,
                       po, plane_words, n_zones, chunks, n_chunks, planes, c64, s64);
  return ffa_check_launch("zone_change");
}
