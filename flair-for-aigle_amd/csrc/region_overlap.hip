// Region overlaps of two uint8 class rasters on one grid: the pairs (region of A, region of B) that share pixels, with
// the size of each intersection (include/flairhip_objects.h has the definitions).  Integers only.
//
// ffa_region_overlap_count, per raster:
//   1. labels + counts  the polygoniser's labelling (ffa_ccl.h): root = smallest row-major pixel index, count on it
//   2. region index     the kept roots (count >= min_pixels) numbered in label order by a device-wide exclusive scan of
//                       their flags: block_sums_kernel -> scan_blocks_kernel (one block) -> index_kernel.  Within a
//                       block the scan is a ballot per wave and a popcount of the lanes below.
//   3. relabel          L[p] becomes the region index of pixel p's region, -1 where the pixel is background or its
//                       region was dropped; the class of a kept root is set aside, so that the second call needs no raster
// then heads_kernel counts the pair bound Q over both index rasters.
// ffa_region_overlap_pairs:
//   4. tables           one thread per pixel, kept roots only: first pixel, class and pixel count at the region's index
//   5. insert           one read of both index rasters; a run of equal keys (index_a << 32 | index_b) inside a wave is
//                       one insertion by its first lane: linear probing from a multiplicative hash, a 64-bit atomicCAS
//                       on the key slot, a 64-bit atomicAdd of the run length on the count slot.  The probe loop is
//                       bounded by the capacity; a lane that exhausts it raises the overflow flag and leaves.
//   6. compaction       occupied slots take their output position from one counter, one atomic per wave
// Separate launches order the stages; no grid-wide barrier, no spinning, every loop bound fixed on the host.
#include "ffa_common.h"
#include "ffa_ccl.h"
#include "ffa_workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int kItems = 16;  // pixels per thread in the scan kernels: a block covers kChunk consecutive pixels
constexpr int kChunk = kT * kItems;
constexpr int kWaves = kT / 64;
constexpr u64 kEmpty = ~0ull;  // the key of a free slot; a real key has index_a < 2^30 in its upper half

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ u64 lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

__device__ __forceinline__ bool kept_root(const int* __restrict__ L, const int* __restrict__ cnt, int minp, int p) {
  return L[p] == p && cnt[p] >= minp;
}

// ---- 2. region index: exclusive scan of the kept-root flags --------------------------------------------------------

__global__ __launch_bounds__(kT) void block_sums_kernel(int N, const int* __restrict__ L, const int* __restrict__ cnt,
                                                        int minp, int* __restrict__ bsum) {
  __shared__ int part[kWaves];
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  int n = 0;
  for (int k = 0; k < kItems; ++k) {
    const long long q = base + (long long)k * kT;
    if (q < N && kept_root(L, cnt, minp, (int)q)) ++n;
  }
  n = wave_sum(n);
  if (lane_id() == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kWaves; ++w) s += part[w];
    bsum[blockIdx.x] = s;
  }
}

// one block: bsum[nb] becomes its exclusive scan, *total the sum (the number of regions)
__global__ __launch_bounds__(kT) void scan_blocks_kernel(int nb, int* __restrict__ bsum, long long* __restrict__ total) {
  __shared__ int wtot[kWaves];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nb; base += kT) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wtot[w];
      all += wtot[w];
    }
    if (i < nb) bsum[i] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

// S[root] = number of kept roots before it, for the kept roots only
__global__ __launch_bounds__(kT) void index_kernel(int N, const int* __restrict__ L, const int* __restrict__ cnt,
                                                   int minp, const int* __restrict__ bsum, int* __restrict__ S) {
  __shared__ int wt[kItems * kWaves];  // kept roots per (pass, wave), then their exclusive scan
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  unsigned int flags = 0;
  int pre[kItems];
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const long long q = base + (long long)k * kT;
    const bool f = q < N && kept_root(L, cnt, minp, (int)q);
    const u64 b = __ballot(f);
    pre[k] = __builtin_popcountll(b & lanes_below(lane));
    flags |= f ? 1u << k : 0u;
    if (lane == 0) wt[k * kWaves + wave] = __builtin_popcountll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < kItems * kWaves; ++i) {
      const int v = wt[i];
      wt[i] = run;
      run += v;
    }
  }
  __syncthreads();
  const int b0 = bsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    if (flags >> k & 1u) S[base + (long long)k * kT] = b0 + wt[k * kWaves + wave] + pre[k];
  }
}

// ---- 3. labels -> region indices, in place ---------------------------------------------------------------------------
// Thread p alone reads and writes L[p]; of other pixels it reads cnt and S, which nothing writes here.
__global__ __launch_bounds__(kT) void relabel_kernel(int N, const uint8_t* __restrict__ cls, int* L,
                                                     const int* __restrict__ cnt, int minp, const int* __restrict__ S,
                                                     uint8_t* __restrict__ root_class) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= N) return;
  const int lab = L[p];
  int r = -1;
  if (lab >= 0 && cnt[lab] >= minp) r = S[lab];
  if (lab == p && r >= 0) root_class[p] = cls[p];
  L[p] = r;
}

// the pair bound: pixels with a pair whose left and upper neighbours have none or another one; one atomic per wave
__global__ __launch_bounds__(kT) void heads_kernel(int N, int W, const int* __restrict__ Ra, const int* __restrict__ Rb,
                                                   u64* __restrict__ q_out) {
  const int p = blockIdx.x * kT + threadIdx.x;  // no early exit: the ballot needs whole waves
  const bool in = p < N;
  const int ra = in ? Ra[p] : -1, rb = in ? Rb[p] : -1;
  bool head = ra >= 0 && rb >= 0;
  if (head && p % W > 0 && Ra[p - 1] == ra && Rb[p - 1] == rb) head = false;
  if (head && p >= W && Ra[p - W] == ra && Rb[p - W] == rb) head = false;
  const u64 b = __ballot(head);
  if (lane_id() == 0 && b) atomicAdd(q_out, (u64)__builtin_popcountll(b));
}

// ---- 4. region tables ---------------------------------------------------------------------------------------------------
// After relabel_kernel a kept root is a pixel with an index and a count: count_kernel left counts on roots only.
__global__ __launch_bounds__(kT) void tables_kernel(int N, int P, const int* __restrict__ R, const int* __restrict__ cnt,
                                                    const uint8_t* __restrict__ root_class, int32_t* __restrict__ first,
                                                    int32_t* __restrict__ cls, int64_t* __restrict__ pixels) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= N) return;
  const int r = R[p];
  if (r < 0 || r >= P || cnt[p] <= 0) return;
  first[r] = p;
  cls[r] = root_class[p];
  pixels[r] = cnt[p];
}

// ---- 5. insert ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void insert_kernel(int N, const int* __restrict__ Ra, const int* __restrict__ Rb,
                                                    u64* keys, u64* counts, u64 cap, int shift, u64* overflow) {
  const int p = blockIdx.x * kT + threadIdx.x;  // no early exit: the shuffles need whole waves
  const bool in = p < N;
  const int ra = in ? Ra[p] : -1, rb = in ? Rb[p] : -1;
  const bool has = ra >= 0 && rb >= 0;
  const int ka = has ? ra : -1, kb = has ? rb : -1;
  const int lane = lane_id();
  const int pa = __shfl_up(ka, 1), pb = __shfl_up(kb, 1);
  const bool head = lane == 0 || pa != ka || pb != kb;
  const u64 heads = __ballot(head);
  if (!(head && has)) return;
  const u64 len = (u64)(run_end(heads, lane) - lane);
  const u64 key = ((u64)(unsigned int)ra << 32) | (u64)(unsigned int)rb;
  const u64 mask = cap - 1;
  u64 h = (key * 0x9E3779B97F4A7C15ull) >> shift;
  for (u64 step = 0; step < cap; ++step) {
    const u64 old = atomicCAS(&keys[h], kEmpty, key);
    if (old == kEmpty || old == key) {
      atomicAdd(&counts[h], len);
      return;
    }
    h = (h + 1) & mask;
  }
  atomicOr(overflow, 1ull);  // the table is full: cap >= 2 * Q rules that out on correct code
}

// ---- 6. compaction ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void compact_kernel(u64 cap, const u64* __restrict__ keys, const u64* __restrict__ counts,
                                                     u64 Q, u64* n_pairs, int32_t* __restrict__ pair_a,
                                                     int32_t* __restrict__ pair_b, int64_t* __restrict__ pair_pixels) {
  const u64 i = (u64)blockIdx.x * kT + threadIdx.x;  // no early exit: the ballot needs whole waves
  const u64 key = i < cap ? keys[i] : kEmpty;
  const bool live = key != kEmpty;
  const u64 b = __ballot(live);
  if (!b) return;
  const int lane = lane_id();
  const int leader = __builtin_ctzll(b);
  u64 base = 0;
  if (lane == leader) base = atomicAdd(n_pairs, (u64)__builtin_popcountll(b));
  base = __shfl(base, leader, 64);
  if (!live) return;
  const u64 pos = base + (u64)__builtin_popcountll(b & lanes_below(lane));
  if (pos >= Q) return;  // more pairs than heads cannot be: the count is still reported, nothing is written past the end
  pair_a[pos] = (int32_t)(key >> 32);
  pair_b[pos] = (int32_t)(key & 0xffffffffull);
  pair_pixels[pos] = (int64_t)counts[i];
}

// ---- host side ----------------------------------------------------------------------------------------------------------

struct Side {
  int *R, *cnt;  // labels, after relabel_kernel region indices; pixel counts on the roots
  uint8_t* root_class;
};

struct Arrays {
  long long N;
  int nb;  // scan blocks
  Side a, b;
  int *S, *bsum;
};

long long carve(void* ws, int H, int W, Arrays* a) {
  const long long N = (long long)H * W;
  if (H < 1 || W < 1 || N >= (1ll << 30)) return -1;
  a->N = N;
  a->nb = (int)((N + kChunk - 1) / kChunk);
  ffa_carver c{ws};
  for (Side* s : {&a->a, &a->b}) {
    c.take(s->R, N);
    c.take(s->cnt, N);
    c.take(s->root_class, N);
  }
  c.take(a->S, N);
  c.take(a->bsum, a->nb);
  return c.off;
}

int clamp_min_pixels(long long min_pixels, long long N) {
  return (int)(min_pixels < 1 ? 1 : (min_pixels > N + 1 ? N + 1 : min_pixels));
}

void index_side(const Arrays& a, const Side& s, const uint8_t* classes, int H, int W, int background, int minp,
                long long* total, hipStream_t st) {
  const int N = (int)a.N, gN = (N + kT - 1) / kT;
  ccl_label_and_count(classes, H, W, background, s.R, s.cnt, st);
  hipLaunchKernelGGL(block_sums_kernel, dim3(a.nb), dim3(kT), 0, st, N, s.R, s.cnt, minp, a.bsum);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kT), 0, st, a.nb, a.bsum, total);
  hipLaunchKernelGGL(index_kernel, dim3(a.nb), dim3(kT), 0, st, N, s.R, s.cnt, minp, a.bsum, a.S);
  hipLaunchKernelGGL(relabel_kernel, dim3(gN), dim3(kT), 0, st, N, classes, s.R, s.cnt, minp, a.S, s.root_class);
}

// capacity of the hash table for the pair bound Q: the smallest power of two >= max(2 * Q, 64); 0 beyond Q < 2^30
u64 table_capacity(long long Q, int* log2cap) {
  if (Q < 0 || Q >= (1ll << 30)) return 0;
  const u64 want = 2 * (u64)Q > 64 ? 2 * (u64)Q : 64;
  int lg = 6;
  while ((1ull << lg) < want) ++lg;
  if (log2cap) *log2cap = lg;
  return 1ull << lg;
}

}  // namespace

extern "C" long long ffa_region_overlap_bytes(int H, int W) {
  Arrays a;
  const long long need = carve(nullptr, H, W, &a);
  if (need < 0) {
    ffa_set_error("region_overlap: raster %d x %d outside 1 <= H, W and H * W < 2^30", H, W);
    return FFA_ERR_ARG;
  }
  return need;
}

extern "C" int ffa_region_overlap_count(const uint8_t* a_classes, const uint8_t* b_classes, int H, int W,
                                        int background_a, int background_b, long long min_pixels_a,
                                        long long min_pixels_b, void* ws, long long ws_bytes, long long* counts_dev,
                                        hipStream_t st) {
  Arrays a;
  const long long need = carve(ws, H, W, &a);
  FFA_REQUIRE(need >= 0, "region_overlap: raster %d x %d outside 1 <= H, W and H * W < 2^30", H, W);
  FFA_REQUIRE(a_classes && b_classes && ws && counts_dev, "region_overlap_count: null pointer");
  FFA_REQUIRE(background_a >= -1 && background_a <= 255 && background_b >= -1 && background_b <= 255,
              "region_overlap_count: a background must be -1 (none) or 0..255");
  if (ws_bytes < need) {
    ffa_set_error("region_overlap_count: workspace %lld bytes < %lld", ws_bytes, need);
    return FFA_ERR_WORKSPACE;
  }
  const int N = (int)a.N, gN = (N + kT - 1) / kT;
  FFA_TRY(ffa_zero_async(counts_dev, 4 * sizeof(long long), "region_overlap_count", "the counts", st));
  FFA_TRY(ffa_zero_async(a.a.cnt, 4ll * N, "region_overlap_count", "the pixel counts of a", st));
  FFA_TRY(ffa_zero_async(a.b.cnt, 4ll * N, "region_overlap_count", "the pixel counts of b", st));
  index_side(a, a.a, a_classes, H, W, background_a, clamp_min_pixels(min_pixels_a, a.N), counts_dev, st);
  index_side(a, a.b, b_classes, H, W, background_b, clamp_min_pixels(min_pixels_b, a.N), counts_dev + 1, st);
  hipLaunchKernelGGL(heads_kernel, dim3(gN), dim3(kT), 0, st, N, W, a.a.R, a.b.R,
                     reinterpret_cast<u64*>(counts_dev + 2));
  return ffa_check_launch("region_overlap_count");
}

extern "C" long long ffa_region_overlap_table_bytes(long long Q) {
  const u64 cap = table_capacity(Q, nullptr);
  if (!cap) {
    ffa_set_error("region_overlap: pair bound %lld outside 0 <= Q < 2^30", Q);
    return FFA_ERR_ARG;
  }
  return (long long)(cap * 16);
}

extern "C" int ffa_region_overlap_pairs(const void* ws, long long ws_bytes, int H, int W, long long Pa, long long Pb,
                                        long long Q, void* table, long long table_bytes, int32_t* a_first,
                                        int32_t* a_class, int64_t* a_pixels, int32_t* b_first, int32_t* b_class,
                                        int64_t* b_pixels, int32_t* pair_a, int32_t* pair_b, int64_t* pair_pixels,
                                        long long* counts_dev, hipStream_t st) {
  Arrays a;
  const long long need = carve(const_cast<void*>(ws), H, W, &a);
  FFA_REQUIRE(need >= 0, "region_overlap: raster %d x %d outside 1 <= H, W and H * W < 2^30", H, W);
  FFA_REQUIRE(ws && counts_dev, "region_overlap_pairs: null pointer");
  FFA_REQUIRE(Pa >= 0 && Pa <= a.N && Pb >= 0 && Pb <= a.N && Q >= 0 && Q <= a.N,
              "region_overlap_pairs: counts %lld, %lld, %lld outside 0 .. H * W = %lld", Pa, Pb, Q, a.N);
  FFA_REQUIRE(!Pa || (a_first && a_class && a_pixels), "region_overlap_pairs: null region table of a");
  FFA_REQUIRE(!Pb || (b_first && b_class && b_pixels), "region_overlap_pairs: null region table of b");
  if (ws_bytes < need) {
    ffa_set_error("region_overlap_pairs: workspace %lld bytes < %lld", ws_bytes, need);
    return FFA_ERR_WORKSPACE;
  }
  const int N = (int)a.N, gN = (N + kT - 1) / kT;
  FFA_TRY(ffa_zero_async(counts_dev + 2, 2 * sizeof(long long), "region_overlap_pairs", "the counts", st));
  if (Pa) {
    hipLaunchKernelGGL(tables_kernel, dim3(gN), dim3(kT), 0, st, N, (int)Pa, a.a.R, a.a.cnt, a.a.root_class, a_first,
                       a_class, a_pixels);
  }
  if (Pb) {
    hipLaunchKernelGGL(tables_kernel, dim3(gN), dim3(kT), 0, st, N, (int)Pb, a.b.R, a.b.cnt, a.b.root_class, b_first,
                       b_class, b_pixels);
  }
  if (Pa && Pb && Q) {
    int lg = 0;
    const u64 cap = table_capacity(Q, &lg);
    FFA_REQUIRE(table && pair_a && pair_b && pair_pixels, "region_overlap_pairs: null table or pair output");
    if (table_bytes < (long long)(cap * 16)) {
      ffa_set_error("region_overlap_pairs: table %lld bytes < %lld", table_bytes, (long long)(cap * 16));
      return FFA_ERR_WORKSPACE;
    }
    u64* keys = static_cast<u64*>(table);
    u64* counts = keys + cap;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)(cap * 8), st);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, (size_t)(cap * 8), st);
    if (e != hipSuccess) {
      ffa_set_error("region_overlap_pairs: clearing the table failed: %s", hipGetErrorString(e));
      return (int)e;
    }
    u64* c = reinterpret_cast<u64*>(counts_dev);
    hipLaunchKernelGGL(insert_kernel, dim3(gN), dim3(kT), 0, st, N, a.a.R, a.b.R, keys, counts, cap, 64 - lg, c + 2);
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned int)((cap + kT - 1) / kT)), dim3(kT), 0, st, cap, keys, counts,
                       (u64)Q, c + 3, pair_a, pair_b, pair_pixels);
  }
  return ffa_check_launch("region_overlap_pairs");
}
