// Sieve filter on a uint8 class raster, in place: 4-connected components of fewer than min_pixels pixels take the
// class of their greatest neighbour (gdal_sieve / rasterio.features.sieve's job, with exact, schedule-independent
// semantics; include/flairhip.h has the definition).  One ABI call = one round:
//   1. labels + counts  the polygoniser's labelling (ffa_ccl.h): root = smallest row-major pixel index, count on it
//   2. vote             one thread per pixel looks at its right and lower sides; a side between components A and B
//                       votes for B at A when A is small and for A at B when B is small: a 64-bit atomicMax of the
//                       packed key (count << 32 | 0x7FFFFFFF - root) on best[root].  Runs of equal (A, B) pairs along
//                       a wave issue one atomic (max is idempotent, so the head of the run alone speaks).
//   3. decide           16 pixels per thread, roots only: new_class[root] = class of best's root when best's key is
//                       greater than the component's own, else the component's class -- read from the classes of
//                       the start of the round, which nothing has modified yet
//   4. apply            classes[p] = new_class[L[p]] where that differs; the two relabel counters get one atomic
//                       per wave
// Separate launches order the stages; no grid-wide barrier, no spinning, every loop bound fixed on the host.
#include "ffa_common.h"
#include "ffa_ccl.h"
#include "ffa_workspace.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 pack_key(int count, int root) {
  return ((u64)(unsigned int)count << 32) | (u64)(0x7FFFFFFFu - (unsigned int)root);
}

// a side between the pixels of labels a and b (valid: both inside the raster): every lane of the wave calls this
__device__ __forceinline__ void vote_side(int a, int b, bool valid, int lane, const int* __restrict__ cnt, int T,
                                          u64* __restrict__ best) {
  const bool live = valid && a >= 0 && b >= 0 && a != b;  // background casts no vote, a == b is no boundary
  const int ka = live ? a : -1, kb = live ? b : -1;
  const int pa = __shfl_up(ka, 1), pb = __shfl_up(kb, 1);
  const bool head = lane == 0 || pa != ka || pb != kb;    // lanes whose pair differs never collapse
  if (head && live) {
    const int ca = cnt[a], cb = cnt[b];
    if (ca < T) atomicMax(&best[a], pack_key(cb, b));
    if (cb < T) atomicMax(&best[b], pack_key(ca, a));
  }
}

__global__ __launch_bounds__(kT) void vote_kernel(int H, int W, const int* __restrict__ L, const int* __restrict__ cnt,
                                                  int T, u64* __restrict__ best) {
  const int N = H * W;
  const int p = blockIdx.x * kT + threadIdx.x;  // no early exit: the shuffles need whole waves
  const bool in = p < N;
  const int lane = lane_id();
  const int a = in ? L[p] : -1;
  const bool has_right = in && (p % W) + 1 < W, has_down = in && p + W < N;
  const int r = has_right ? L[p + 1] : -1;
  const int d = has_down ? L[p + W] : -1;
  vote_side(a, r, has_right, lane, cnt, T, best);
  vote_side(a, d, has_down, lane, cnt, T, best);
}

constexpr int kItems = 16;  // pixels per thread in decide / apply: the counters take one atomic per wave of 1024 pixels
constexpr int kChunk = kT * kItems;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// counts[0] += small components, counts[3] += components (one atomic per wave each)
__global__ __launch_bounds__(kT) void decide_kernel(int N, const uint8_t* __restrict__ cls, const int* __restrict__ L,
                                                    const int* __restrict__ cnt, int T, const u64* __restrict__ best,
                                                    uint8_t* __restrict__ new_class, u64* __restrict__ counts) {
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  int roots = 0, smalls = 0;
  for (int k = 0; k < kItems; ++k) {
    const long long q = base + (long long)k * kT;
    if (q >= N) break;
    const int p = (int)q;
    if (L[p] != p) continue;
    const int c = cnt[p];
    uint8_t nc = cls[p];
    ++roots;
    if (c < T) {
      ++smalls;
      const u64 b = best[p];  // 0 when no neighbour voted: never greater than a key, whose count is >= 1
      if (b > pack_key(c, p)) nc = cls[0x7FFFFFFF - (int)(unsigned int)(b & 0xFFFFFFFFull)];
    }
    new_class[p] = nc;
  }
  roots = wave_sum(roots);
  smalls = wave_sum(smalls);
  if (lane_id() == 0) {
    if (smalls) atomicAdd(&counts[0], (u64)smalls);
    if (roots) atomicAdd(&counts[3], (u64)roots);
  }
}

// counts[1] += relabelled components (their root pixel changed), counts[2] += relabelled pixels
__global__ __launch_bounds__(kT) void apply_kernel(int N, uint8_t* __restrict__ cls, const int* __restrict__ L,
                                                   const uint8_t* __restrict__ new_class, u64* __restrict__ counts) {
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  int changed = 0, roots = 0;
  for (int k = 0; k < kItems; ++k) {
    const long long q = base + (long long)k * kT;
    if (q >= N) break;
    const int p = (int)q;
    const int lab = L[p];
    if (lab < 0) continue;
    const uint8_t nc = new_class[lab];
    if (nc != cls[p]) {
      cls[p] = nc;
      ++changed;
      roots += lab == p ? 1 : 0;
    }
  }
  changed = wave_sum(changed);
  roots = wave_sum(roots);
  if (lane_id() == 0 && changed) {
    atomicAdd(&counts[2], (u64)changed);
    if (roots) atomicAdd(&counts[1], (u64)roots);
  }
}

// The four arrays of a round, carved from ws (null: sized only); the bytes they take, < 0 beyond the limit.
struct Arrays {
  long long N;
  int *L, *cnt;
  u64* best;
  uint8_t* new_class;
};

long long carve(void* ws, int H, int W, Arrays* a) {
  const long long N = (long long)H * W;
  if (H < 1 || W < 1 || 4 * N >= (1ll << 31)) return -1;
  a->N = N;
  ffa_carver c{ws};
  c.take(a->L, N);
  c.take(a->cnt, N);
  c.take(a->best, N);
  c.take(a->new_class, N);
  return c.off;
}

}  // namespace

extern "C" long long ffa_sieve_workspace_bytes(int H, int W) {
  Arrays a;
  const long long need = carve(nullptr, H, W, &a);
  if (need < 0) {
    ffa_set_error("sieve: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
    return FFA_ERR_ARG;
  }
  return need;
}

extern "C" int ffa_sieve_round_u8(uint8_t* classes, int H, int W, int background, long long min_pixels, void* ws,
                                  long long ws_bytes, long long* counts_dev, hipStream_t st) {
  Arrays a;
  const long long need = carve(ws, H, W, &a);
  FFA_REQUIRE(need >= 0, "sieve: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
  FFA_REQUIRE(classes && ws && counts_dev, "sieve_round_u8: null pointer");
  FFA_REQUIRE(background >= -1 && background <= 255, "sieve_round_u8: background must be -1 (none) or 0..255");
  FFA_REQUIRE(min_pixels >= 0, "sieve_round_u8: min_pixels %lld is negative", min_pixels);
  if (ws_bytes < need) {
    ffa_set_error("sieve_round_u8: workspace %lld bytes < %lld", ws_bytes, need);
    return FFA_ERR_WORKSPACE;
  }
  const int N = (int)a.N;
  const int T = (int)(min_pixels > a.N + 1 ? a.N + 1 : min_pixels);
  u64* counts = reinterpret_cast<u64*>(counts_dev);
  const int gN = (N + kT - 1) / kT, gC = (int)((a.N + kChunk - 1) / kChunk);

  FFA_TRY(ffa_zero_async(counts_dev, 4 * sizeof(long long), "sieve_round_u8", "the counters", st));
  FFA_TRY(ffa_zero_async(a.cnt, 4ll * N, "sieve_round_u8", "the pixel counts", st));
  if (T > 1) FFA_TRY(ffa_zero_async(a.best, 8ll * N, "sieve_round_u8", "the votes", st));
  ccl_label_and_count(classes, H, W, background, a.L, a.cnt, st);
  if (T > 1) {  // a component has at least one pixel: below that nothing is small, nothing votes or moves
    hipLaunchKernelGGL(vote_kernel, dim3(gN), dim3(kT), 0, st, H, W, a.L, a.cnt, T, a.best);
  }
  hipLaunchKernelGGL(decide_kernel, dim3(gC), dim3(kT), 0, st, N, classes, a.L, a.cnt, T, a.best, a.new_class, counts);
  if (T > 1) hipLaunchKernelGGL(apply_kernel, dim3(gC), dim3(kT), 0, st, N, classes, a.L, a.new_class, counts);
  return ffa_check_launch("sieve_round_u8");
}
