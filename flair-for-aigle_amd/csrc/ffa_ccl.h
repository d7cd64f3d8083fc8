// Connected-component labelling of a uint8 class raster, shared by polygonize.hip and sieve.hip.  Everything sits in
// an unnamed namespace: each including file gets its own copy with internal linkage.
//
//   ccl_local_kernel (union-find in LDS on 32 x 32 tiles) -> ccl_merge_kernel (atomicMin unions across tile seams,
//   the larger root links to the smaller) -> ccl_flatten_kernel -> count_kernel (pixel counts on the root, one atomic
//   per wave run of equal labels).
//
// The root of a component is its smallest row-major pixel index, whatever the block schedule, so every later stage
// is deterministic.  Background pixels get -1.  Separate launches, no grid-wide barrier anywhere.
#pragma once
#include "ffa_common.h"

namespace {

constexpr int kT = 256;         // threads per block everywhere
constexpr int kTile = 32;       // CCL tile edge

__device__ __forceinline__ int ld_relaxed(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 1. connected-component labelling ----------------------------------------------------------------------------

__device__ __forceinline__ int lds_find(const int* lab, int x) {
  int y = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (y != x) {
    x = y;
    y = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  return x;
}

__device__ void lds_union(int* lab, int a, int b) {
  bool done = false;
  while (!done) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a < b) {
      const int old = atomicMin(&lab[b], a);
      done = old == b;
      b = old;
    } else if (b < a) {
      const int old = atomicMin(&lab[a], b);
      done = old == a;
      a = old;
    } else {
      done = true;
    }
  }
}

__device__ __forceinline__ int g_find(const int* L, int x) {
  int y = ld_relaxed(&L[x]);
  while (y != x) {
    x = y;
    y = ld_relaxed(&L[x]);
  }
  return x;
}

__device__ void g_union(int* L, int a, int b) {
  bool done = false;
  while (!done) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a < b) {
      const int old = atomicMin(&L[b], a);
      done = old == b;
      b = old;
    } else if (b < a) {
      const int old = atomicMin(&L[a], b);
      done = old == a;
      a = old;
    } else {
      done = true;
    }
  }
}

// one 32 x 32 tile per block, 4 pixels per thread; L[p] = global index of the tile-local root (its smallest pixel)
__global__ __launch_bounds__(kT) void ccl_local_kernel(const uint8_t* __restrict__ cls, int H, int W, int bg,
                                                       int* __restrict__ L) {
  __shared__ int lab[kTile * kTile];
  __shared__ uint8_t c[kTile * kTile];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = 0; k < 4; ++k) {
    const int ly = ty + 8 * k, l = ly * kTile + tx;
    const int y = y0 + ly, x = x0 + tx;
    int v = -1;
    uint8_t cv = 0;
    if (y < H && x < W) {
      cv = cls[(long long)y * W + x];
      if ((int)cv != bg) v = l;
    }
    lab[l] = v;
    c[l] = cv;
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int ly = ty + 8 * k, l = ly * kTile + tx;
    if (lab[l] < 0) continue;
    if (tx > 0 && lab[l - 1] >= 0 && c[l - 1] == c[l]) lds_union(lab, l, l - 1);
    if (ly > 0 && lab[l - kTile] >= 0 && c[l - kTile] == c[l]) lds_union(lab, l, l - kTile);
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int ly = ty + 8 * k, l = ly * kTile + tx;
    const int y = y0 + ly, x = x0 + tx;
    if (y >= H || x >= W) continue;
    int out = -1;
    if (lab[l] >= 0) {
      const int r = lds_find(lab, l);
      out = (y0 + r / kTile) * W + x0 + (r % kTile);
    }
    L[y * W + x] = out;
  }
}

// unions across the tile seams: pixels in the first column / row of a tile with their left / upper neighbour
__global__ __launch_bounds__(kT) void ccl_merge_kernel(const uint8_t* __restrict__ cls, int H, int W, int* L) {
  const int nv = (W - 1) / kTile, nh = (H - 1) / kTile;  // seams
  const long long nvert = (long long)nv * H, total = nvert + (long long)nh * W;
  for (long long i = blockIdx.x * (long long)kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    int p, q;
    if (i < nvert) {
      const int s = (int)(i / H), y = (int)(i % H);
      p = y * W + (s + 1) * kTile;
      q = p - 1;
    } else {
      const long long j = i - nvert;
      const int s = (int)(j / W), x = (int)(j % W);
      p = (s + 1) * kTile * W + x;
      q = p - W;
    }
    if (ld_relaxed(&L[p]) < 0 || ld_relaxed(&L[q]) < 0 || cls[p] != cls[q]) continue;
    g_union(L, p, q);
  }
}

__global__ __launch_bounds__(kT) void ccl_flatten_kernel(int N, int* L) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= N || ld_relaxed(&L[p]) < 0) return;
  L[p] = g_find(L, p);
}

// ---- wave helpers ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// end (exclusive lane index) of the run of equal keys that starts at or before this lane
__device__ __forceinline__ int run_end(unsigned long long heads, int lane) {
  const unsigned long long above = lane == 63 ? 0ull : (heads & (~0ull << (lane + 1)));
  return above ? __builtin_ctzll(above) : 64;
}

// ---- 2. per-component pixel counts ---------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void count_kernel(int N, const int* __restrict__ L, int* __restrict__ cnt) {
  const int p = blockIdx.x * kT + threadIdx.x;
  const int lab = p < N ? L[p] : -2;
  const int lane = lane_id();
  const int prev = __shfl_up(lab, 1);
  const bool head = lane == 0 || prev != lab;
  const unsigned long long heads = __ballot(head);
  if (head && lab >= 0) atomicAdd(&cnt[lab], run_end(heads, lane) - lane);
}

// ---- host side ------------------------------------------------------------------------------------------------------

int grid_for(long long n) {
  long long g = (n + kT - 1) / kT;
  if (g > 8192) g = 8192;
  return g < 1 ? 1 : (int)g;
}

// labels L[N] and pixel counts cnt[N] (zeroed by the caller on the same stream beforehand) of classes[H][W]
void ccl_label_and_count(const uint8_t* classes, int H, int W, int background, int* L, int* cnt, hipStream_t st) {
  const int N = H * W, gN = (N + kT - 1) / kT;
  hipLaunchKernelGGL(ccl_local_kernel, dim3((W + kTile - 1) / kTile, (H + kTile - 1) / kTile), dim3(kT), 0, st,
                     classes, H, W, background, L);
  const long long seams = (long long)((W - 1) / kTile) * H + (long long)((H - 1) / kTile) * W;
  if (seams > 0) hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid_for(seams)), dim3(kT), 0, st, classes, H, W, L);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(gN), dim3(kT), 0, st, N, L);
  hipLaunchKernelGGL(count_kernel, dim3(gN), dim3(kT), 0, st, N, L, cnt);
}

}  // namespace
