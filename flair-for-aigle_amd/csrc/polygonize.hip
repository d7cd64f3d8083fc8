// Polygonisation of a uint8 class raster: one polygon per 4-connected component of equal class, pixel-corner
// vertices, holes included -- the polygon set rasterio.features.shapes(mask, mask=mask, connectivity=4) yields per
// class in the reference's raster_to_polygons (flair_zonal_detection/inference.py:359-413), for all classes at once.
//
// Stages (separate launches, no grid-wide barrier anywhere):
//   1. labels      (kernels of stages 1 and 2 live in ffa_ccl.h, shared with sieve.hip)
//                  ccl_local_kernel (union-find in LDS on 32 x 32 tiles) -> ccl_merge_kernel (atomicMin unions across
//                  tile seams, the larger root links to the smaller) -> ccl_flatten_kernel.  The root of a component is
//                  its smallest row-major pixel index, whatever the block schedule, so every later stage is
//                  deterministic.  Background pixels get -1.
//   2. statistics  pixel counts accumulated on the root (one atomic per wave run of equal labels); a component is
//                  kept when count >= min_pixels.
//   3. edges       a pixel side is a boundary edge when the pixel across it is outside the raster or has another
//                  label.  Edge (p, d) runs with its pixel on the LEFT in map coordinates (y up): d = 0 bottom side
//                  heading east, 1 right side heading north, 2 top side heading west, 3 left side heading south.  Edges
//                  of kept components are compacted (exclusive scan of per-pixel edge counts): compact order ==
//                  order of the edge id 4 p + d.  The successor of an edge follows from the 2 x 2 window at its end
//                  corner alone: the pixel ahead-right in the component -> turn right; else ahead-left in it ->
//                  straight; else turn left.  The pinch (ahead-right in, ahead-left out) turns right, i.e. hugs the
//                  non-component pixel behind: the two diagonal component pixels stay apart and every ring is simple.
//   4. rings       cycles of the successor permutation by pointer jumping: min propagation gives the ring id (the
//                  smallest compact edge index on the cycle), then list ranking over predecessors with the cycle
//                  broken at the ring id counts the direction changes before each edge = vertex index.
//   5. layout      signed ring areas (exact, int64, map orientation) -> exterior = the one positive ring per
//                  component; polygons sorted by (class, label) and rings by (polygon, hole, ring id) with stable
//                  8-bit LSD radix passes; offsets by exclusive scans.
//   6. emit        (second ABI call) writes the flat output arrays.
#include "ffa_common.h"
#include "ffa_ccl.h"

namespace {

constexpr int kItems = 16;      // items per thread in scans / radix passes
constexpr int kChunk = kT * kItems;

// ---- 3. boundary edges ---------------------------------------------------------------------------------------------

// pixel across side d: 0 below, 1 right, 2 above, 3 left; forward direction of edge d = across side d + 1
__constant__ int kDR[4] = {1, 0, -1, 0};
__constant__ int kDC[4] = {0, 1, 0, -1};

__device__ __forceinline__ int label_at(const int* L, int H, int W, int r, int c) {
  return (r < 0 || r >= H || c < 0 || c >= W) ? -1 : L[r * W + c];
}

// 4-bit mask of boundary sides of a pixel of a kept component (0 for background / dropped components)
__device__ __forceinline__ int edge_mask(const int* L, const int* cnt, int H, int W, int r, int c, int min_pixels) {
  const int lab = L[r * W + c];
  if (lab < 0 || cnt[lab] < min_pixels) return 0;
  int m = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d)
    if (label_at(L, H, W, r + kDR[d], c + kDC[d]) != lab) m |= 1 << d;
  return m;
}

__global__ __launch_bounds__(kT) void edge_count_kernel(int H, int W, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, int min_pixels,
                                                        int* __restrict__ ecount) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= H * W) return;
  ecount[p] = __builtin_popcount(edge_mask(L, cnt, H, W, p / W, p % W, min_pixels));
}

__device__ __forceinline__ int compact_index(const int* L, const int* cnt, const int* off, int H, int W, int r, int c,
                                             int d, int min_pixels) {
  const int m = edge_mask(L, cnt, H, W, r, c, min_pixels);
  return off[r * W + c] + __builtin_popcount(m & ((1 << d) - 1));
}

// eid[i] = 4 p + d, succ[i], and the min-propagation start state (nxt = succ, mn = i)
__global__ __launch_bounds__(kT) void edge_build_kernel(int H, int W, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, const int* __restrict__ off,
                                                        int min_pixels, int* __restrict__ eid, int* __restrict__ succ,
                                                        int* __restrict__ nxt, int* __restrict__ mn) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= H * W) return;
  const int r = p / W, c = p % W;
  const int m = edge_mask(L, cnt, H, W, r, c, min_pixels);
  if (!m) return;
  const int lab = L[p];
  int i = off[p];
  for (int d = 0; d < 4; ++d) {
    if (!(m & (1 << d))) continue;
    const int fd = (d + 1) & 3;
    const int ar = r + kDR[fd], ac = c + kDC[fd];              // ahead-left pixel
    const int br = ar + kDR[d], bc = ac + kDC[d];              // ahead-right pixel
    int s;
    if (label_at(L, H, W, br, bc) == lab)
      s = compact_index(L, cnt, off, H, W, br, bc, (d + 3) & 3, min_pixels);  // turn right (also the pinch)
    else if (label_at(L, H, W, ar, ac) == lab)
      s = compact_index(L, cnt, off, H, W, ar, ac, d, min_pixels);            // straight on
    else
      s = off[p] + __builtin_popcount(m & ((1 << fd) - 1));                   // turn left, same pixel
    eid[i] = 4 * p + d;
    succ[i] = s;
    nxt[i] = s;
    mn[i] = i;
    ++i;
  }
}

// ---- 4. rings: pointer jumping ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void jump_min_kernel(const int* __restrict__ n_dev, const int* __restrict__ nxt,
                                                      const int* __restrict__ mn, int* __restrict__ nxt2,
                                                      int* __restrict__ mn2) {
  const int n = *n_dev;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const int j = nxt[i];
    nxt2[i] = nxt[j];
    mn2[i] = min(mn[i], mn[j]);
  }
}

__device__ __forceinline__ int edge_dir(int e) { return e & 3; }

// list ranking start state over predecessors, the cycle broken at the ring id: for j = succ(i), P[j] = i and D[j] =
// 1 when the direction changes at the corner between i and j (a vertex at the start corner of j); the ring id edge
// gets P = itself, D = 0
__global__ __launch_bounds__(kT) void rank_init_kernel(const int* __restrict__ n_dev, const int* __restrict__ eid,
                                                       const int* __restrict__ succ, const int* __restrict__ ring,
                                                       int* __restrict__ P, int* __restrict__ D) {
  const int n = *n_dev;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const int j = succ[i];
    if (ring[j] == j) {
      P[j] = j;
      D[j] = 0;
    } else {
      P[j] = i;
      D[j] = edge_dir(eid[i]) != edge_dir(eid[j]) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kT) void jump_sum_kernel(const int* __restrict__ n_dev, const int* __restrict__ P,
                                                      const int* __restrict__ D, int* __restrict__ P2,
                                                      int* __restrict__ D2) {
  const int n = *n_dev;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const int j = P[i];
    P2[i] = P[j];
    D2[i] = D[i] + (j == i ? 0 : D[j]);
  }
}

__global__ __launch_bounds__(kT) void root_flag_kernel(const int* __restrict__ n_dev, const int* __restrict__ ring,
                                                       int* __restrict__ flag) {
  const int n = *n_dev;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) flag[i] = ring[i] == i ? 1 : 0;
}

// start corner (col, row) of edge e = 4 p + d
__device__ __forceinline__ void edge_start(int e, int W, int* x, int* y) {
  const int p = e >> 2, d = e & 3, r = p / W, c = p % W;
  *x = c + (d == 1 || d == 2 ? 1 : 0);
  *y = r + (d == 0 || d == 1 ? 1 : 0);
}

// per ring (ordinal r = ring_ord[ring id]): label, vertex count, whether the ring-id edge starts at a vertex, and
// the doubled signed area in map orientation (sum of dx*y - x*dy over its unit edges, pixel coordinates with y down)
__global__ __launch_bounds__(kT) void ring_info_kernel(const int* __restrict__ n_dev, int W, const int* __restrict__ L,
                                                       const int* __restrict__ eid, const int* __restrict__ succ,
                                                       const int* __restrict__ ring, const int* __restrict__ D,
                                                       const int* __restrict__ ring_ord, int* __restrict__ ring_label,
                                                       int* __restrict__ ring_nv, int* __restrict__ ring_s,
                                                       unsigned long long* __restrict__ ring_area2) {
  const int n = *n_dev;
  const int lane = lane_id();
  // grid-stride over whole waves so that every lane reaches the ballots below
  for (int base = blockIdx.x * kT + (threadIdx.x & ~63); base < n; base += gridDim.x * kT) {
    const int i = base + lane;
    int r = -1;
    long long a = 0;
    if (i < n) {
      const int e = eid[i], root = ring[i];
      r = ring_ord[root];
      int x, y;
      edge_start(e, W, &x, &y);
      const int d = e & 3;
      const int dx = d == 0 ? 1 : (d == 2 ? -1 : 0), dy = d == 3 ? 1 : (d == 1 ? -1 : 0);
      a = (long long)dx * y - (long long)x * dy;
      if (root == i) ring_label[r] = L[e >> 2];
      const int s = succ[i];
      if (s == root) {  // i is the last edge of its ring
        const int emit_end = edge_dir(e) != edge_dir(eid[s]) ? 1 : 0;
        ring_nv[r] = D[i] + emit_end;
        ring_s[r] = emit_end;
      }
    }
    // segmented sum of the area terms over runs of equal ring ordinals in the wave, one atomic per run
    const int prev = __shfl_up(r, 1);
    const bool head = lane == 0 || prev != r;
    const unsigned long long heads = __ballot(head);
    const int end = run_end(heads, lane);
    for (int k = 1; k < 64; k <<= 1) {
      const long long v = __shfl_down(a, k);
      if (lane + k < end) a += v;
    }
    if (head && r >= 0) atomicAdd(&ring_area2[r], (unsigned long long)a);
  }
}

// ---- exclusive scan (int32, in place allowed) --------------------------------------------------------------------

__device__ int block_exclusive_scan(int v, int* total) {
  __shared__ int wsum[kT / 64];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  int x = v;
  for (int k = 1; k < 64; k <<= 1) {
    const int y = __shfl_up(x, k);
    if (lane >= k) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < kT / 64; ++k) {
    if (k < w) before += wsum[k];
    all += wsum[k];
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

__device__ __forceinline__ int scan_n(const int* n_dev, int n_host) { return n_dev ? *n_dev : n_host; }

__global__ __launch_bounds__(kT) void scan_reduce_kernel(const int* __restrict__ in, const int* n_dev, int n_host,
                                                         int* __restrict__ part) {
  const int n = scan_n(n_dev, n_host);
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x * kItems;
  int s = 0;
  for (int k = 0; k < kItems; ++k)
    if (base + k < n) s += in[base + k];
  int total;
  block_exclusive_scan(s, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one block: exclusive scan of the block partials in place, the grand total to *total_out
__global__ __launch_bounds__(kT) void scan_partials_kernel(int* part, int nparts, int* total_out) {
  int carry = 0;
  for (int b0 = 0; b0 < nparts; b0 += kT) {
    const int i = b0 + threadIdx.x;
    const int v = i < nparts ? part[i] : 0;
    int tot;
    const int ex = block_exclusive_scan(v, &tot);
    if (i < nparts) part[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0 && total_out) *total_out = carry;
}

__global__ __launch_bounds__(kT) void scan_apply_kernel(const int* in, const int* n_dev, int n_host,
                                                        const int* __restrict__ part, int* out) {
  const int n = scan_n(n_dev, n_host);
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x * kItems;
  int v[kItems];
  int s = 0;
  for (int k = 0; k < kItems; ++k) {
    v[k] = base + k < n ? in[base + k] : 0;
    s += v[k];
  }
  int total;
  int run = block_exclusive_scan(s, &total) + part[blockIdx.x];
  for (int k = 0; k < kItems; ++k) {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (n_dev == nullptr && base <= n && n < base + kItems) out[n] = run;  // host-sized scans also get out[n] = total
}

// ---- stable 8-bit LSD radix pass (int32 keys, int32 values, count on the device) -----------------------------------

__global__ __launch_bounds__(kT) void radix_hist_kernel(const int* __restrict__ keys, const int* n_dev, int shift,
                                                        int nb, int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int n = *n_dev;
  const long long base = (long long)blockIdx.x * kChunk;
  for (int k = 0; k < kItems; ++k) {
    const long long i = base + k * kT + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
  }
  __syncthreads();
  hist[threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kT) void radix_scatter_kernel(const int* __restrict__ keys, const int* __restrict__ vals,
                                                           const int* n_dev, int shift, int nb,
                                                           const int* __restrict__ hist, int* __restrict__ keys2,
                                                           int* __restrict__ vals2) {
  __shared__ int run[256];
  __shared__ int wcnt[kT / 64][256];
  const int n = *n_dev;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  run[threadIdx.x] = hist[threadIdx.x * nb + blockIdx.x];
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const long long base = (long long)blockIdx.x * kChunk;
  for (int k = 0; k < kItems; ++k) {
    for (int q = 0; q < kT / 64; ++q) wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const long long i = base + k * kT + threadIdx.x;
    const bool valid = i < n;
    const int key = valid ? keys[i] : 0;
    const int dig = (key >> shift) & 255;
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bal = __ballot((dig >> b) & 1);
      peers &= ((dig >> b) & 1) ? bal : ~bal;
    }
    const int rank = __builtin_popcountll(peers & lt);
    if (valid && rank == 0) wcnt[w][dig] = __builtin_popcountll(peers);
    __syncthreads();
    if (valid) {
      int pos = run[dig] + rank;
      for (int q = 0; q < w; ++q) pos += wcnt[q][dig];
      keys2[pos] = key;
      vals2[pos] = vals[i];
    }
    __syncthreads();
    int add = 0;
    for (int q = 0; q < kT / 64; ++q) add += wcnt[q][threadIdx.x];
    run[threadIdx.x] += add;
    __syncthreads();
  }
}

// ---- 5. polygons and rings in output order ---------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void kept_root_flag_kernel(int N, const int* __restrict__ L,
                                                            const int* __restrict__ cnt, int min_pixels,
                                                            int* __restrict__ flag) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= N) return;
  flag[p] = (L[p] == p && cnt[p] >= min_pixels) ? 1 : 0;
}

// compacted kept roots in label order: key = class, value = label
__global__ __launch_bounds__(kT) void comp_list_kernel(int N, const uint8_t* __restrict__ cls,
                                                       const int* __restrict__ L, const int* __restrict__ cnt,
                                                       int min_pixels, const int* __restrict__ ord,
                                                       int* __restrict__ keys, int* __restrict__ vals) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= N || L[p] != p || cnt[p] < min_pixels) return;
  keys[ord[p]] = cls[p];
  vals[ord[p]] = p;
}

__global__ __launch_bounds__(kT) void poly_index_kernel(const int* n_dev, const int* __restrict__ poly_label,
                                                        int* __restrict__ polyidx) {
  const int n = *n_dev;
  for (int q = blockIdx.x * kT + threadIdx.x; q < n; q += gridDim.x * kT) polyidx[poly_label[q]] = q;
}

__global__ __launch_bounds__(kT) void ring_keys_kernel(const int* n_dev, const int* __restrict__ ring_label,
                                                       const unsigned long long* __restrict__ ring_area2,
                                                       const int* __restrict__ polyidx, int* __restrict__ keys,
                                                       int* __restrict__ vals) {
  const int n = *n_dev;
  for (int r = blockIdx.x * kT + threadIdx.x; r < n; r += gridDim.x * kT) {
    const long long a = (long long)ring_area2[r];
    keys[r] = 2 * polyidx[ring_label[r]] + (a > 0 ? 0 : 1);
    vals[r] = r;
  }
}

// sorted ring j = ring ordinal rs[j]: position of each ring, vertex counts in output order, first ring per polygon
__global__ __launch_bounds__(kT) void ring_order_kernel(const int* n_dev, const int* __restrict__ sk,
                                                        const int* __restrict__ rs, const int* __restrict__ ring_nv,
                                                        int* __restrict__ ring_pos, int* __restrict__ nv_sorted,
                                                        int* __restrict__ poly_first) {
  const int n = *n_dev;
  for (int j = blockIdx.x * kT + threadIdx.x; j < n; j += gridDim.x * kT) {
    const int r = rs[j];
    ring_pos[r] = j;
    nv_sorted[j] = ring_nv[r];
    if (!(sk[j] & 1)) poly_first[sk[j] >> 1] = j;
  }
}

struct Counters {
  int edges, rings, polys, verts;
};

__global__ void counts_kernel(const Counters* c, long long* out) {
  if (threadIdx.x == 0) {
    out[0] = c->polys;
    out[1] = c->rings;
    out[2] = c->verts;
    out[3] = c->edges;
  }
}

// ---- 6. emit ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kT) void emit_polys_kernel(int P, int R, const int* __restrict__ poly_cls,
                                                        const int* __restrict__ cnt, const int* __restrict__ poly_label,
                                                        const int* __restrict__ poly_first, int32_t* __restrict__ pcls,
                                                        int64_t* __restrict__ ppix, int32_t* __restrict__ proff) {
  const int q = blockIdx.x * kT + threadIdx.x;
  if (q > P) return;
  if (q == P) {
    proff[P] = R;
    return;
  }
  const int lab = poly_label[q];
  pcls[q] = poly_cls[q];
  ppix[q] = cnt[lab];
  proff[q] = poly_first[q];
}

__global__ __launch_bounds__(kT) void emit_ring_offsets_kernel(int R, int V, const int* __restrict__ voff,
                                                               int32_t* __restrict__ rvoff) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j < R) rvoff[j] = voff[j];
  if (j == R) rvoff[R] = V;
}

// one thread per edge i with a direction change at its end corner: that corner is the start corner of succ(i)
__global__ __launch_bounds__(kT) void emit_vertices_kernel(const int* n_dev, int W, const int* __restrict__ eid,
                                                           const int* __restrict__ succ, const int* __restrict__ ring,
                                                           const int* __restrict__ D, const int* __restrict__ ring_ord,
                                                           const int* __restrict__ ring_s,
                                                           const int* __restrict__ ring_pos,
                                                           const int* __restrict__ voff, int32_t* __restrict__ verts) {
  const int E = *n_dev;
  for (int i = blockIdx.x * kT + threadIdx.x; i < E; i += gridDim.x * kT) {
    const int j = succ[i];
    const int ej = eid[j];
    if (edge_dir(eid[i]) == edge_dir(ej)) continue;
    const int r = ring_ord[ring[i]];
    const int idx = D[j] - 1 + ring_s[r];
    const int v = voff[ring_pos[r]] + idx;
    int x, y;
    edge_start(ej, W, &x, &y);
    verts[2 * v] = x;
    verts[2 * v + 1] = y;
  }
}

// ---- 7. zonal sums (optional third ABI call) --------------------------------------------------------------------------

constexpr int kZSlots = 1024;  // LDS accumulator slots per block (power of two)
constexpr int kZProbes = 4;

// sums[polygon of label lab] += v, nothing for labels of dropped components.  polyidx is only written for kept
// components, so what it holds for lab counts only when poly_label maps that polygon back to lab.
__device__ __forceinline__ void zonal_flush(int lab, unsigned int v, int P, const int* __restrict__ polyidx,
                                            const int* __restrict__ poly_label,
                                            unsigned long long* __restrict__ sums) {
  const int q = polyidx[lab];
  if ((unsigned int)q < (unsigned int)P && poly_label[q] == lab) atomicAdd(&sums[q], (unsigned long long)v);
}

// One block per kChunk consecutive pixels, three levels of partial sums so that a component of millions of pixels
// costs one 64-bit global atomic per block: (1) segmented wave sum over runs of equal labels (the count_kernel
// pattern), (2) the run totals meet in an LDS table keyed by label (open addressing, a few probes; a block sums at
// most kChunk * 255 < 2^32), (3) one global atomic per occupied slot.  A run that finds no slot goes to global memory
// directly (blocks with thousands of tiny components).  Integer adds only: the result does not depend on the order.
__global__ __launch_bounds__(kT) void zonal_sum_kernel(int N, int P, const int* __restrict__ L,
                                                       const uint8_t* __restrict__ values,
                                                       const int* __restrict__ polyidx,
                                                       const int* __restrict__ poly_label,
                                                       unsigned long long* __restrict__ sums) {
  __shared__ int key[kZSlots];
  __shared__ unsigned int acc[kZSlots];
  for (int s = threadIdx.x; s < kZSlots; s += kT) {
    key[s] = -1;
    acc[s] = 0u;
  }
  __syncthreads();
  const int lane = lane_id();
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  for (int k = 0; k < kItems; ++k) {  // every lane runs every iteration: the shuffles and the ballot need whole waves
    const long long p = base + (long long)k * kT;
    const int lab = p < N ? L[p] : -2;
    int v = (p < N && lab >= 0) ? (int)values[p] : 0;
    const int prev = __shfl_up(lab, 1);
    const bool head = lane == 0 || prev != lab;
    const unsigned long long heads = __ballot(head);
    const int end = run_end(heads, lane);
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_down(v, d);
      if (lane + d < end) v += u;
    }
    if (head && lab >= 0) {
      unsigned int h = ((unsigned int)lab * 2654435761u) >> 22;  // 10 bits = kZSlots
      bool placed = false;
      for (int t = 0; t < kZProbes && !placed; ++t) {
        const int old = atomicCAS(&key[h], -1, lab);
        if (old == -1 || old == lab) {
          atomicAdd(&acc[h], (unsigned int)v);
          placed = true;
        }
        h = (h + 1) & (kZSlots - 1);
      }
      if (!placed) zonal_flush(lab, (unsigned int)v, P, polyidx, poly_label, sums);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kZSlots; s += kT)
    if (key[s] >= 0) zonal_flush(key[s], acc[s], P, polyidx, poly_label, sums);
}

// ---- workspace ----------------------------------------------------------------------------------------------------

struct Layout {
  long long N, E, nb_n, nb_e, nb_r;  // pixels, edge bound, scan / radix block counts
  int rounds;
  // offsets in bytes
  long long L, cnt, off, polyidx, poly_label, poly_cls, poly_first, rk0, rv0, rk1, rv1, ring_label, ring_nv, ring_s, ring_pos,
      voff, ring_area2, eid, succ, ring, P0, P1, D0, D1, hist, part, ctr, total;
};

long long align_up(long long v) { return (v + 255) & ~255ll; }

bool make_layout(int H, int W, Layout* lo) {
  if (H < 1 || W < 1) return false;
  const long long N = (long long)H * W;
  if (4 * N >= (1ll << 31)) return false;
  lo->N = N;
  lo->E = 4 * N;
  lo->nb_n = (N + 1 + kChunk - 1) / kChunk;
  lo->nb_e = (lo->E + 1 + kChunk - 1) / kChunk;
  lo->nb_r = (N + kChunk - 1) / kChunk;  // radix passes run over <= N items (components, rings)
  int rounds = 0;
  while ((1ll << rounds) < lo->E) ++rounds;
  lo->rounds = rounds;
  long long o = 0;
  auto take = [&](long long bytes) {
    const long long at = o;
    o += align_up(bytes);
    return at;
  };
  const long long n4 = 4 * (N + 1), e4 = 4 * (lo->E + 1);
  lo->L = take(n4);
  lo->cnt = take(n4);
  lo->off = take(n4);
  lo->polyidx = take(n4);
  lo->poly_label = take(n4);
  lo->poly_cls = take(n4);
  lo->poly_first = take(n4);
  lo->rk0 = take(n4);
  lo->rv0 = take(n4);
  lo->rk1 = take(n4);
  lo->rv1 = take(n4);
  lo->ring_label = take(n4);
  lo->ring_nv = take(n4);
  lo->ring_s = take(n4);
  lo->ring_pos = take(n4);
  lo->voff = take(n4);
  lo->ring_area2 = take(8 * (N + 1));
  lo->eid = take(e4);
  lo->succ = take(e4);
  lo->ring = take(e4);
  lo->P0 = take(e4);
  lo->P1 = take(e4);
  lo->D0 = take(e4);
  lo->D1 = take(e4);
  lo->hist = take(4ll * 256 * lo->nb_r + 4);
  lo->part = take(4ll * (lo->nb_e + lo->nb_n + 256 * lo->nb_r / kChunk + 16));
  lo->ctr = take(sizeof(Counters));
  lo->total = o;
  return true;
}

template <typename T>
T* at(void* ws, long long off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// exclusive scan of n items (n_dev on the device, else n_host, in which case out[n_host] = total as well)
void scan(const int* in, int* out, const int* n_dev, long long n_max, int* part, int* total_dev, hipStream_t st) {
  const int nb = (int)((n_max + 1 + kChunk - 1) / kChunk);
  const int n_host = n_dev ? 0 : (int)n_max;
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kT), 0, st, in, n_dev, n_host, part);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kT), 0, st, part, nb, total_dev);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kT), 0, st, in, n_dev, n_host, part, out);
}

// stable LSD radix sort of (key, value) pairs by the low `bits` key bits; result in (k0, v0)
void radix_sort(int* k0, int* v0, int* k1, int* v1, const int* n_dev, const Layout& lo, int bits, int* hist,
                int* part, hipStream_t st) {
  const int nb = (int)lo.nb_r;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(kT), 0, st, k0, n_dev, shift, nb, hist);
    scan(hist, hist, nullptr, 256ll * nb, part, nullptr, st);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(kT), 0, st, k0, v0, n_dev, shift, nb, hist, k1, v1);
    int* t = k0; k0 = k1; k1 = t;
    t = v0; v0 = v1; v1 = t;
  }
  if ((bits + 7) / 8 % 2 == 1) {  // an odd number of passes left the result in the second buffers
    (void)hipMemcpyAsync(k1, k0, 4 * lo.N, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(v1, v0, 4 * lo.N, hipMemcpyDeviceToDevice, st);
  }
}

int bits_for(long long v) {
  int b = 1;
  while ((1ll << b) <= v) ++b;
  return b;
}

}  // namespace

extern "C" long long ffa_polygonize_workspace_bytes(int H, int W) {
  Layout lo;
  if (!make_layout(H, W, &lo)) {
    ffa_set_error("polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
    return FFA_ERR_ARG;
  }
  return lo.total;
}

extern "C" int ffa_polygonize_label(const uint8_t* classes, int H, int W, int background, long long min_pixels,
                                    void* ws, long long ws_bytes, long long* counts_dev, hipStream_t st) {
  Layout lo;
  FFA_REQUIRE(make_layout(H, W, &lo), "polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
  FFA_REQUIRE(classes && ws && counts_dev, "polygonize_label: null pointer");
  FFA_REQUIRE(background >= -1 && background <= 255, "polygonize_label: background must be -1 (none) or 0..255");
  if (ws_bytes < lo.total) {
    ffa_set_error("polygonize_label: workspace %lld bytes < %lld", ws_bytes, lo.total);
    return FFA_ERR_WORKSPACE;
  }
  const int N = (int)lo.N;
  const int minp = (int)(min_pixels < 1 ? 1 : (min_pixels > lo.N + 1 ? lo.N + 1 : min_pixels));
  int* L = at<int>(ws, lo.L);
  int* cnt = at<int>(ws, lo.cnt);
  int* off = at<int>(ws, lo.off);
  int* eid = at<int>(ws, lo.eid);
  int* succ = at<int>(ws, lo.succ);
  int* ring = at<int>(ws, lo.ring);
  int* P0 = at<int>(ws, lo.P0);
  int* P1 = at<int>(ws, lo.P1);
  int* D0 = at<int>(ws, lo.D0);
  int* D1 = at<int>(ws, lo.D1);
  int* part = at<int>(ws, lo.part);
  int* hist = at<int>(ws, lo.hist);
  Counters* ctr = at<Counters>(ws, lo.ctr);
  const int gN = (N + kT - 1) / kT, gE = grid_for(lo.E);

  (void)hipMemsetAsync(ctr, 0, sizeof(Counters), st);
  (void)hipMemsetAsync(cnt, 0, 4ll * N, st);
  (void)hipMemsetAsync(at<void>(ws, lo.ring_area2), 0, 8ll * (N + 1), st);
  // 1. labels, 2. counts (ffa_ccl.h)
  ccl_label_and_count(classes, H, W, background, L, cnt, st);
  // 3. edges: off = exclusive scan of per-pixel edge counts, total -> ctr->edges
  hipLaunchKernelGGL(edge_count_kernel, dim3(gN), dim3(kT), 0, st, H, W, L, cnt, minp, off);
  scan(off, off, nullptr, N, part, &ctr->edges, st);
  hipLaunchKernelGGL(edge_build_kernel, dim3(gN), dim3(kT), 0, st, H, W, L, cnt, off, minp, eid, succ, P0, D0);
  // 4a. ring id = min compact index on the cycle (P = next pointer, D = running minimum)
  int *pa = P0, *pb = P1, *da = D0, *db = D1;
  for (int k = 0; k < lo.rounds; ++k) {
    hipLaunchKernelGGL(jump_min_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, pa, da, pb, db);
    int* t = pa; pa = pb; pb = t;
    t = da; da = db; db = t;
  }
  (void)hipMemcpyAsync(ring, da, 4 * lo.E, hipMemcpyDeviceToDevice, st);
  // 4b. vertex ranks: D[i] = direction changes on the ring between the ring id edge and edge i
  hipLaunchKernelGGL(rank_init_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, eid, succ, ring, P0, D0);
  pa = P0; pb = P1; da = D0; db = D1;
  for (int k = 0; k < lo.rounds; ++k) {
    hipLaunchKernelGGL(jump_sum_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, pa, da, pb, db);
    int* t = pa; pa = pb; pb = t;
    t = da; da = db; db = t;
  }
  if (da != D0) (void)hipMemcpyAsync(D0, da, 4 * lo.E, hipMemcpyDeviceToDevice, st);  // final ranks live in D0
  // ring ordinals (ring id order) in P0, R -> ctr->rings
  hipLaunchKernelGGL(root_flag_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, ring, P1);
  scan(P1, P0, &ctr->edges, lo.E, part, &ctr->rings, st);
  int* ring_label = at<int>(ws, lo.ring_label);
  int* ring_nv = at<int>(ws, lo.ring_nv);
  int* ring_s = at<int>(ws, lo.ring_s);
  unsigned long long* area2 = at<unsigned long long>(ws, lo.ring_area2);
  hipLaunchKernelGGL(ring_info_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, W, L, eid, succ, ring, D0, P0,
                     ring_label, ring_nv, ring_s, area2);
  // 5. polygons sorted by (class, label)
  int* rk0 = at<int>(ws, lo.rk0);
  int* rv0 = at<int>(ws, lo.rv0);
  int* rk1 = at<int>(ws, lo.rk1);
  int* rv1 = at<int>(ws, lo.rv1);
  int* polyidx = at<int>(ws, lo.polyidx);
  int* poly_label = at<int>(ws, lo.poly_label);
  hipLaunchKernelGGL(kept_root_flag_kernel, dim3(gN), dim3(kT), 0, st, N, L, cnt, minp, rk1);
  scan(rk1, rk1, nullptr, N, part, &ctr->polys, st);
  hipLaunchKernelGGL(comp_list_kernel, dim3(gN), dim3(kT), 0, st, N, classes, L, cnt, minp, rk1, rk0, rv0);
  radix_sort(rk0, rv0, rk1, rv1, &ctr->polys, lo, 8, hist, part, st);
  (void)hipMemcpyAsync(poly_label, rv0, 4 * lo.N, hipMemcpyDeviceToDevice, st);
  (void)hipMemcpyAsync(at<int>(ws, lo.poly_cls), rk0, 4 * lo.N, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(poly_index_kernel, dim3(grid_for(N)), dim3(kT), 0, st, &ctr->polys, poly_label, polyidx);
  // rings sorted by (polygon, hole, ring id)
  hipLaunchKernelGGL(ring_keys_kernel, dim3(grid_for(N)), dim3(kT), 0, st, &ctr->rings, ring_label, area2, polyidx,
                     rk0, rv0);
  radix_sort(rk0, rv0, rk1, rv1, &ctr->rings, lo, bits_for(2 * lo.N), hist, part, st);
  int* ring_pos = at<int>(ws, lo.ring_pos);
  int* voff = at<int>(ws, lo.voff);
  hipLaunchKernelGGL(ring_order_kernel, dim3(grid_for(N)), dim3(kT), 0, st, &ctr->rings, rk0, rv0, ring_nv, ring_pos,
                     rk1, at<int>(ws, lo.poly_first));
  scan(rk1, voff, &ctr->rings, lo.N, part, &ctr->verts, st);
  hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, st, ctr, counts_dev);
  return ffa_check_launch("polygonize_label");
}

extern "C" int ffa_polygonize_emit(const void* ws_c, long long ws_bytes, int H, int W, long long n_polys,
                                   long long n_rings, long long n_vertices, int32_t* poly_class, int64_t* poly_pixels,
                                   int32_t* poly_ring_offsets, int32_t* ring_vertex_offsets, int32_t* vertices,
                                   hipStream_t st) {
  Layout lo;
  FFA_REQUIRE(make_layout(H, W, &lo), "polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
  FFA_REQUIRE(ws_c && ws_bytes >= lo.total, "polygonize_emit: workspace missing or too small");
  FFA_REQUIRE(n_polys >= 0 && n_polys <= lo.N && n_rings >= n_polys && n_rings <= lo.N && n_vertices >= 4 * n_rings &&
                  n_vertices <= lo.E,
              "polygonize_emit: counts (%lld, %lld, %lld) are not those of ffa_polygonize_label", n_polys, n_rings,
              n_vertices);
  FFA_REQUIRE(poly_ring_offsets && ring_vertex_offsets && (n_polys == 0 || (poly_class && poly_pixels && vertices)),
              "polygonize_emit: null output pointer");
  void* ws = const_cast<void*>(ws_c);
  const int P = (int)n_polys, R = (int)n_rings;
  // thread q < P writes polygon q, thread P writes poly_ring_offsets[P] = R
  hipLaunchKernelGGL(emit_polys_kernel, dim3((P + 1 + kT - 1) / kT), dim3(kT), 0, st, P, R, at<int>(ws, lo.poly_cls),
                     at<int>(ws, lo.cnt), at<int>(ws, lo.poly_label), at<int>(ws, lo.poly_first), poly_class,
                     poly_pixels, poly_ring_offsets);
  hipLaunchKernelGGL(emit_ring_offsets_kernel, dim3((R + 1 + kT - 1) / kT), dim3(kT), 0, st, R, (int)n_vertices,
                     at<int>(ws, lo.voff), ring_vertex_offsets);
  if (n_vertices > 0) {
    const Counters* ctr = at<Counters>(ws, lo.ctr);
    hipLaunchKernelGGL(emit_vertices_kernel, dim3(grid_for(lo.E)), dim3(kT), 0, st, &ctr->edges, W, at<int>(ws, lo.eid),
                       at<int>(ws, lo.succ), at<int>(ws, lo.ring), at<int>(ws, lo.D0), at<int>(ws, lo.P0),
                       at<int>(ws, lo.ring_s), at<int>(ws, lo.ring_pos), at<int>(ws, lo.voff), vertices);
  }
  return ffa_check_launch("polygonize_emit");
}

// Reads the workspace ffa_polygonize_label left (labels, polygon index) and nothing ffa_polygonize_emit writes, so it
// may run before or after that call; it writes caller memory only.
extern "C" int ffa_polygonize_zonal_sum_u8(const void* ws_c, long long ws_bytes, int H, int W, const uint8_t* values,
                                           long long n_polys, int64_t* sums, hipStream_t st) {
  Layout lo;
  FFA_REQUIRE(make_layout(H, W, &lo), "polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
  FFA_REQUIRE(ws_c && ws_bytes >= lo.total, "polygonize_zonal_sum_u8: workspace missing or too small");
  FFA_REQUIRE(n_polys >= 0 && n_polys <= lo.N, "polygonize_zonal_sum_u8: %lld polygons are not those of "
              "ffa_polygonize_label", n_polys);
  FFA_REQUIRE(values && (n_polys == 0 || sums), "polygonize_zonal_sum_u8: null pointer");
  if (n_polys == 0) return FFA_OK;
  void* ws = const_cast<void*>(ws_c);
  (void)hipMemsetAsync(sums, 0, 8 * n_polys, st);
  const int N = (int)lo.N;
  hipLaunchKernelGGL(zonal_sum_kernel, dim3((unsigned int)((lo.N + kChunk - 1) / kChunk)), dim3(kT), 0, st, N,
                     (int)n_polys, at<int>(ws, lo.L), values, at<int>(ws, lo.polyidx), at<int>(ws, lo.poly_label),
                     reinterpret_cast<unsigned long long*>(sums));
  return ffa_check_launch("polygonize_zonal_sum_u8");
}
