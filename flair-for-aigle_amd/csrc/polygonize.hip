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
#include "ffa_workspace.h"

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

// eid[i] = 4 p + d, succ[i], and the min-propagation start state (nxt = succ, mn = i).  Edge ids are unsigned: the
// count-sized path takes p up to 2^30 - 1, so 4 p + d needs all 32 bits; compact indices stay below 2^31.
__global__ __launch_bounds__(kT) void edge_build_kernel(int H, int W, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, const int* __restrict__ off,
                                                        int min_pixels, unsigned int* __restrict__ eid,
                                                        int* __restrict__ succ, int* __restrict__ nxt,
                                                        int* __restrict__ mn) {
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
    eid[i] = 4u * (unsigned int)p + (unsigned int)d;
    succ[i] = s;
    nxt[i] = s;
    mn[i] = i;
    ++i;
  }
}

// ---- 4. rings: pointer jumping ---------------------------------------------------------------------------------------

// Grid-stride loops over the edges count unsigned: n may be close to 2^31, where i + gridDim.x * kT no longer fits an
// int but, with at most 2^21 threads in a grid (grid_for), stays far below 2^32.
__device__ __forceinline__ unsigned int grid_first() { return blockIdx.x * kT + threadIdx.x; }
__device__ __forceinline__ unsigned int grid_step() { return gridDim.x * kT; }

__global__ __launch_bounds__(kT) void jump_min_kernel(const int* __restrict__ n_dev, const int* __restrict__ nxt,
                                                      const int* __restrict__ mn, int* __restrict__ nxt2,
                                                      int* __restrict__ mn2) {
  const int n = *n_dev;
  for (unsigned int i = grid_first(); i < (unsigned int)n; i += grid_step()) {
    const int j = nxt[i];
    nxt2[i] = nxt[j];
    mn2[i] = min(mn[i], mn[j]);
  }
}

__device__ __forceinline__ int edge_dir(unsigned int e) { return (int)(e & 3u); }

// list ranking start state over predecessors, the cycle broken at the ring id: for j = succ(i), P[j] = i and D[j] =
// 1 when the direction changes at the corner between i and j (a vertex at the start corner of j); the ring id edge
// gets P = itself, D = 0
__global__ __launch_bounds__(kT) void rank_init_kernel(const int* __restrict__ n_dev,
                                                       const unsigned int* __restrict__ eid,
                                                       const int* __restrict__ succ, const int* __restrict__ ring,
                                                       int* __restrict__ P, int* __restrict__ D) {
  const int n = *n_dev;
  for (unsigned int i = grid_first(); i < (unsigned int)n; i += grid_step()) {
    const int j = succ[i];
    if (ring[j] == j) {
      P[j] = j;
      D[j] = 0;
    } else {
      P[j] = (int)i;
      D[j] = edge_dir(eid[i]) != edge_dir(eid[j]) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kT) void jump_sum_kernel(const int* __restrict__ n_dev, const int* __restrict__ P,
                                                      const int* __restrict__ D, int* __restrict__ P2,
                                                      int* __restrict__ D2) {
  const int n = *n_dev;
  for (unsigned int i = grid_first(); i < (unsigned int)n; i += grid_step()) {
    const int j = P[i];
    P2[i] = P[j];
    D2[i] = D[i] + (j == i ? 0 : D[j]);
  }
}

__global__ __launch_bounds__(kT) void root_flag_kernel(const int* __restrict__ n_dev, const int* __restrict__ ring,
                                                       int* __restrict__ flag) {
  const int n = *n_dev;
  for (unsigned int i = grid_first(); i < (unsigned int)n; i += grid_step()) flag[i] = ring[i] == i ? 1 : 0;
}

// start corner (col, row) of edge e = 4 p + d
__device__ __forceinline__ void edge_start(unsigned int e, int W, int* x, int* y) {
  const int p = (int)(e >> 2), d = (int)(e & 3u), r = p / W, c = p % W;
  *x = c + (d == 1 || d == 2 ? 1 : 0);
  *y = r + (d == 0 || d == 1 ? 1 : 0);
}

// per ring (ordinal r = ring_ord[ring id]): label, vertex count, whether the ring-id edge starts at a vertex, and
// the doubled signed area in map orientation (sum of dx*y - x*dy over its unit edges, pixel coordinates with y down)
__global__ __launch_bounds__(kT) void ring_info_kernel(const int* __restrict__ n_dev, int W, const int* __restrict__ L,
                                                       const unsigned int* __restrict__ eid,
                                                       const int* __restrict__ succ, const int* __restrict__ ring,
                                                       const int* __restrict__ D, const int* __restrict__ ring_ord,
                                                       int* __restrict__ ring_label, int* __restrict__ ring_nv,
                                                       int* __restrict__ ring_s,
                                                       unsigned long long* __restrict__ ring_area2) {
  const int n = *n_dev;
  const int lane = lane_id();
  // grid-stride over whole waves so that every lane reaches the ballots below
  for (unsigned int base = blockIdx.x * kT + (threadIdx.x & ~63u); base < (unsigned int)n; base += grid_step()) {
    const unsigned int i = base + lane;
    int r = -1;
    long long a = 0;
    if (i < n) {
      const unsigned int e = eid[i];
      const int root = ring[i];
      r = ring_ord[root];
      int x, y;
      edge_start(e, W, &x, &y);
      const int d = edge_dir(e);
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

// one block: exclusive scan of the block partials in place, the grand total to *total_out.  *total64_out receives the
// same total accumulated in 64 bits (a partial of per-pixel edge counts is at most 4 * kChunk, so 256 of them fit an
// int): when it is 2^31 or more the 32-bit offsets have wrapped and mean nothing, which the caller finds out from the
// total before it uses them.
__global__ __launch_bounds__(kT) void scan_partials_kernel(int* part, int nparts, int* total_out,
                                                           long long* total64_out) {
  unsigned int carry = 0;
  long long carry64 = 0;
  for (int b0 = 0; b0 < nparts; b0 += kT) {
    const int i = b0 + threadIdx.x;
    const int v = i < nparts ? part[i] : 0;
    int tot;
    const int ex = block_exclusive_scan(v, &tot);
    if (i < nparts) part[i] = (int)(carry + (unsigned int)ex);
    carry += (unsigned int)tot;
    carry64 += tot;
  }
  if (threadIdx.x == 0 && total_out) *total_out = (int)carry;
  if (threadIdx.x == 0 && total64_out) *total64_out = carry64;
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
  for (unsigned int q = grid_first(); q < (unsigned int)n; q += grid_step()) polyidx[poly_label[q]] = (int)q;
}

__global__ __launch_bounds__(kT) void ring_keys_kernel(const int* n_dev, const int* __restrict__ ring_label,
                                                       const unsigned long long* __restrict__ ring_area2,
                                                       const int* __restrict__ polyidx, int* __restrict__ keys,
                                                       int* __restrict__ vals) {
  const int n = *n_dev;
  for (unsigned int r = grid_first(); r < (unsigned int)n; r += grid_step()) {
    const long long a = (long long)ring_area2[r];
    keys[r] = 2 * polyidx[ring_label[r]] + (a > 0 ? 0 : 1);
    vals[r] = (int)r;
  }
}

// sorted ring j = ring ordinal rs[j]: position of each ring, vertex counts in output order, first ring per polygon
__global__ __launch_bounds__(kT) void ring_order_kernel(const int* n_dev, const int* __restrict__ sk,
                                                        const int* __restrict__ rs, const int* __restrict__ ring_nv,
                                                        int* __restrict__ ring_pos, int* __restrict__ nv_sorted,
                                                        int* __restrict__ poly_first) {
  const int n = *n_dev;
  for (unsigned int j = grid_first(); j < (unsigned int)n; j += grid_step()) {
    const int r = rs[j];
    ring_pos[r] = (int)j;
    nv_sorted[j] = ring_nv[r];
    if (!(sk[j] & 1)) poly_first[sk[j] >> 1] = (int)j;
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

// The count-sized path keeps its counters in the pixel workspace: the count phase leaves the edge and polygon counts
// there, the trace phase reads them as the loop bounds and adds rings and vertices.  edges64 is the edge total in
// 64 bits; c.edges is its low half and equal to it whenever the trace phase may run.
struct PixelCounters {
  Counters c;
  long long edges64;
};

__global__ void pixel_counts_kernel(const PixelCounters* c, long long* out) {
  if (threadIdx.x == 0) {
    out[0] = c->edges64;
    out[1] = c->c.polys;
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
__global__ __launch_bounds__(kT) void emit_vertices_kernel(const int* n_dev, int W,
                                                           const unsigned int* __restrict__ eid,
                                                           const int* __restrict__ succ, const int* __restrict__ ring,
                                                           const int* __restrict__ D, const int* __restrict__ ring_ord,
                                                           const int* __restrict__ ring_s,
                                                           const int* __restrict__ ring_pos,
                                                           const int* __restrict__ voff, int32_t* __restrict__ verts) {
  const int E = *n_dev;
  for (unsigned int i = grid_first(); i < (unsigned int)E; i += grid_step()) {
    const int j = succ[i];
    const unsigned int ej = eid[j];
    if (edge_dir(eid[i]) == edge_dir(ej)) continue;
    const int r = ring_ord[ring[i]];
    const int idx = D[j] - 1 + ring_s[r];
    const long long v = (long long)voff[ring_pos[r]] + idx;  // below V < 2^31, so 2 v needs 64 bits
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

// ---- workspaces ---------------------------------------------------------------------------------------------------
// Two ways to give the stages their arrays.  The bound-sized layout (ffa_polygonize_label) sizes everything from the
// raster before anything is known about it: 4 edges per pixel, a ring and a polygon per pixel.  The count-sized
// layouts split the work at the one point where the sizes are known: a pixel workspace for labels, counts, edge
// offsets and the polygon index (ffa_polygonize_count), then, once the host has read the edge and polygon counts, a
// trace workspace sized by those two numbers alone (ffa_polygonize_trace).  Both run the same stages on an Arrays.

struct Arrays {
  long long N, e_cap, r_cap, m_cap;  // pixels; capacity of the edge arrays, the ring arrays, the polygon / radix arrays
  int rounds, nb_r;                  // pointer-jumping rounds, blocks of a radix pass
  int *L, *cnt, *off, *polyidx;      // per pixel
  int* ord;                          // per pixel: scanned kept-root flags (radix buffer rk1 or polyidx, see the layouts)
  int *poly_label, *poly_cls, *poly_first, *rk0, *rv0, *rk1, *rv1;  // m_cap + 1
  int *ring_label, *ring_nv, *ring_s, *ring_pos, *voff;              // r_cap + 1
  unsigned long long* ring_area2;                                    // r_cap + 1
  unsigned int* eid;                                                 // e_cap + 1, as the six below
  int *succ, *ring, *P0, *P1, *D0, *D1;
  int *hist, *part;
  Counters* ctr;
  PixelCounters* pc;  // count-sized path: where the counters live (ctr = &pc->c), else null
};

int rounds_for(long long edges) {
  int rounds = 0;
  while ((1ll << rounds) < edges) ++rounds;
  return rounds;
}

long long chunks(long long n) { return (n + kChunk - 1) / kChunk; }  // blocks of a scan over n items
long long radix_blocks(long long m_cap) { return m_cap > 0 ? chunks(m_cap) : 1; }

// Both layouts are carved by the same two routines (ffa_workspace.h: with a null base the walk only sizes), so an
// array is listed once.  The per-pixel arrays: four int32 arrays of N + 1.
void carve_pixels(ffa_carver& c, long long N, Arrays* a) {
  a->N = N;
  for (int** p : {&a->L, &a->cnt, &a->off, &a->polyidx}) c.take(*p, N + 1);
}

// The edge, ring and polygon arrays for e_cap edges, r_cap rings and m_cap polygon slots (the polygon arrays double
// as radix buffers for the rings), 1 KiB of radix histogram per block of m_cap and part_ints scan partials, whose
// number is the caller's: the layouts differ in it.
void carve_trace(ffa_carver& c, long long e_cap, long long r_cap, long long m_cap, long long part_ints, Arrays* a) {
  a->e_cap = e_cap;
  a->r_cap = r_cap;
  a->m_cap = m_cap;
  a->rounds = rounds_for(e_cap > 2 ? e_cap : 2);
  a->nb_r = (int)radix_blocks(m_cap);
  for (int** p : {&a->poly_label, &a->poly_cls, &a->poly_first, &a->rk0, &a->rv0, &a->rk1, &a->rv1})
    c.take(*p, m_cap + 1);
  for (int** p : {&a->ring_label, &a->ring_nv, &a->ring_s, &a->ring_pos, &a->voff}) c.take(*p, r_cap + 1);
  c.take(a->ring_area2, r_cap + 1);
  c.take(a->eid, e_cap + 1);
  for (int** p : {&a->succ, &a->ring, &a->P0, &a->P1, &a->D0, &a->D1}) c.take(*p, e_cap + 1);
  c.take(a->hist, 256ll * a->nb_r + 1);
  c.take(a->part, part_ints);
}

// Each layout below binds its arrays in ws (null: none) and returns the bytes they take, < 0 beyond its limit.

// Bound-sized: both groups in one buffer, 4 edges, a ring and a polygon per pixel; 4 * H * W < 2^31.
long long carve_bound(void* ws, int H, int W, Arrays* a) {
  const long long N = (long long)H * W;
  if (H < 1 || W < 1 || 4 * N >= (1ll << 31)) return -1;
  *a = {};
  ffa_carver c{ws};
  carve_pixels(c, N, a);
  carve_trace(c, 4 * N, N, N, chunks(4 * N + 1) + chunks(N + 1) + 256 * radix_blocks(N) / kChunk + 16, a);
  a->ord = a->rk1;  // free until the first radix sort, which runs after its only reader (comp_list_kernel)
  c.take(a->ctr, 1);
  return c.off;
}

// Pixel workspace of the count-sized path: the per-pixel arrays, the scan partials and the counters.  With
// N < 2^30 the partials are below 1 MiB, so the total stays within 16 N + 2 MiB.
constexpr long long kCountedMaxPixels = 1ll << 30;
constexpr long long kCountedMaxEdges = (1ll << 31) - 1;  // exclusive

long long carve_count(void* ws_px, int H, int W, Arrays* a) {
  const long long N = (long long)H * W;
  if (H < 1 || W < 1 || N >= kCountedMaxPixels) return -1;
  *a = {};
  ffa_carver c{ws_px};
  carve_pixels(c, N, a);
  // comp_list_kernel reads the ordinals of the kept roots before poly_index_kernel writes the polygon index over
  // them; what stays at the roots of dropped components is at most P and fails zonal_flush's check like any stale
  // value
  a->ord = a->polyidx;
  c.take(a->part, chunks(N + 1) + 16);
  c.take(a->pc, 1);
  a->ctr = a->pc ? &a->pc->c : nullptr;
  return c.off;
}

// Trace workspace, on top of carve_count's Arrays: a function of the two counts only.  A ring has at least 4 edges,
// so E / 4 bounds the rings; the polygon arrays double as radix buffers for the rings, hence max(P, E / 4).  28 bytes
// per edge for the seven edge arrays, 28 per ring, 28 per polygon slot and 1 KiB of histogram per 4096 slots: with
// P <= E / 4 about 42 bytes per edge, and never more than 48 per edge + 64 per polygon + 64 KiB.  The scan partials
// are the trace workspace's from here on.
long long carve_traced(void* ws_tr, long long E, long long P, Arrays* a) {
  if (E < 0 || P < 0 || E >= kCountedMaxEdges || P >= kCountedMaxPixels) return -1;
  const long long r_cap = E / 4, m_cap = P > r_cap ? P : r_cap;
  ffa_carver c{ws_tr};
  carve_trace(c, E, r_cap, m_cap, chunks(E + 1) + chunks(256 * radix_blocks(m_cap) + 1) + 16, a);
  return c.off;
}

// exclusive scan of n items (n_dev on the device, else n_host, in which case out[n_host] = total as well)
void scan(const int* in, int* out, const int* n_dev, long long n_max, int* part, int* total_dev, long long* total64_dev,
          hipStream_t st) {
  const int nb = (int)((n_max + 1 + kChunk - 1) / kChunk);
  const int n_host = n_dev ? 0 : (int)n_max;
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kT), 0, st, in, n_dev, n_host, part);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kT), 0, st, part, nb, total_dev, total64_dev);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kT), 0, st, in, n_dev, n_host, part, out);
}

constexpr const char* kOp = "polygonize";  // names the failed clear or copy of a stage in ffa_last_error()

// stable LSD radix sort of (key, value) pairs by the low `bits` key bits; result in (k0, v0)
int radix_sort(int* k0, int* v0, int* k1, int* v1, const int* n_dev, const Arrays& a, int bits, hipStream_t st) {
  const int nb = a.nb_r;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(kT), 0, st, k0, n_dev, shift, nb, a.hist);
    scan(a.hist, a.hist, nullptr, 256ll * nb, a.part, nullptr, nullptr, st);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(kT), 0, st, k0, v0, n_dev, shift, nb, a.hist, k1, v1);
    int* t = k0; k0 = k1; k1 = t;
    t = v0; v0 = v1; v1 = t;
  }
  if ((bits + 7) / 8 % 2 == 1) {  // an odd number of passes left the result in the second buffers
    FFA_TRY(ffa_copy_async(k1, k0, 4 * a.m_cap, kOp, "the sorted keys", st));
    FFA_TRY(ffa_copy_async(v1, v0, 4 * a.m_cap, kOp, "the sorted values", st));
  }
  return 0;
}

int bits_for(long long v) {
  int b = 1;
  while ((1ll << b) <= v) ++b;
  return b;
}

int clamp_min_pixels(long long min_pixels, long long N) {
  return (int)(min_pixels < 1 ? 1 : (min_pixels > N + 1 ? N + 1 : min_pixels));
}

// The stages come in four groups.  The bound-sized path runs them as label_stages, ring_stages, kept_root_stage,
// order_stages (the kept roots late: edge_build_kernel finds the edge offsets, and comp_list_kernel the ordinals,
// still in the last-level cache); the count-sized path needs both counts first: label_stages and kept_root_stage in
// the count phase, ring_stages and order_stages in the trace phase.

// Stages 1 to 3a: labels, pixel counts, per-pixel edge counts with their exclusive scan (total -> ctr->edges, and in
// 64 bits -> *edges64 when given).
int label_stages(const Arrays& a, const uint8_t* classes, int H, int W, int background, int minp, long long* edges64,
                  hipStream_t st) {
  const int N = (int)a.N, gN = (N + kT - 1) / kT;
  FFA_TRY(ffa_zero_async(a.ctr, sizeof(Counters), kOp, "the counters", st));
  FFA_TRY(ffa_zero_async(a.cnt, 4ll * N, kOp, "the pixel counts", st));
  // 1. labels, 2. counts (ffa_ccl.h)
  ccl_label_and_count(classes, H, W, background, a.L, a.cnt, st);
  // 3. edges: off = exclusive scan of per-pixel edge counts
  hipLaunchKernelGGL(edge_count_kernel, dim3(gN), dim3(kT), 0, st, H, W, a.L, a.cnt, minp, a.off);
  scan(a.off, a.off, nullptr, N, a.part, &a.ctr->edges, edges64, st);
  return 0;
}

// head of stage 5: ordinals of the kept roots in label order, their number -> ctr->polys
void kept_root_stage(const Arrays& a, int minp, hipStream_t st) {
  const int N = (int)a.N, gN = (N + kT - 1) / kT;
  hipLaunchKernelGGL(kept_root_flag_kernel, dim3(gN), dim3(kT), 0, st, N, a.L, a.cnt, minp, a.ord);
  scan(a.ord, a.ord, nullptr, N, a.part, &a.ctr->polys, nullptr, st);
}

// ring_info_kernel accumulates the ring areas: zeroed before ring_stages, on the same stream
int zero_ring_areas(const Arrays& a, hipStream_t st) {
  return ffa_zero_async(a.ring_area2, 8ll * (a.r_cap + 1), kOp, "the ring areas", st);
}

// Stages 3b and 4 on e_cap >= ctr->edges edge slots: successors, ring ids, vertex ranks, per-ring facts.
int ring_stages(const Arrays& a, int H, int W, int minp, hipStream_t st) {
  const int N = (int)a.N, gN = (N + kT - 1) / kT, gE = grid_for(a.e_cap);
  Counters* ctr = a.ctr;
  hipLaunchKernelGGL(edge_build_kernel, dim3(gN), dim3(kT), 0, st, H, W, a.L, a.cnt, a.off, minp, a.eid, a.succ, a.P0,
                     a.D0);
  // 4a. ring id = min compact index on the cycle (P = next pointer, D = running minimum)
  int *pa = a.P0, *pb = a.P1, *da = a.D0, *db = a.D1;
  for (int k = 0; k < a.rounds; ++k) {
    hipLaunchKernelGGL(jump_min_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, pa, da, pb, db);
    int* t = pa; pa = pb; pb = t;
    t = da; da = db; db = t;
  }
  FFA_TRY(ffa_copy_async(a.ring, da, 4 * a.e_cap, kOp, "the ring ids", st));
  // 4b. vertex ranks: D[i] = direction changes on the ring between the ring id edge and edge i
  hipLaunchKernelGGL(rank_init_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, a.eid, a.succ, a.ring, a.P0, a.D0);
  pa = a.P0; pb = a.P1; da = a.D0; db = a.D1;
  for (int k = 0; k < a.rounds; ++k) {
    hipLaunchKernelGGL(jump_sum_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, pa, da, pb, db);
    int* t = pa; pa = pb; pb = t;
    t = da; da = db; db = t;
  }
  if (da != a.D0) FFA_TRY(ffa_copy_async(a.D0, da, 4 * a.e_cap, kOp, "the vertex ranks", st));  // final ranks live in D0
  // ring ordinals (ring id order) in P0, R -> ctr->rings
  hipLaunchKernelGGL(root_flag_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, a.ring, a.P1);
  scan(a.P1, a.P0, &ctr->edges, a.e_cap, a.part, &ctr->rings, nullptr, st);
  hipLaunchKernelGGL(ring_info_kernel, dim3(gE), dim3(kT), 0, st, &ctr->edges, W, a.L, a.eid, a.succ, a.ring, a.D0,
                     a.P0, a.ring_label, a.ring_nv, a.ring_s, a.ring_area2);
  return 0;
}

// Stage 5 after the kept roots: polygons and rings in output order; counts_dev[4] = polygons, rings, vertices, edges.
int order_stages(const Arrays& a, const uint8_t* classes, int minp, long long* counts_dev, hipStream_t st) {
  const int N = (int)a.N, gN = (N + kT - 1) / kT, gM = grid_for(a.m_cap);
  Counters* ctr = a.ctr;
  // polygons sorted by (class, label)
  hipLaunchKernelGGL(comp_list_kernel, dim3(gN), dim3(kT), 0, st, N, classes, a.L, a.cnt, minp, a.ord, a.rk0, a.rv0);
  FFA_TRY(radix_sort(a.rk0, a.rv0, a.rk1, a.rv1, &ctr->polys, a, 8, st));
  FFA_TRY(ffa_copy_async(a.poly_label, a.rv0, 4 * a.m_cap, kOp, "the polygon labels", st));
  FFA_TRY(ffa_copy_async(a.poly_cls, a.rk0, 4 * a.m_cap, kOp, "the polygon classes", st));
  hipLaunchKernelGGL(poly_index_kernel, dim3(gM), dim3(kT), 0, st, &ctr->polys, a.poly_label, a.polyidx);
  // rings sorted by (polygon, hole, ring id); key bits above those of 2 * m_cap are zero in both layouts
  hipLaunchKernelGGL(ring_keys_kernel, dim3(gM), dim3(kT), 0, st, &ctr->rings, a.ring_label, a.ring_area2, a.polyidx,
                     a.rk0, a.rv0);
  FFA_TRY(radix_sort(a.rk0, a.rv0, a.rk1, a.rv1, &ctr->rings, a, bits_for(2 * a.m_cap), st));
  hipLaunchKernelGGL(ring_order_kernel, dim3(gM), dim3(kT), 0, st, &ctr->rings, a.rk0, a.rv0, a.ring_nv, a.ring_pos,
                     a.rk1, a.poly_first);
  scan(a.rk1, a.voff, &ctr->rings, a.r_cap, a.part, &ctr->verts, nullptr, st);
  hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(64), 0, st, ctr, counts_dev);
  return 0;
}

void emit_stages(const Arrays& a, int W, long long n_polys, long long n_rings, long long n_vertices,
                 int32_t* poly_class, int64_t* poly_pixels, int32_t* poly_ring_offsets, int32_t* ring_vertex_offsets,
                 int32_t* vertices, hipStream_t st) {
  const int P = (int)n_polys, R = (int)n_rings;
  // thread q < P writes polygon q, thread P writes poly_ring_offsets[P] = R
  hipLaunchKernelGGL(emit_polys_kernel, dim3((P + 1 + kT - 1) / kT), dim3(kT), 0, st, P, R, a.poly_cls, a.cnt,
                     a.poly_label, a.poly_first, poly_class, poly_pixels, poly_ring_offsets);
  hipLaunchKernelGGL(emit_ring_offsets_kernel, dim3((R + 1 + kT - 1) / kT), dim3(kT), 0, st, R, (int)n_vertices, a.voff,
                     ring_vertex_offsets);
  if (n_vertices > 0)
    hipLaunchKernelGGL(emit_vertices_kernel, dim3(grid_for(a.e_cap)), dim3(kT), 0, st, &a.ctr->edges, W, a.eid, a.succ,
                       a.ring, a.D0, a.P0, a.ring_s, a.ring_pos, a.voff, vertices);
}

int zonal_stage(const Arrays& a, const uint8_t* values, long long n_polys, int64_t* sums, hipStream_t st) {
  FFA_TRY(ffa_zero_async(sums, 8 * n_polys, kOp, "the zonal sums", st));
  hipLaunchKernelGGL(zonal_sum_kernel, dim3((unsigned int)((a.N + kChunk - 1) / kChunk)), dim3(kT), 0, st, (int)a.N,
                     (int)n_polys, a.L, values, a.polyidx, a.poly_label, reinterpret_cast<unsigned long long*>(sums));
  return 0;
}

// What the three bound-sized entry points check first: the raster against the limit, the workspace pointer and its
// size.  A short workspace is FFA_ERR_WORKSPACE from the call that fills it and FFA_ERR_ARG from the two that read it.
int bound_arrays(const char* what, int short_rc, const void* ws, long long ws_bytes, int H, int W, Arrays* a) {
  const long long need = carve_bound(const_cast<void*>(ws), H, W, a);
  FFA_REQUIRE(need >= 0, "polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
  FFA_REQUIRE(ws, "%s: null workspace", what);
  if (ws_bytes < need) {
    ffa_set_error("%s: workspace %lld bytes < %lld", what, ws_bytes, need);
    return short_rc;
  }
  return FFA_OK;
}

// the checks the three calls after the count phase share; binds both workspaces
int counted_arrays(const char* what, const void* ws_px, long long ws_px_bytes, int H, int W, const void* ws_tr,
                   long long ws_tr_bytes, long long n_edges, long long n_polys, Arrays* a) {
  const long long need_px = carve_count(const_cast<void*>(ws_px), H, W, a);
  FFA_REQUIRE(need_px >= 0, "%s: raster %d x %d = %lld pixels outside 1 <= H, W and H * W < 2^30", what, H, W,
              (long long)H * W);
  const long long need_tr = carve_traced(const_cast<void*>(ws_tr), n_edges, n_polys, a);
  FFA_REQUIRE(need_tr >= 0, "%s: %lld boundary edges and %lld polygons outside 0 <= edges < 2^31 - 1 and 0 <= polygons "
              "< 2^30", what, n_edges, n_polys);
  FFA_REQUIRE(n_edges >= 4 && n_polys >= 1 && 4 * n_polys <= n_edges && n_edges <= 4 * a->N,
              "%s: %lld edges and %lld polygons are not counts of ffa_polygonize_count on %d x %d (nothing to trace "
              "when either is 0)", what, n_edges, n_polys, H, W);
  FFA_REQUIRE(ws_px && ws_tr, "%s: null workspace", what);
  if (ws_px_bytes < need_px || ws_tr_bytes < need_tr) {
    ffa_set_error("%s: workspaces of %lld and %lld bytes < %lld and %lld", what, ws_px_bytes, ws_tr_bytes, need_px,
                  need_tr);
    return FFA_ERR_WORKSPACE;
  }
  return FFA_OK;
}

}  // namespace

extern "C" long long ffa_polygonize_workspace_bytes(int H, int W) {
  Arrays a;
  const long long need = carve_bound(nullptr, H, W, &a);
  if (need < 0) {
    ffa_set_error("polygonize: raster %d x %d outside 1 <= H, W and 4 * H * W < 2^31", H, W);
    return FFA_ERR_ARG;
  }
  return need;
}

extern "C" int ffa_polygonize_label(const uint8_t* classes, int H, int W, int background, long long min_pixels,
                                    void* ws, long long ws_bytes, long long* counts_dev, hipStream_t st) {
  FFA_REQUIRE(classes && counts_dev, "polygonize_label: null pointer");
  FFA_REQUIRE(background >= -1 && background <= 255, "polygonize_label: background must be -1 (none) or 0..255");
  Arrays a;
  FFA_TRY(bound_arrays("polygonize_label", FFA_ERR_WORKSPACE, ws, ws_bytes, H, W, &a));
  const int minp = clamp_min_pixels(min_pixels, a.N);
  FFA_TRY(zero_ring_areas(a, st));
  FFA_TRY(label_stages(a, classes, H, W, background, minp, nullptr, st));
  FFA_TRY(ring_stages(a, H, W, minp, st));
  kept_root_stage(a, minp, st);
  FFA_TRY(order_stages(a, classes, minp, counts_dev, st));
  return ffa_check_launch("polygonize_label");
}

extern "C" int ffa_polygonize_emit(const void* ws, long long ws_bytes, int H, int W, long long n_polys,
                                   long long n_rings, long long n_vertices, int32_t* poly_class, int64_t* poly_pixels,
                                   int32_t* poly_ring_offsets, int32_t* ring_vertex_offsets, int32_t* vertices,
                                   hipStream_t st) {
  Arrays a;
  FFA_TRY(bound_arrays("polygonize_emit", FFA_ERR_ARG, ws, ws_bytes, H, W, &a));
  FFA_REQUIRE(n_polys >= 0 && n_polys <= a.N && n_rings >= n_polys && n_rings <= a.N && n_vertices >= 4 * n_rings &&
                  n_vertices <= a.e_cap,
              "polygonize_emit: counts (%lld, %lld, %lld) are not those of ffa_polygonize_label", n_polys, n_rings,
              n_vertices);
  FFA_REQUIRE(poly_ring_offsets && ring_vertex_offsets && (n_polys == 0 || (poly_class && poly_pixels && vertices)),
              "polygonize_emit: null output pointer");
  emit_stages(a, W, n_polys, n_rings, n_vertices, poly_class, poly_pixels, poly_ring_offsets, ring_vertex_offsets,
              vertices, st);
  return ffa_check_launch("polygonize_emit");
}

// Reads the workspace ffa_polygonize_label left (labels, polygon index) and nothing ffa_polygonize_emit writes, so it
// may run before or after that call; it writes caller memory only.
extern "C" int ffa_polygonize_zonal_sum_u8(const void* ws, long long ws_bytes, int H, int W, const uint8_t* values,
                                           long long n_polys, int64_t* sums, hipStream_t st) {
  Arrays a;
  FFA_TRY(bound_arrays("polygonize_zonal_sum_u8", FFA_ERR_ARG, ws, ws_bytes, H, W, &a));
  FFA_REQUIRE(n_polys >= 0 && n_polys <= a.N, "polygonize_zonal_sum_u8: %lld polygons are not those of "
              "ffa_polygonize_label", n_polys);
  FFA_REQUIRE(values && (n_polys == 0 || sums), "polygonize_zonal_sum_u8: null pointer");
  if (n_polys == 0) return FFA_OK;
  FFA_TRY(zonal_stage(a, values, n_polys, sums, st));
  return ffa_check_launch("polygonize_zonal_sum_u8");
}

// ---- the count-sized path ---------------------------------------------------------------------------------------------

extern "C" long long ffa_polygonize_count_bytes(int H, int W) {
  Arrays a;
  const long long need = carve_count(nullptr, H, W, &a);
  if (need < 0) {
    ffa_set_error("polygonize_count: raster %d x %d = %lld pixels outside 1 <= H, W and H * W < 2^30", H, W,
                  (long long)H * W);
    return FFA_ERR_ARG;
  }
  return need;
}

extern "C" int ffa_polygonize_count(const uint8_t* classes, int H, int W, int background, long long min_pixels,
                                    void* ws_px, long long ws_px_bytes, long long* counts_dev, hipStream_t st) {
  Arrays a;
  const long long need = carve_count(ws_px, H, W, &a);
  FFA_REQUIRE(need >= 0, "polygonize_count: raster %d x %d = %lld pixels outside 1 <= H, W and H * W < 2^30", H, W,
              (long long)H * W);
  FFA_REQUIRE(classes && ws_px && counts_dev, "polygonize_count: null pointer");
  FFA_REQUIRE(background >= -1 && background <= 255, "polygonize_count: background must be -1 (none) or 0..255");
  if (ws_px_bytes < need) {
    ffa_set_error("polygonize_count: workspace %lld bytes < %lld", ws_px_bytes, need);
    return FFA_ERR_WORKSPACE;
  }
  FFA_TRY(ffa_zero_async(a.pc, sizeof(PixelCounters), kOp, "the pixel workspace's counters", st));
  const int minp = clamp_min_pixels(min_pixels, a.N);
  FFA_TRY(label_stages(a, classes, H, W, background, minp, &a.pc->edges64, st));
  kept_root_stage(a, minp, st);
  hipLaunchKernelGGL(pixel_counts_kernel, dim3(1), dim3(64), 0, st, a.pc, counts_dev);
  return ffa_check_launch("polygonize_count");
}

extern "C" long long ffa_polygonize_trace_bytes(long long n_edges, long long n_polys) {
  Arrays a;
  const long long need = carve_traced(nullptr, n_edges, n_polys, &a);
  if (need < 0) {
    ffa_set_error("polygonize_trace: %lld boundary edges and %lld polygons outside 0 <= edges < 2^31 - 1 (which also "
                  "keeps vertices < 2^31) and 0 <= polygons < 2^30", n_edges, n_polys);
    return FFA_ERR_ARG;
  }
  return need;
}

extern "C" int ffa_polygonize_trace(const uint8_t* classes, int H, int W, long long min_pixels, void* ws_px,
                                    long long ws_px_bytes, long long n_edges, long long n_polys, void* ws_tr,
                                    long long ws_tr_bytes, long long* counts_dev, hipStream_t st) {
  Arrays a;
  FFA_TRY(counted_arrays("polygonize_trace", ws_px, ws_px_bytes, H, W, ws_tr, ws_tr_bytes, n_edges, n_polys, &a));
  FFA_REQUIRE(classes && counts_dev, "polygonize_trace: null pointer");
  const int minp = clamp_min_pixels(min_pixels, a.N);
  FFA_TRY(zero_ring_areas(a, st));
  FFA_TRY(ring_stages(a, H, W, minp, st));
  FFA_TRY(order_stages(a, classes, minp, counts_dev, st));
  return ffa_check_launch("polygonize_trace");
}

extern "C" int ffa_polygonize_counted_emit(const void* ws_px, long long ws_px_bytes, int H, int W, const void* ws_tr,
                                           long long ws_tr_bytes, long long n_edges, long long n_polys,
                                           long long n_rings, long long n_vertices, int32_t* poly_class,
                                           int64_t* poly_pixels, int32_t* poly_ring_offsets,
                                           int32_t* ring_vertex_offsets, int32_t* vertices, hipStream_t st) {
  Arrays a;
  FFA_TRY(counted_arrays("polygonize_counted_emit", ws_px, ws_px_bytes, H, W, ws_tr, ws_tr_bytes, n_edges, n_polys,
                         &a));
  FFA_REQUIRE(n_rings >= n_polys && n_rings <= a.r_cap && n_vertices >= 4 * n_rings && n_vertices <= n_edges,
              "polygonize_counted_emit: counts (%lld, %lld, %lld) are not those of ffa_polygonize_trace", n_polys,
              n_rings, n_vertices);
  FFA_REQUIRE(poly_class && poly_pixels && poly_ring_offsets && ring_vertex_offsets && vertices,
              "polygonize_counted_emit: null output pointer");
  emit_stages(a, W, n_polys, n_rings, n_vertices, poly_class, poly_pixels, poly_ring_offsets, ring_vertex_offsets,
              vertices, st);
  return ffa_check_launch("polygonize_counted_emit");
}

extern "C" int ffa_polygonize_counted_zonal_sum_u8(const void* ws_px, long long ws_px_bytes, int H, int W,
                                                   const void* ws_tr, long long ws_tr_bytes, long long n_edges,
                                                   const uint8_t* values, long long n_polys, int64_t* sums,
                                                   hipStream_t st) {
  Arrays a;
  FFA_TRY(counted_arrays("polygonize_counted_zonal_sum_u8", ws_px, ws_px_bytes, H, W, ws_tr, ws_tr_bytes, n_edges,
                         n_polys, &a));
  FFA_REQUIRE(values && sums, "polygonize_counted_zonal_sum_u8: null pointer");
  FFA_TRY(zonal_stage(a, values, n_polys, sums, st));
  return ffa_check_launch("polygonize_counted_zonal_sum_u8");
}
