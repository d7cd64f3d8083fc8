// Topology-preserving polygon simplification (host only): the counterpart of the reference's
// poly.simplify(simplification, preserve_topology=True) (flair_zonal_detection/inference.py:371-372), i.e. shapely /
// JTS TopologyPreservingSimplifier, on the flat polygon arrays of ffa_polygonize_*.
//
// Per polygon, one ring after the other (exterior first), each ring as the closed line v0 .. v(n-1), v0:
//   * Douglas-Peucker: a section i..j is replaced by the shortcut (v_i, v_j) when every vertex strictly between lies
//     within `tolerance` of that segment; otherwise it is split at its farthest vertex and both halves are tried
//   * the shortcut is rejected (and the section split) when it would intersect any other CURRENT segment of the same
//     polygon -- the other rings as they stand (simplified or not yet) and the rest of this ring -- except where it
//     only touches a segment at one of its own two end vertices
//   * a ring keeps at least 4 points counting the closing one (JTS's minimum ring size: 3 distinct vertices), holes
//     are never removed, vertex 0 of every ring stays
// Topology is only preserved inside each polygon; neighbouring polygons may overlap afterwards, as in the reference.
// The candidate tests use a uniform grid over the polygon's bounding box.  Tolerance 0 keeps every vertex.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "ffa_common_host.h"

namespace {

struct Seg {
  double ax, ay, bx, by;
  int ring, idx;  // idx: index of the input segment (>= 0) or -1 for a shortcut
  bool alive;
};

double seg_dist(double px, double py, double ax, double ay, double bx, double by) {
  const double dx = bx - ax, dy = by - ay;
  const double l2 = dx * dx + dy * dy;
  double t = l2 > 0 ? ((px - ax) * dx + (py - ay) * dy) / l2 : 0.0;
  t = t < 0 ? 0 : (t > 1 ? 1 : t);
  const double qx = ax + t * dx - px, qy = ay + t * dy - py;
  return sqrt(qx * qx + qy * qy);
}

int orient(double ax, double ay, double bx, double by, double cx, double cy) {
  const double v = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  return v > 0 ? 1 : (v < 0 ? -1 : 0);
}

bool on_seg(double ax, double ay, double bx, double by, double px, double py) {
  return std::min(ax, bx) <= px && px <= std::max(ax, bx) && std::min(ay, by) <= py && py <= std::max(ay, by);
}

bool same(double ax, double ay, double bx, double by) { return ax == bx && ay == by; }

// true when segment s meets the candidate (p, q) anywhere other than in a single shared end vertex
bool bad_intersection(const Seg& s, double px, double py, double qx, double qy) {
  const int o1 = orient(px, py, qx, qy, s.ax, s.ay), o2 = orient(px, py, qx, qy, s.bx, s.by);
  const int o3 = orient(s.ax, s.ay, s.bx, s.by, px, py), o4 = orient(s.ax, s.ay, s.bx, s.by, qx, qy);
  bool meet = false;
  if (o1 != o2 && o3 != o4 && o1 * o2 <= 0 && o3 * o4 <= 0) meet = true;
  if (o1 == 0 && on_seg(px, py, qx, qy, s.ax, s.ay)) meet = true;
  if (o2 == 0 && on_seg(px, py, qx, qy, s.bx, s.by)) meet = true;
  if (o3 == 0 && on_seg(s.ax, s.ay, s.bx, s.by, px, py)) meet = true;
  if (o4 == 0 && on_seg(s.ax, s.ay, s.bx, s.by, qx, qy)) meet = true;
  if (!meet) return false;
  // allowed: the two segments share exactly one end vertex and are not collinear-overlapping
  const bool shared = same(s.ax, s.ay, px, py) || same(s.ax, s.ay, qx, qy) || same(s.bx, s.by, px, py) ||
                      same(s.bx, s.by, qx, qy);
  if (!shared) return true;
  if (o1 == 0 && o2 == 0) {  // collinear: more than one common point unless they only abut
    const double ux = qx - px, uy = qy - py;
    double t0 = (s.ax - px) * ux + (s.ay - py) * uy, t1 = (s.bx - px) * ux + (s.by - py) * uy;
    const double L = ux * ux + uy * uy;
    if (t0 > t1) std::swap(t0, t1);
    const double lo = std::max(t0, 0.0), hi = std::min(t1, L);
    return hi > lo;
  }
  // a shared end vertex and a second crossing is impossible for two straight non-collinear segments
  return false;
}

struct Grid {
  double x0, y0, cell;
  int nx, ny;
  std::vector<std::vector<int>> cells;
  void init(double minx, double miny, double maxx, double maxy, size_t nseg) {
    const double w = std::max(maxx - minx, 1e-12), h = std::max(maxy - miny, 1e-12);
    const double target = std::max(1.0, (double)nseg / 2.0);
    cell = std::max(sqrt(w * h / target), std::max(w, h) / 1024.0);
    nx = std::max(1, std::min(1024, (int)(w / cell) + 1));
    ny = std::max(1, std::min(1024, (int)(h / cell) + 1));
    x0 = minx;
    y0 = miny;
    cells.assign((size_t)nx * ny, {});
  }
  int cx(double x) const { return std::max(0, std::min(nx - 1, (int)floor((x - x0) / cell))); }
  int cy(double y) const { return std::max(0, std::min(ny - 1, (int)floor((y - y0) / cell))); }
  template <typename F>
  void visit(double ax, double ay, double bx, double by, F f) {
    const int i0 = cx(std::min(ax, bx)), i1 = cx(std::max(ax, bx));
    const int j0 = cy(std::min(ay, by)), j1 = cy(std::max(ay, by));
    for (int j = j0; j <= j1; ++j)
      for (int i = i0; i <= i1; ++i) f(cells[(size_t)j * nx + i]);
  }
  void add(const Seg& s, int id) {
    visit(s.ax, s.ay, s.bx, s.by, [&](std::vector<int>& c) { c.push_back(id); });
  }
};

struct PolySimplifier {
  const double* xy;
  double tol;
  std::vector<Seg> segs;
  std::vector<int> first_seg;  // per ring: index of its first input segment in segs
  std::vector<int> stamp;
  int cur_stamp = 0;
  Grid grid;
  bool use_grid = false;

  bool candidate_ok(int ring, int i, int j, double px, double py, double qx, double qy) {
    const int lo = first_seg[ring] + i, hi = first_seg[ring] + j;  // input segments i .. j-1 are being replaced
    auto test = [&](int id) {
      const Seg& s = segs[id];
      if (!s.alive) return true;
      if (s.idx >= 0 && s.ring == ring && id >= lo && id < hi) return true;
      return !bad_intersection(s, px, py, qx, qy);
    };
    if (!use_grid) {
      for (size_t id = 0; id < segs.size(); ++id)
        if (!test((int)id)) return false;
      return true;
    }
    ++cur_stamp;
    bool ok = true;
    grid.visit(px, py, qx, qy, [&](const std::vector<int>& c) {
      for (int id : c) {
        if (!ok) return;
        if (stamp[id] == cur_stamp) continue;
        stamp[id] = cur_stamp;
        if (!test(id)) ok = false;
      }
    });
    return ok;
  }

  void replace(int ring, int i, int j, double px, double py, double qx, double qy) {
    for (int t = i; t < j; ++t) segs[first_seg[ring] + t].alive = false;
    segs.push_back({px, py, qx, qy, ring, -1, true});
    stamp.push_back(0);
    if (use_grid) grid.add(segs.back(), (int)segs.size() - 1);
  }

  // vertex t of a ring of n vertices, t in 0 .. n (n = vertex 0 again)
  void section(int ring, const double* v, int n, int i, int j, int depth, int* result_size, uint8_t* keep) {
    ++depth;
    if (i + 1 == j) {
      keep[j % n] = 1;
      ++*result_size;
      return;
    }
    bool ok = true;
    if (*result_size < 4 && depth + 1 < 4) ok = false;  // JTS: a ring keeps at least 4 points
    double best = -1.0;
    int far = i + 1;
    const double ax = v[2 * i], ay = v[2 * i + 1], bx = v[2 * (j % n)], by = v[2 * (j % n) + 1];
    for (int t = i + 1; t < j; ++t) {
      const double d = seg_dist(v[2 * t], v[2 * t + 1], ax, ay, bx, by);
      if (d > best) {
        best = d;
        far = t;
      }
    }
    if (best > tol) ok = false;
    if (ok && !candidate_ok(ring, i, j, ax, ay, bx, by)) ok = false;
    if (ok) {
      replace(ring, i, j, ax, ay, bx, by);
      keep[j % n] = 1;
      ++*result_size;
      return;
    }
    section(ring, v, n, i, far, depth, result_size, keep);
    section(ring, v, n, far, j, depth, result_size, keep);
  }

  void run(const int32_t* ring_off, int r0, int r1, uint8_t* keep) {
    segs.clear();
    first_seg.clear();
    double minx = INFINITY, miny = INFINITY, maxx = -INFINITY, maxy = -INFINITY;
    for (int r = r0; r < r1; ++r) {
      const int a = ring_off[r], n = ring_off[r + 1] - a;
      first_seg.push_back((int)segs.size());
      for (int t = 0; t < n; ++t) {
        const double* p = xy + 2 * (a + t);
        const double* q = xy + 2 * (a + (t + 1) % n);
        segs.push_back({p[0], p[1], q[0], q[1], r - r0, t, true});
        minx = std::min(minx, p[0]);
        maxx = std::max(maxx, p[0]);
        miny = std::min(miny, p[1]);
        maxy = std::max(maxy, p[1]);
      }
    }
    stamp.assign(segs.size(), 0);
    cur_stamp = 0;
    use_grid = segs.size() > 64;
    if (use_grid) {
      grid.init(minx, miny, maxx, maxy, segs.size());
      for (size_t id = 0; id < segs.size(); ++id) grid.add(segs[id], (int)id);
    }
    for (int r = r0; r < r1; ++r) {
      const int a = ring_off[r], n = ring_off[r + 1] - a;
      uint8_t* k = keep + a;
      memset(k, 0, n);
      k[0] = 1;
      if (n <= 3) {
        memset(k, 1, n);
        continue;
      }
      int result_size = 1;
      section(r - r0, xy + 2 * a, n, 0, n, 0, &result_size, k);
    }
  }
};

}  // namespace

extern "C" int ffa_polygon_simplify(const double* xy, const int32_t* ring_offsets, const int32_t* poly_ring_offsets,
                                    long long n_polys, double tolerance, int n_threads, uint8_t* keep) {
  if (n_polys < 0 || (n_polys > 0 && !(xy && ring_offsets && poly_ring_offsets && keep)) || !(tolerance >= 0)) {
    ffa_set_error("polygon_simplify: bad arguments");
    return FFA_ERR_ARG;
  }
  if (n_polys == 0) return FFA_OK;
  const long long nv = ring_offsets[poly_ring_offsets[n_polys]];
  if (tolerance == 0) {
    memset(keep, 1, (size_t)nv);
    return FFA_OK;
  }
  n_threads = std::max(1, std::min(16, n_threads));
  std::atomic<long long> next{0};
  auto worker = [&]() {
    PolySimplifier s;
    s.xy = xy;
    s.tol = tolerance;
    for (;;) {
      const long long q0 = next.fetch_add(64);
      if (q0 >= n_polys) break;
      const long long q1 = std::min(n_polys, q0 + 64);
      for (long long q = q0; q < q1; ++q) s.run(ring_offsets, poly_ring_offsets[q], poly_ring_offsets[q + 1], keep);
    }
  };
  if (n_threads == 1 || n_polys < 256) {
    worker();
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; ++t) th.emplace_back(worker);
    for (auto& t : th) t.join();
  }
  return FFA_OK;
}
