"""Topology-preserving simplification (csrc/polygon_simplify.cpp, host ABI only, no GPU)."""
import numpy as np
import pytest


def simplify(rings_per_poly, tol):
    from flairhip import ops
    xy, rvo, pro = [], [0], [0]
    for rings in rings_per_poly:
        for r in rings:
            xy.extend(r)
            rvo.append(rvo[-1] + len(r))
        pro.append(pro[-1] + len(rings))
    xy = np.asarray(xy, float)
    keep = ops.polygon_simplify(xy, rvo, pro, tol)
    out = []
    for q in range(len(rings_per_poly)):
        out.append([xy[rvo[j]:rvo[j + 1]][keep[rvo[j]:rvo[j + 1]]] for j in range(pro[q], pro[q + 1])])
    return out, keep


def seg_dist(p, a, b):
    d = b - a
    t = np.clip(np.dot(p - a, d) / max(np.dot(d, d), 1e-300), 0, 1)
    return np.linalg.norm(a + t * d - p)


def proper_cross(a, b, c, d):
    o = lambda p, q, r: np.sign((q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0]))
    return o(a, b, c) * o(a, b, d) < 0 and o(c, d, a) * o(c, d, b) < 0


def segments(rings):
    return [(r[i], r[(i + 1) % len(r)], k, i) for k, r in enumerate(rings) for i in range(len(r))]


def assert_valid(rings):
    segs = segments(rings)
    for i, (a, b, ka, ia) in enumerate(segs):
        for c, d, kc, ic in segs[i + 1:]:
            assert not proper_cross(a, b, c, d), (a, b, c, d)
    for r in rings:
        assert len(r) >= 3  # 4 points counting the closing one
        assert len({tuple(p) for p in r}) == len(r)


L_SHAPE = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]


def staircase(n, step=0.2):
    """a one-pixel staircase from S = (A, 0) to E = (0, A), A = n * step, closed through F = (-10, -10): every other
    step corner lies on the diagonal S-E, the others step / sqrt 2 (0.1414 m for 0.2 m pixels) off it"""
    pts = [(n, 0)]
    for k in range(n):
        pts += [(n - k, k + 1), (n - k - 1, k + 1)]
    return [(x * step, y * step) for x, y in pts] + [(-10.0, -10.0)]


def test_tolerance_zero_is_the_identity():
    rings = [[np.array(L_SHAPE, float)], [np.array(staircase(7), float)]]
    out, keep = simplify(rings, 0.0)
    assert keep.all()


def test_l_shape_by_hand():
    # closed ring 0..5,0: the whole ring must split (JTS keeps >= 4 points): farthest from v0 is v2 (sqrt 5, first of
    # the two); 0..2 splits again at v1 (still under 4 points); 2..6 splits at v5 (4 / sqrt 5 from the chord v2-v0);
    # 2..5 may now shortcut: v3 and v4 both lie 1 / sqrt 5 = 0.447 from the chord (2, 1)-(0, 2); below that it
    # splits at v3, and 3..5 keeps v4 (1 / sqrt 2 from (1, 1)-(0, 2))
    out, _ = simplify([[np.array(L_SHAPE, float)]], 0.45)
    assert out[0][0].tolist() == [[0, 0], [2, 0], [2, 1], [0, 2]]
    out, _ = simplify([[np.array(L_SHAPE, float)]], 0.44)
    assert out[0][0].tolist() == [list(p) for p in L_SHAPE]


@pytest.mark.parametrize("tol,survive", [(0.14, True), (0.15, False)])
def test_staircase_corners_just_below_and_above_their_offset(tol, survive):
    # from v0 = S the farthest vertex is F (forced split: a ring keeps 4 points); S..F splits at E (farthest from the
    # chord S-F); S..E is then tried against the exact diagonal, 0.1414 from the outer step corners
    n, s = 6, 0.2
    st = np.array(staircase(n, s), float)
    out, keep = simplify([[st]], tol)
    ring = out[0][0].tolist()
    A = n * s
    if survive:  # the diagonal is refused and the first outer corner stays
        assert len(ring) > 3 and [A, s] in ring
    else:        # the whole staircase becomes its diagonal
        assert ring == [[A, 0.0], [0.0, A], [-10.0, -10.0]]


def test_removed_vertices_lie_within_tolerance_of_their_replacement():
    g = np.random.default_rng(0)
    ang = np.sort(g.uniform(0, 2 * np.pi, 300))
    rad = 10 + g.normal(0, 0.3, 300)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    tol = 0.5
    out, keep = simplify([[ring]], tol)
    kept = np.flatnonzero(keep)
    for a, b in zip(kept, np.roll(kept, -1)):
        idx = range(a + 1, b) if b > a else list(range(a + 1, len(ring))) + list(range(0, b))
        for i in idx:
            assert seg_dist(ring[i], ring[a], ring[b]) <= tol + 1e-12
    assert_valid(out[0])


def test_rings_keep_four_points_and_holes_survive():
    ext = np.array([(0, 0), (10, 0), (10, 10), (0, 10)], float)
    hole = np.array([(4, 4), (4, 5), (5, 5), (5, 4)], float)
    out, keep = simplify([[ext, hole]], 100.0)
    assert len(out[0]) == 2 and len(out[0][0]) >= 3 and len(out[0][1]) >= 3
    tiny = np.array([(0, 0), (1, 0), (1, 0.01), (0.5, 0.02), (0, 0.01)], float)
    out, _ = simplify([[tiny]], 100.0)
    assert len(out[0][0]) >= 3


def test_hole_blocking_the_shortcut_keeps_the_polygon_valid():
    # exterior: a shallow notch below y = 0 whose plain DP shortcut (0, 0) -> (10, 0) would cut through the hole
    ext = np.array([(0, 0), (5, -0.9), (10, 0), (10, 10), (0, 10)], float)
    hole = np.array([(4.5, 0.5), (5.5, 0.5), (5.5, -0.3), (4.5, -0.3)], float)  # straddles the chord y = 0
    plain, _ = simplify([[ext]], 1.0)
    assert [5, -0.9] not in plain[0][0].tolist()  # without the hole the notch vertex goes
    out, _ = simplify([[ext, hole]], 1.0)
    assert [5, -0.9] in out[0][0].tolist()  # with it, the shortcut is refused
    assert_valid(out[0])


def test_many_polygons_threaded_equals_serial():
    from flairhip import ops
    g = np.random.default_rng(1)
    xy, rvo, pro = [], [0], [0]
    for q in range(600):
        n = int(g.integers(8, 40))
        ang = np.sort(g.uniform(0, 2 * np.pi, n))
        r = 5 + g.normal(0, 0.5, n)
        xy.extend(np.stack([q * 20 + r * np.cos(ang), r * np.sin(ang)], 1))
        rvo.append(rvo[-1] + n)
        pro.append(pro[-1] + 1)
    xy = np.asarray(xy)
    a = ops.polygon_simplify(xy, rvo, pro, 0.4, 1)
    b = ops.polygon_simplify(xy, rvo, pro, 0.4, 16)
    assert np.array_equal(a, b) and not a.all()
