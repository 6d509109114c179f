"""vgx_concave_triangulate: a numpy / Python statement of the rule in include/vgx.h -- the canonical edge value, orientation, the
edge-pair test, the clipping loop -- and of what a call writes, the fixtures the CPU and GPU tests share, and the conditions those
fixtures must meet (tests/test_concave_triangulate_cpu.py: the lane code through libvgx_hosttest.so; tests/test_gpu_concave_triangulate.py:
the kernels).

What a REFUSED draw holds, and the fringe and the moved vertices of an AA draw, are vgx_concave_contours' (tests/test_concave_contours_cpu.py
pins them against the reference): `expected` takes that call's output for the same input and states how the triangulating call differs
from it. The rule itself is stated here alone: Python floats are binary64 and Python has no FMA."""
import numpy as np

import raster_model as R

capi = R.capi
F = np.float32
CONCAVE, AA, EO, ENABLE = capi.FILL_CONCAVE, 0x2, capi.FILL_EVEN_ODD, 0x1
TRIANGLES, MULTI, TOO_LONG, NONFINITE = capi.TRI_ROUTE_TRIANGLES, capi.TRI_REFUSED_MULTI, capi.TRI_REFUSED_TOO_LONG, capi.TRI_REFUSED_NONFINITE
DEGENERATE, NOT_SIMPLE, STALLED = capi.TRI_REFUSED_DEGENERATE, capi.TRI_REFUSED_NOT_SIMPLE, capi.TRI_REFUSED_STALLED
CAP = capi.TRIANGULATE_MAX_VERTICES
FILL_KIND = capi.MESH_CONCAVE_FILL_AA << 28


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def c(a, b, p):
    """The canonical edge value of a -> b at p (float32 pairs): a Python float."""
    ax, ay, bx, by, px, py = (float(v) for v in (a[0], a[1], b[0], b[1], p[0], p[1]))
    a_lo = ax < bx or (ax == bx and ay <= by)
    lx, ly, hx, hy = (ax, ay, bx, by) if a_lo else (bx, by, ax, ay)
    g = (hx - lx) * (py - ly) - (hy - ly) * (px - lx)
    if np.asarray(a, dtype=F).tobytes() == np.asarray(b, dtype=F).tobytes():
        return 0.0
    return g if a_lo else -g


def c_many(A, B, P):
    """c over arrays: A, B, P float32 [n, 2] (or one pair each, broadcast): float64 [n]."""
    A, B, P = (np.atleast_2d(np.asarray(v, dtype=F)) for v in (A, B, P))
    n = max(len(A), len(B), len(P))
    A, B, P = (np.broadcast_to(v, (n, 2)) for v in (A, B, P))
    same = (np.ascontiguousarray(A).view(np.uint32) == np.ascontiguousarray(B).view(np.uint32)).all(axis=1)
    a, b, p = A.astype(np.float64), B.astype(np.float64), P.astype(np.float64)
    a_lo = (a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & (a[:, 1] <= b[:, 1]))
    lo, hi = np.where(a_lo[:, None], a, b), np.where(a_lo[:, None], b, a)
    with np.errstate(all="ignore"):
        g = (hi[:, 0] - lo[:, 0]) * (p[:, 1] - lo[:, 1]) - (hi[:, 1] - lo[:, 1]) * (p[:, 0] - lo[:, 0])
    return np.where(same, 0.0, np.where(a_lo, g, -g))


def sign(x):
    return 1 if x > 0 else (-1 if x < 0 else 0)


def orientation(ring):
    V = len(ring)
    k = min(range(V), key=lambda i: (float(ring[i][0]), float(ring[i][1]), i))
    return sign(c(ring[(k - 1) % V], ring[k], ring[(k + 1) % V]))


def in_box(P, A, B):
    lo, hi = np.minimum(A, B), np.maximum(A, B)
    return ((P >= lo) & (P <= hi)).all(axis=1)


def meets(ring, proper_only=False):
    """Does any pair of edges without a common vertex index meet? proper_only: by the first clause alone (strictly opposite signs both
    ways), for the conditions of the fixtures that only the second clause -- a zero value with the endpoint in the other edge's closed
    box -- refuses."""
    V = len(ring)
    nxt = np.roll(ring, -1, axis=0)
    for i in range(V - 2):
        j = np.arange(i + 2, V - 1 if i == 0 else V)
        if j.size == 0:
            continue
        u1, v1, u2, v2 = ring[i][None], nxt[i][None], ring[j], nxt[j]
        a, b = np.sign(c_many(u1, v1, u2)), np.sign(c_many(u1, v1, v2))
        cc, d = np.sign(c_many(u2, v2, u1)), np.sign(c_many(u2, v2, v1))
        U1, V1 = np.broadcast_to(u1, u2.shape), np.broadcast_to(v1, u2.shape)
        hit = (a * b < 0) & (cc * d < 0)
        if not proper_only:
            hit = hit | ((a == 0) & in_box(u2, U1, V1)) | ((b == 0) & in_box(v2, U1, V1)) | ((cc == 0) & in_box(U1, u2, v2)) | ((d == 0) & in_box(V1, u2, v2))
        if hit.any():
            return True
    return False


def clip(ring, s):
    """The clipping loop: the list of triangles (a, b, c) as ring indices, or None when it stalls."""
    V = len(ring)
    prev, nxt = [(i - 1) % V for i in range(V)], [(i + 1) % V for i in range(V)]
    linked = np.ones(V, dtype=bool)
    tris, b, size, misses = [], 0, V, 0
    while size > 3:
        a, cn = prev[b], nxt[b]
        t = s * c(ring[a], ring[b], ring[cn])
        ear = t == 0
        if t > 0:
            others = linked.copy()
            others[[a, b, cn]] = False
            P = ring[others]
            inside = (s * c_many(ring[a], ring[b], P) >= 0) & (s * c_many(ring[b], ring[cn], P) >= 0) & (s * c_many(ring[cn], ring[a], P) >= 0)
            ear = not inside.any()
        if ear:
            tris.append((a, b, cn))
            nxt[a], prev[cn], linked[b] = cn, a, False
            b, size, misses = nxt[cn], size - 1, 0
        else:
            b, misses = cn, misses + 1
            if misses > size:
                return None
    tris.append((prev[b], b, nxt[b]))
    return tris


def ring_route(ring):
    """(route, triangles or None) of ONE ring of at most CAP vertices: float32 [V, 2]."""
    ring = np.ascontiguousarray(ring, dtype=F)
    if not np.isfinite(ring).all():
        return NONFINITE, None
    s = orientation(ring)
    if s == 0:
        return DEGENERATE, None
    if meets(ring):
        return NOT_SIMPLE, None
    tris = clip(ring, s)
    return (STALLED, None) if tris is None else (TRIANGLES, tris)


# ---- what the call writes, from what vgx_concave_contours writes for the same input ----------------------------------------------
def makes(spec):
    contours, flags = spec[0], spec[1]
    return bool(flags & CONCAVE) and not (flags & ENABLE) and len(contours) > 0 and all(len(q) >= 3 for q in contours)


_routes = {}


def expected(specs, cpos, ccol, cidx, cmeshes):
    """specs: (contours, fill_flags, colour, fringe) per draw; c*: the streams and mesh records vgx_concave_contours gives for them.
    Returns (routes [ndraws], pos, color, idx, meshes). A ring's route is computed once per session (the clipping of a long ring takes
    seconds)."""
    routes, pos, col, idx, meshes = [], [], [], [], []
    nv = ni = k = 0
    for d, spec in enumerate(specs):
        contours, flags, color, _ = spec
        if not makes(spec):
            routes.append(0)
            continue
        V = sum(len(q) for q in contours)
        aa = bool(flags & AA)
        mine = cmeshes[k:k + (2 if aa else 1)]
        k += len(mine)
        last = mine[-1]
        ring = cpos[int(last["first_vertex"]):int(last["first_vertex"]) + V]   # the polyline, with AA the moved ring
        if len(contours) > 1:
            route, tris = MULTI, None
        elif V > CAP:
            route, tris = TOO_LONG, None
        else:
            kept = np.ascontiguousarray(ring).tobytes()
            if kept not in _routes:
                _routes[kept] = ring_route(ring)
            route, tris = _routes[kept]
        routes.append(route)
        a, b = int(mine[0]["first_vertex"]), int(mine[0]["first_index"])
        if route != TRIANGLES:
            n, q = sum(int(m["num_vertices"]) for m in mine), sum(int(m["num_indices"]) for m in mine)
            pos.append(cpos[a:a + n]); col.append(ccol[a:a + n]); idx.append(cidx[b:b + q])
            for m in mine:
                meshes.append((nv + int(m["first_vertex"]) - a, ni + int(m["first_index"]) - b, int(m["num_vertices"]), int(m["num_indices"]), d, int(m["subpath_kind"])))
            nv, ni = nv + n, ni + q
            continue
        t = np.array(tris, dtype=np.int64).reshape(-1)
        assert t.size == 3 * (V - 2)
        if aa:   # the fringe mesh as it stands, the moved vertices behind it, the triangles rebased by the fringe's vertices
            pos.append(cpos[a:a + 3 * V]); col.append(ccol[a:a + 3 * V]); idx.append(cidx[b:b + 6 * V]); idx.append((t + 2 * V).astype(np.uint16))
            meshes.append((nv, ni, 3 * V, 6 * V + t.size, d, FILL_KIND))
            nv, ni = nv + 3 * V, ni + 6 * V + t.size
        else:
            pos.append(cpos[a:a + V]); col.append(np.full(V, color, dtype=np.uint32)); idx.append(t.astype(np.uint16))
            meshes.append((nv, ni, V, t.size, d, FILL_KIND))
            nv, ni = nv + V, ni + t.size
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return (np.array(routes, dtype=np.uint32), cat(pos, np.zeros((0, 2), F)), cat(col, np.zeros(0, np.uint32)), cat(idx, np.zeros(0, np.uint16)),
            np.array(meshes, dtype=capi.mesh_dtype))


# ---- fixtures: the smallest shapes at which the code can still go wrong ------------------------------------------------------------
def star(cx, cy, r0, r1, points, phase=0.0):
    a = phase + np.arange(2 * points) * (np.pi / points)
    rad = np.where(np.arange(2 * points) % 2 == 0, r0, r1)
    return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], axis=1).astype(F)


def spiral(n=80, cx=45.0, cy=45.0, turns=2.5, r0=6.0, r1=40.0, width=3.0):
    """A spiral arm of n vertices: out along one side, back along the other. Ears are rare: most candidates contain the next turn."""
    h = n // 2
    t = np.linspace(0.0, 1.0, h)
    ang, rad = turns * 2 * np.pi * t, r0 + (r1 - r0) * t
    outer = np.stack([cx + (rad + width) * np.cos(ang), cy + (rad + width) * np.sin(ang)], axis=1)
    inner = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)[::-1]
    return np.concatenate([outer, inner]).astype(F)


def star_shaped(n, seed, cx=45.0, cy=45.0, r0=12.0, r1=40.0):
    rs = np.random.RandomState(seed)
    ang = np.sort(rs.uniform(0, 2 * np.pi, n))
    rad = rs.uniform(r0, r1, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).astype(F)


BLOB = np.array([(3.3, 4.2), (40.5, 2.7), (84.2, 5.9), (86.6, 44.1), (83.7, 85.3), (50.2, 86.8), (44.6, 70.3), (38.1, 87.4), (4.9, 84.6), (2.2, 40.8),
                 (9.7, 30.4), (2.9, 20.6)], dtype=F)
L_SHAPE = np.array([(4.5, 4.5), (20.5, 4.5), (20.5, 10.5), (11.5, 10.5), (11.5, 21.5), (4.5, 21.5)], dtype=F)
NOTCH = np.array([(6.25, 4.5), (30.25, 4.5), (30.25, 16.5), (20.65, 16.5), (18.25, 9.3), (15.85, 16.5), (6.25, 16.5)], dtype=F)
COMB = np.array([(2, 2), (38, 2), (38, 30), (32, 30), (32, 9), (26, 9), (26, 30), (20, 30), (20, 9), (14, 9), (14, 30), (8, 30), (8, 9), (2, 9)], dtype=F)
COLLINEAR = np.array([(5, 5), (15, 5), (25, 5), (40, 5), (40, 20), (40, 30), (22, 30), (22, 18), (14, 18), (14, 30), (5, 30), (5, 17)], dtype=F)
DART = np.array([(10.25, 8.5), (40.5, 22.75), (10.75, 40.25), (19.5, 23.0)], dtype=F)
TRI3 = np.array([(6.5, 7.25), (33.0, 11.5), (14.75, 30.0)], dtype=F)
BOWTIE = np.array([(4, 6), (34, 30), (34, 6), (4, 30)], dtype=F)
# Rings that touch themselves and cross nowhere: only the zero-in-box clause of the edge-pair test refuses them (ZERO_CLAUSE_ONLY)
TOUCH = np.array([(4, 4), (36, 4), (36, 30), (20, 4), (4, 30)], dtype=F)          # vertex 3 lies inside edge 0 -> 1, reached from the fill's side
TEE = np.array([(4, 4), (30, 4), (30, 30), (4, 30), (4, 22), (30, 17), (4, 12)], dtype=F)   # vertex 5 lies inside the vertical edge 1 -> 2
PINCH = np.array([(4, 4), (20, 16), (36, 4), (36, 28), (20, 16), (4, 28)], dtype=F)          # vertices 1 and 4 are one point
ZERO_CLAUSE_ONLY = ("touch", "tee", "pinch")
FLAT3 = np.array([(4, 4), (12, 8), (20, 12)], dtype=F)                              # three collinear vertices: no orientation
SPIKE = np.array([(4, 4), (40, 4), (40, 14), (22.25, 14), (22, 40), (21.75, 14), (4, 14)], dtype=F)   # its inset by half a fringe of 1 crosses itself
WITH_NAN = np.array([(4, 4), (30, 6), (np.nan, 20), (6, 28)], dtype=F)
SQUARE = np.array([(0, 0), (40, 0), (40, 40), (0, 40)], dtype=F)
# No ear in binary64 although the orientation is not 0 and no edge pair meets: seven nearly collinear vertices whose coordinates lie up
# to 2^33 apart, so that the products inside c round and its signs stop being those of one polygon. Bit patterns, found by
# stalled_ring_search
STALLED_RING = np.array([[3477403122, 3487774008], [1053483605, 1063914106], [1152524439, 1162705779], [1305185399, 1315622588], [1202475874, 1212598824],
                         [1073376634, 1083208030], [3385254217, 3395644419]], dtype=np.uint32).view(F)

COLOR = 0x8040C0F0   # alpha 128: a sample drawn twice, or not at all, shows

# name -> (ring, fill flags beyond CONCAVE, the route the fixture is FOR)
RINGS = {
    "tri3": (TRI3, 0, TRIANGLES), "dart": (DART, 0, TRIANGLES), "l": (L_SHAPE, 0, TRIANGLES), "notch": (NOTCH, 0, TRIANGLES),
    "blob": (BLOB, 0, TRIANGLES), "blob_cw": (BLOB[::-1], 0, TRIANGLES), "l_cw_aa": (L_SHAPE[::-1] * F(2.0), AA, TRIANGLES),
    "comb": (COMB, 0, TRIANGLES), "collinear": (COLLINEAR, 0, TRIANGLES), "spiral": (spiral(), 0, TRIANGLES), "spiral_cw": (spiral()[::-1], EO, TRIANGLES),
    "ring65": (star_shaped(65, 7), 0, TRIANGLES), "ring257": (star_shaped(257, 8), 0, TRIANGLES), "star40_aa": (star(45.2, 44.7, 38.0, 29.0, 20, 0.05), AA, TRIANGLES), "star300": (star(45.3, 44.9, 41.7, 17.2, 150, 0.01), 0, TRIANGLES),
    "blob_aa": (BLOB, AA | EO, TRIANGLES), "notch_aa": (NOTCH * F(2.5), AA, TRIANGLES), "comb_aa": (COMB * F(2.0), AA, TRIANGLES),
    "cap": (star(45.0, 45.0, 44.0, 39.0, CAP // 2, 0.003), 0, TRIANGLES), "cap_plus_1": (star_shaped(CAP + 1, 9), 0, TOO_LONG),
    "bowtie": (BOWTIE, 0, NOT_SIMPLE), "touch": (TOUCH, 0, NOT_SIMPLE), "touch_aa": (TOUCH, AA, NOT_SIMPLE),
    "tee": (TEE, 0, NOT_SIMPLE), "pinch": (PINCH, 0, NOT_SIMPLE), "flat3": (FLAT3, 0, DEGENERATE), "nan": (WITH_NAN, 0, NONFINITE),
    "spike": (SPIKE, 0, TRIANGLES), "spike_aa": (SPIKE, AA, NOT_SIMPLE), "stalled": (STALLED_RING, 0, STALLED),
}


def ring_spec(name, color=COLOR, fringe=1.0):
    ring, flags, _ = RINGS[name]
    return ([ring], CONCAVE | flags, color, fringe)


def mixed_specs():
    """Triangulated and refused draws of every reason but TOO_LONG and STALLED between draws that make nothing."""
    return [
        ring_spec("blob"),                                                         # 0 triangles
        ([SQUARE], ENABLE | AA, 0xFF112233, 1.0),                                  # 1 a convex fill: nothing
        ring_spec("l_cw_aa"),                                                      # 2 triangles behind a fringe
        ([star_shaped(24, 3), star(45.0, 45.0, 9.0, 4.0, 8)[::-1]], CONCAVE | AA, 0x80FF8040, 1.5),   # 3 MULTI: the AA pair
        ([], CONCAVE | AA, 0xFFFFFFFF, 1.0),                                       # 4 no sub-path: nothing
        ring_spec("bowtie"),                                                       # 5 NOT_SIMPLE: one contour mesh
        ([star_shaped(12, 4), SQUARE[:2]], CONCAVE, 0xFF00AA55, 1.0),              # 6 a sub-path of 2 vertices: nothing at all
        ring_spec("spike_aa"),                                                     # 7 NOT_SIMPLE after the inset: the AA pair
        ring_spec("spiral_cw"),                                                    # 8 triangles (the EvenOdd bit has no place in them)
        ring_spec("nan"), ring_spec("flat3"),                                      # 9, 10 NONFINITE, DEGENERATE
        ([SQUARE + F(7)], CONCAVE | ENABLE, 0xFF445566, 1.0),                      # 11 VGX_FILL_ENABLE set: nothing
        ring_spec("ring257"), ring_spec("tri3"), ring_spec("comb_aa"),             # 12 .. 14 triangles
        ([star_shaped(9, 5), star_shaped(7, 6)], CONCAVE | EO, 0xFF00AA55, 1.0),   # 15 MULTI, EvenOdd
        ring_spec("touch"), ring_spec("pinch"),                                    # 16, 17 NOT_SIMPLE by the zero-in-box clause alone
    ]


MIXED_ROUTES = [TRIANGLES, 0, TRIANGLES, MULTI, 0, NOT_SIMPLE, 0, NOT_SIMPLE, TRIANGLES, NONFINITE, DEGENERATE, 0, TRIANGLES, TRIANGLES, TRIANGLES, MULTI, NOT_SIMPLE, NOT_SIMPLE]


def stalled_ring_search(tries=60000, seed=1):
    """How STALLED_RING was found: points t * (u, v) along one line, t over many binades, rounded to binary32 with a relative wobble of
    1e-7, joined as an upper chain forth and a lower chain back. Most such rings are NOT_SIMPLE or are triangulated; about one in
    20 000 passes the orientation and the edge-pair test and then finds no ear. Returns the first such ring."""
    rs = np.random.RandomState(seed)
    for _ in range(tries):
        n = int(rs.randint(4, 8))
        u = rs.uniform(0.3, 1.7, 2)
        t = np.sort(rs.uniform(-1, 1, n) * np.exp2(rs.randint(0, int(rs.randint(0, 40)) + 1, n)))
        wobble = rs.uniform(-1, 1, (n, 2)) * np.exp2(rs.randint(-30, 0))
        pts = (np.outer(t, u) * (1 + wobble * 1e-7)).astype(F)
        ring = pts[list(range(0, n, 2)) + list(range(n - 1 if (n - 1) % 2 else n - 2, 0, -2))]
        if ring_route(ring)[0] == STALLED:
            return ring
    return None
