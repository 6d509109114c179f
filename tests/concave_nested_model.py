"""vgx_concave_triangulate_nested: the rule of include/vgx.h for a draw of several outlines and islands in holes, in numpy / Python over
tests/concave_rings_model.py and tests/concave_triangulate_model.py (imported, untouched): the rings are classified by containment depth
and cut into groups of one even-depth ring with the odd-depth rings directly inside it, and every group is given to the rings model (one
ring: to the single-ring model) AS A DRAW OF ITS OWN, its indices translated back. The lane code and the kernel never form such a draw:
they walk the group's slots inside the whole draw's tables. That the two agree on every fixture is part of what the tests show.

What a call writes; the fixtures the CPU and GPU tests share (tests/test_concave_nested_cpu.py: the lane code;
tests/test_gpu_concave_nested.py: the kernels)."""
import numpy as np

import concave_rings_model as RM
import concave_triangulate_model as TM
from concave_triangulate_model import c_many

capi = TM.capi
F = np.float32
CONCAVE, AA, EO, ENABLE = TM.CONCAVE, TM.AA, TM.EO, TM.ENABLE
TRIANGLES, TOO_LONG, NONFINITE, DEGENERATE, NOT_SIMPLE, STALLED = TM.TRIANGLES, TM.TOO_LONG, TM.NONFINITE, TM.DEGENERATE, TM.NOT_SIMPLE, TM.STALLED
NESTING, NO_BRIDGE = RM.NESTING, RM.NO_BRIDGE
CAP = TM.CAP
FILL_KIND = TM.FILL_KIND
COLOR = TM.COLOR
sq, rev = RM.sq, RM.rev


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def inside_matrix(rings):
    """inside(m_r, r') for every ordered pair of rings at once: bool [S, S], row r = the rings m_r is inside of (the diagonal False)."""
    S = len(rings)
    lens = [len(r) for r in rings]
    pos = np.concatenate(rings)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    ring_of = np.repeat(np.arange(S), lens)
    nxt = np.concatenate([start[r] + (np.arange(lens[r]) + 1) % lens[r] for r in range(S)])
    m = np.array([max(range(start[r], start[r + 1]), key=lambda i: RM.key(pos, i)) for r in range(S)])
    U, W, M = pos, pos[nxt], pos[m]
    straddle = (U[None, :, 1] <= M[:, None, 1]) != (W[None, :, 1] <= M[:, None, 1])   # [S, V]
    ir, iv = np.nonzero(straddle)
    count = np.zeros((S, S), dtype=np.int64)
    if ir.size:
        side = np.sign(c_many(U[iv], W[iv], M[ir])) == np.sign(W[iv, 1].astype(np.float64) - U[iv, 1].astype(np.float64))
        np.add.at(count, (ir[side], ring_of[iv[side]]), 1)
    inside = (count & 1).astype(bool)
    inside[np.arange(S), np.arange(S)] = False
    return inside


def classify(rings, even_odd):
    """(depth [S], outer [S]: the outer ring of every ring's group) or None when the containment is not a forest the rule can use."""
    S = len(rings)
    inside = inside_matrix(rings)
    depth = inside.sum(axis=1)
    sg = [TM.orientation(r) for r in rings]
    outer = np.arange(S)
    for r in range(S):
        if depth[r] == 0:
            continue
        parents = [q for q in np.nonzero(inside[r])[0] if depth[q] == depth[r] - 1]
        if len(parents) != 1:
            return None
        if depth[r] & 1:
            if not even_odd and sg[r] != -sg[parents[0]]:
                return None
            outer[r] = parents[0]
    return depth, outer


def nested_route(rings, even_odd):
    """(route, triangles as vertex triples or None, notes) of a draw of S >= 2 rings. notes: 'groups' = the sub-path indices of every
    group (its outer ring first in NUMBER, the list itself in sub-path order), 'depth'."""
    rings = [np.ascontiguousarray(r, dtype=F) for r in rings]
    S = len(rings)
    V = sum(len(r) for r in rings)
    notes = {"groups": []}
    if V + 2 * (S - 1) > CAP:
        return TOO_LONG, None, notes
    pos = np.concatenate(rings)
    if not np.isfinite(pos).all():
        return NONFINITE, None, notes
    if any(TM.orientation(r) == 0 for r in rings):
        return DEGENERATE, None, notes
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(int)
    nxt0 = np.concatenate([start[r] + (np.arange(len(rings[r])) + 1) % len(rings[r]) for r in range(S)])
    EU, EV = pos, pos[nxt0]
    for i in range(V - 1):   # over the whole draw, pairs of edges of different groups included
        j = np.arange(i + 1, V)
        j = j[(j != nxt0[i]) & (nxt0[j] != i)]
        if j.size and RM.meet_many(EU[i], EV[i], EU[j], EV[j]).any():
            return NOT_SIMPLE, None, notes
    cls = classify(rings, even_odd)
    if cls is None:
        return NESTING, None, notes
    depth, outer = cls
    notes["depth"] = depth.tolist()
    tris = []
    for o in range(S):   # groups ascending by the sub-path index of their outer ring; the first refusal is the draw's
        if outer[o] != o:
            continue
        members = [r for r in range(S) if outer[r] == o]
        notes["groups"].append(members)
        local = np.concatenate([np.arange(start[r], start[r + 1]) for r in members])   # group-local vertex -> draw vertex
        if len(members) == 1:
            route, t = TM.ring_route(rings[o])
        else:
            route, t, _ = RM.rings_route([rings[r] for r in members], even_odd)
        if route != TRIANGLES:
            assert route in (NO_BRIDGE, STALLED), route   # everything else was decided over the whole draw
            return route, None, notes
        assert len(t) == len(local) + 2 * (len(members) - 1) - 2
        tris += [tuple(int(local[x]) for x in tri) for tri in t]
    assert len(tris) == V + 2 * S - 4 * len(notes["groups"])
    return TRIANGLES, tris, notes


# ---- what the call writes, from what vgx_concave_contours writes for the same input ----------------------------------------------
makes = TM.makes
_routes = {}


def draw_route(rings, even_odd):
    """(route, triangles as draw-local vertex triples, notes) of a mesh-making draw. Computed once per session per geometry."""
    k = (b"|".join(np.ascontiguousarray(r, dtype=F).tobytes() for r in rings), tuple(len(r) for r in rings), bool(even_odd) and len(rings) > 1)
    if k not in _routes:
        if len(rings) == 1:
            _routes[k] = ((TOO_LONG, None) if len(rings[0]) > CAP else TM.ring_route(rings[0])) + ({"groups": [[0]]},)
        else:
            _routes[k] = nested_route(rings, even_odd)
    return _routes[k]


def expected(specs, cpos, ccol, cidx, cmeshes, notes=None):
    """RM.expected for the nested entry: 3 (V + 2 S - 4 G) triangle indices, group after group."""
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
        moved = cpos[int(last["first_vertex"]):int(last["first_vertex"]) + V]   # the polyline, with AA the moved rings
        cuts = np.cumsum([len(q) for q in contours])[:-1]
        route, tris, nt = draw_route(np.split(moved, cuts), bool(flags & EO))
        if notes is not None:
            notes[d] = nt
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
        assert t.size == 3 * (V + 2 * len(contours) - 4 * len(nt["groups"]))
        if aa:
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


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def rect(x, y, w, h):
    return np.array([(x, y), (x + w, y), (x + w, y + h), (x, y + h)], dtype=F)


ISLAND = [sq(0, 0, 40), rev(sq(5, 5, 30)), sq(10, 10, 10)]
BULLSEYE = [sq(0, 0, 80), rev(sq(5, 5, 70)), sq(10, 10, 60), rev(sq(15, 15, 50)), sq(20, 20, 40)]
BULLSEYE_SAME = [sq(0, 0, 80), sq(5, 5, 70), sq(10, 10, 60), sq(15, 15, 50), sq(20, 20, 40)]
WORD_GLYPHS = "oBioBio"


def glyph(ch, x):
    if ch == "o":
        return [sq(x, 10, 10), rev(sq(x + 2.5, 12.5, 5))]
    if ch == "B":
        return [rect(x, 10, 10, 14), rev(sq(x + 2, 12, 3.5)), rev(sq(x + 2, 18, 3.5))]
    return [rect(x + 3, 15, 4, 10), sq(x + 3, 9, 4)]   # "i": the stem and the dot


def word_rings():
    subs = [r for k, ch in enumerate(WORD_GLYPHS) for r in glyph(ch, 2 + 13 * k)]
    return [subs[k] for k in np.random.RandomState(5).permutation(len(subs))]


def grid_islands_rings():
    rings = RM.grid_rings()
    for iy in range(12):
        for ix in range(12):
            cx, cy = 12 + 16 * ix, 12 + 16 * iy
            rings.append(np.array([(cx + 0.75, cy), (cx - 0.5, cy + 0.75), (cx - 0.5, cy - 0.75)], dtype=F))
    return rings


def max_rings(extra):
    """VGX_TRI_MAX_RINGS rings in CAP + extra slots: 818 triangles and one hexagon (extra = 1: a heptagon) on a grid of pitch 3."""
    rings = []
    for k in range(819):
        x, y = 3 * (k % 32), 3 * (k // 32)
        if k < 818:
            rings.append(np.array([(x, y), (x + 2, y), (x, y + 2)], dtype=F))
        else:
            pts = [(x, y), (x + 1, y), (x + 2, y), (x + 2, y + 1), (x + 1, y + 2), (x, y + 2)] + ([(x, y + 1)] if extra else [])
            rings.append(np.array(pts, dtype=F))
    return rings


def cap_nested_rings(extra):
    """CAP + extra slots in two groups: the rings model's outer star shortened by six vertices, a hole and an island in it."""
    outer = RM.cap_rings(extra - 6)[0]
    assert len(outer) == CAP - 12 + extra
    return [outer, rev(sq(40, 40, 10)), sq(43, 43, 4)]


# name -> (rings, fill flags beyond CONCAVE, fringe, the route the fixture is FOR, its groups, its triangles)
DRAWS = {
    "separate": ([sq(0, 0, 10), sq(20, 0, 10)], 0, 1.0, TRIANGLES, 2, 4),
    "separate_opposed": ([sq(0, 0, 10), rev(sq(20, 0, 10))], 0, 1.0, TRIANGLES, 2, 4),
    "island": (ISLAND, 0, 1.0, TRIANGLES, 2, 10),
    "island_eo": (ISLAND, EO, 1.0, TRIANGLES, 2, 10),
    "island_aa": (ISLAND, AA, 1.0, TRIANGLES, 2, 10),
    "island_with_hole_nz": (ISLAND[:2] + [rev(ISLAND[2])], 0, 1.0, TRIANGLES, 2, 10),
    "island_first": (ISLAND[::-1], 0, 1.0, TRIANGLES, 2, 10),
    "donut_same_nz": (RM.DRAWS["donut_same_nz"][0], 0, 1.0, NESTING, 0, 0),
    "bullseye": (BULLSEYE, 0, 1.0, TRIANGLES, 3, 18),
    "bullseye_eo_same": (BULLSEYE_SAME, EO, 1.0, TRIANGLES, 3, 18),
    "bullseye_eo_same_aa": (BULLSEYE_SAME, EO | AA, 1.0, TRIANGLES, 3, 18),
    "bullseye_depth3_runs": (BULLSEYE[:3] + [rev(BULLSEYE[3])] + BULLSEYE[4:], 0, 1.0, NESTING, 0, 0),
    "two_donuts_interleaved": ([rev(sq(60, 10, 20)), sq(0, 0, 40), sq(50, 0, 40), rev(sq(10, 10, 20))], 0, 1.0, TRIANGLES, 2, 16),
    "island_touches_hole": ([sq(0, 0, 40), rev(sq(5, 5, 30)), sq(5, 10, 10)], 0, 1.0, NOT_SIMPLE, 0, 0),
}
LARGE = {
    "word": (word_rings, 0, 1.0, TRIANGLES, 9, 60),
    "word_eo": (word_rings, EO, 1.0, TRIANGLES, 9, 60),
    "word_eo_aa": (word_rings, EO | AA, 1.0, TRIANGLES, 9, 60),
    "grid_islands": (grid_islands_rings, 0, 1.0, TRIANGLES, 145, 1442),
    "max_rings": (lambda: max_rings(0), 0, 1.0, TRIANGLES, 819, 822),
    "max_rings_plus_1": (lambda: max_rings(1), 0, 1.0, TOO_LONG, 0, 0),
    "cap_nested": (lambda: cap_nested_rings(0), 0, 1.0, TRIANGLES, 2, CAP - 12 + 8 + 6 - 8),
    "cap_nested_plus_1": (lambda: cap_nested_rings(1), 0, 1.0, TOO_LONG, 0, 0),
}
WORDS = ("word", "word_eo", "word_eo_aa")
_large = {}


def fixture(name):
    if name in LARGE:
        if name not in _large:
            make, *rest = LARGE[name]
            _large[name] = (make(),) + tuple(rest)
        return _large[name]
    return DRAWS[name]


def draw_spec(name, color=COLOR):
    rings, flags, fringe = fixture(name)[:3]
    return (rings, CONCAVE | flags, color, fringe)


def mixed_specs():
    """Triangulated and refused draws of one, two and many groups, between draws that make nothing."""
    return [
        draw_spec("separate"),
        ([TM.SQUARE], ENABLE | AA, 0xFF112233, 1.0),                       # a convex fill: nothing
        TM.ring_spec("l_cw_aa"),                                           # one ring: the single-ring rule
        draw_spec("word_eo_aa"),
        ([], CONCAVE | AA, 0xFFFFFFFF, 1.0),                               # no sub-path: nothing
        draw_spec("bullseye_depth3_runs"), draw_spec("island_touches_hole"),
        ([TM.star_shaped(12, 4), TM.SQUARE[:2]], CONCAVE, 0xFF00AA55, 1.0),   # a sub-path of 2 vertices: nothing at all
        RM.draw_spec("b_aa"),                                              # one group: the rings rule
        draw_spec("bullseye_eo_same_aa"), draw_spec("donut_same_nz"),
        TM.ring_spec("bowtie"),
        draw_spec("island_first"), RM.draw_spec("nan_hole"), draw_spec("word"), draw_spec("two_donuts_interleaved"),
    ]


MIXED_ROUTES = [TRIANGLES, 0, TRIANGLES, TRIANGLES, 0, NESTING, NOT_SIMPLE, 0, TRIANGLES, TRIANGLES, NESTING, NOT_SIMPLE, TRIANGLES, NONFINITE, TRIANGLES, TRIANGLES]
