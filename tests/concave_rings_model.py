"""vgx_concave_triangulate_rings: the rule of include/vgx.h for a draw of several sub-paths -- one outer ring with holes directly inside
it, bridged into one ring of slots and clipped -- in numpy / Python, built on the canonical edge value, the edge-pair clauses and the
single-ring route of tests/concave_triangulate_model.py (imported, untouched); what a call writes; the fixtures the CPU and GPU tests
share and the conditions they must meet (tests/test_concave_rings_cpu.py: the lane code; tests/test_gpu_concave_rings.py: the kernels).

The model keeps the rings' edges and the bridges as explicit lists; the lane code and the kernel read both off the slot links. That the
two agree on every fixture is part of what the tests show."""
import numpy as np

import concave_triangulate_model as TM
from concave_triangulate_model import c, c_many, in_box, sign

capi = TM.capi
F = np.float32
CONCAVE, AA, EO, ENABLE = TM.CONCAVE, TM.AA, TM.EO, TM.ENABLE
TRIANGLES, TOO_LONG, NONFINITE, DEGENERATE, NOT_SIMPLE, STALLED = TM.TRIANGLES, TM.TOO_LONG, TM.NONFINITE, TM.DEGENERATE, TM.NOT_SIMPLE, TM.STALLED
NESTING, NO_BRIDGE = capi.TRI_REFUSED_NESTING, capi.TRI_REFUSED_NO_BRIDGE
CAP = TM.CAP
FILL_KIND = TM.FILL_KIND
COLOR = TM.COLOR


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def meet_many(u1, v1, U2, V2):
    """tri_edges_meet of the one edge u1 -> v1 against the edges U2 -> V2: bool [n]."""
    U2, V2 = np.atleast_2d(U2), np.atleast_2d(V2)
    u1, v1 = np.asarray(u1, dtype=F)[None], np.asarray(v1, dtype=F)[None]
    a, b = np.sign(c_many(u1, v1, U2)), np.sign(c_many(u1, v1, V2))
    cc, d = np.sign(c_many(U2, V2, u1)), np.sign(c_many(U2, V2, v1))
    A, B = np.broadcast_to(u1, U2.shape), np.broadcast_to(v1, U2.shape)
    return ((a * b < 0) & (cc * d < 0)) | ((a == 0) & in_box(U2, A, B)) | ((b == 0) & in_box(V2, A, B)) | ((cc == 0) & in_box(A, U2, V2)) | ((d == 0) & in_box(B, U2, V2))


def key(pos, i):
    return (float(pos[i][0]), float(pos[i][1]), i)


def inside(p, ring):
    """The parity of the edges u -> v of ring with (u.y <= p.y) != (v.y <= p.y) and sign(c(u, v, p)) == sign(v.y - u.y)."""
    u, v = ring, np.roll(ring, -1, axis=0)
    straddle = (u[:, 1] <= p[1]) != (v[:, 1] <= p[1])
    side = np.sign(c_many(u, v, p)) == np.sign(v[:, 1].astype(np.float64) - u[:, 1].astype(np.float64))
    return bool(int((straddle & side).sum()) & 1)


def clip_slots(P, prv, nxt, s):
    """TM.clip over a ring of slots with given links, the cursor at slot 0, with the amendment: a slot whose position compares equal in
    both coordinates to that of a, b or c does not block. Triangles as slots, or None when it stalls."""
    N = len(P)
    prv, nxt = list(prv), list(nxt)
    linked = np.ones(N, dtype=bool)
    tris, b, size, misses = [], 0, N, 0
    while size > 3:
        a, cn = prv[b], nxt[b]
        t = s * c(P[a], P[b], P[cn])
        ear = t == 0
        if t > 0:
            others = linked.copy()
            others[[a, b, cn]] = False
            for k in (a, b, cn):
                others &= ~((P[:, 0] == P[k][0]) & (P[:, 1] == P[k][1]))
            Q = P[others]
            blocks = (s * c_many(P[a], P[b], Q) >= 0) & (s * c_many(P[b], P[cn], Q) >= 0) & (s * c_many(P[cn], P[a], Q) >= 0) if len(Q) else np.zeros(0, bool)
            ear = not blocks.any()
        if ear:
            tris.append((a, b, cn))
            nxt[a], prv[cn], linked[b] = cn, a, False
            b, size, misses = nxt[cn], size - 1, 0
        else:
            b, misses = cn, misses + 1
            if misses > size:
                return None
    tris.append((prv[b], b, nxt[b]))
    return tris


def rings_route(rings, even_odd):
    """(route, triangles as vertex triples or None, notes) of a draw of S >= 2 rings (float32 [n, 2] each, in sub-path order). notes:
    'trips' = candidates tried per processed hole, 'bridges' = (M, slot q) per processed hole, 's', 'outer'."""
    rings = [np.ascontiguousarray(r, dtype=F) for r in rings]
    S, H = len(rings), len(rings) - 1
    V = sum(len(r) for r in rings)
    notes = {"trips": [], "bridges": []}
    if V + 2 * H > CAP:
        return TOO_LONG, None, notes
    pos = np.concatenate(rings)
    if not np.isfinite(pos).all():
        return NONFINITE, None, notes
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(int)
    ring_of = np.repeat(np.arange(S), [len(r) for r in rings])
    nxt0 = np.concatenate([start[r] + (np.arange(len(rings[r])) + 1) % len(rings[r]) for r in range(S)])
    prv0 = np.concatenate([start[r] + (np.arange(len(rings[r])) - 1) % len(rings[r]) for r in range(S)])
    sg = [TM.orientation(r) for r in rings]
    if any(x == 0 for x in sg):
        return DEGENERATE, None, notes
    EU, EV = pos, pos[nxt0]
    for i in range(V - 1):
        j = np.arange(i + 1, V)
        j = j[(j != nxt0[i]) & (nxt0[j] != i)]
        if j.size and meet_many(EU[i], EV[i], EU[j], EV[j]).any():
            return NOT_SIMPLE, None, notes
    o = int(ring_of[min(range(V), key=lambda i: key(pos, i))])
    s = sg[o]
    notes["s"], notes["outer"] = s, o
    holes = [h for h in range(S) if h != o]
    m = {h: max(range(start[h], start[h + 1]), key=lambda i: key(pos, i)) for h in holes}
    for h in holes:
        if not even_odd and sg[h] != -s:
            return NESTING, None, notes
        if not inside(pos[m[h]], rings[o]) or any(inside(pos[m[h]], rings[g]) for g in holes if g != h):
            return NESTING, None, notes
    # the merged ring of slots
    N = V + 2 * H
    vert = list(range(V)) + [0] * (2 * H)
    nxt, prv = list(nxt0) + [0] * (2 * H), list(prv0) + [0] * (2 * H)
    merged = list(range(start[o], start[o + 1]))
    bridges = []
    for j, h in enumerate(sorted(holes, key=lambda h: key(pos, m[h]), reverse=True)):
        M = m[h]
        pM = pos[M]
        q = np.array(merged)
        pq, pa, pn = pos[[vert[x] for x in q]], pos[[vert[prv[x]] for x in q]], pos[[vert[nxt[x]] for x in q]]
        after = (pq[:, 0] > pM[0]) | ((pq[:, 0] == pM[0]) & (pq[:, 1] > pM[1]))
        t, e1, e2 = s * c_many(pa, pq, pn), s * c_many(pa, pq, pM), s * c_many(pq, pn, pM)
        cone = np.where(t > 0, (e1 > 0) & (e2 > 0), (e1 > 0) | (e2 > 0))
        dx, dy = pq[:, 0].astype(np.float64) - float(pM[0]), pq[:, 1].astype(np.float64) - float(pM[1])
        d2 = dx * dx + dy * dy
        cands = sorted((float(d2[k]), int(q[k])) for k in np.nonzero(after & cone)[0])
        trips, found = 0, None
        for _, slot in cands:
            trips += 1
            vq = vert[slot]
            keep = (np.arange(V) != M) & (nxt0 != M) & (np.arange(V) != vq) & (nxt0 != vq)
            hit = meet_many(pM, pos[vq], EU[keep], EV[keep]).any() if keep.any() else False
            for (bm, bq) in bridges:
                if not hit and bm != M and bq != M and bm != vq and bq != vq:
                    hit = bool(meet_many(pM, pos[vq], pos[bm], pos[bq])[0])
            if not hit:
                found = slot
                break
        notes["trips"].append(trips)
        if found is None:
            return NO_BRIDGE, None, notes
        notes["bridges"].append((M, found))
        bridges.append((M, vert[found]))
        members = list(range(start[h], start[h + 1]))
        if sg[h] == s:   # traversed backwards
            for i in members:
                nxt[i], prv[i] = prv[i], nxt[i]
        A, B, qn, last = V + 2 * j, V + 2 * j + 1, nxt[found], prv[M]
        vert[A], vert[B] = M, vert[found]
        nxt[found], prv[M] = M, found
        nxt[last], prv[A] = A, last
        nxt[A], prv[B] = B, A
        nxt[B], prv[qn] = qn, B
        merged += members + [A, B]
    # one ring over all N slots
    seen, x = 0, 0
    while True:
        seen, x = seen + 1, nxt[x]
        assert prv[x] is not None and seen <= N
        if x == 0:
            break
    assert seen == N
    tris = clip_slots(pos[vert], prv, nxt, float(s))
    if tris is None:
        return STALLED, None, notes
    return TRIANGLES, [tuple(vert[x] for x in t) for t in tris], notes


# ---- what the call writes, from what vgx_concave_contours writes for the same input ----------------------------------------------
makes = TM.makes
_routes = {}


def draw_route(rings, even_odd):
    """(route, triangles as draw-local vertex triples) of a mesh-making draw: one ring by the single-ring rule, more by the rule above.
    Computed once per session per geometry."""
    k = (b"|".join(np.ascontiguousarray(r, dtype=F).tobytes() for r in rings), len(rings), bool(even_odd) and len(rings) > 1)
    if k not in _routes:
        if len(rings) == 1:
            _routes[k] = ((TOO_LONG, None) if len(rings[0]) > CAP else TM.ring_route(rings[0])) + ({},)
        else:
            _routes[k] = rings_route(rings, even_odd)
    return _routes[k]


def expected(specs, cpos, ccol, cidx, cmeshes, notes=None):
    """TM.expected for the rings entry: specs (contours, fill_flags, colour, fringe) per draw; c*: vgx_concave_contours' output for
    them. Returns (routes, pos, color, idx, meshes)."""
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
        assert t.size == 3 * (V + 2 * (len(contours) - 1) - 2)
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
def sq(x, y, w):
    return np.array([(x, y), (x + w, y), (x + w, y + w), (x, y + w)], dtype=F)


def rev(r):
    return np.ascontiguousarray(np.asarray(r, dtype=F)[::-1])


def jitter_star(rs, n, cx, cy, r0, r1):
    """A star-shaped ring of n vertices about (cx, cy): one vertex in every sector of 2 pi / n, so no angular gap reaches pi (n >= 5)."""
    ang = (np.arange(n) + rs.uniform(0.1, 0.9, n)) * (2 * np.pi / n)
    rad = rs.uniform(r0, r1, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).astype(F)


OCCLUDED = [np.array([(0, 0), (40, 0), (40, 9), (14.5, 10), (40, 11), (40, 20), (0, 20)], dtype=F),
            rev([(12, 5), (13, 5), (13, 15), (12, 15)]), rev([(4, 8), (10, 10), (4, 12)])]
SHARED = [np.array([(0, 0), (40, 0), (60, 12), (40, 24), (0, 24)], dtype=F), np.array([(33, 10), (10, 5), (10, 15)], dtype=F),
          np.array([(32.5, 18), (25, 17), (25, 19)], dtype=F)]
# a comb: a spine along the top, three teeth down; two holes in the spine, one in every tooth, one more in the widest tooth
COMB_OUTER = np.array([(0, 0), (60, 0), (60, 50), (44, 50), (44, 14), (36, 14), (36, 50), (24, 50), (24, 14), (16, 14), (16, 50), (0, 50)], dtype=F)
COMB = [COMB_OUTER, rev(sq(4, 3, 8)), rev(sq(40, 4, 6)), rev(sq(3, 20, 10)), rev(sq(26, 30, 8)), rev(sq(47, 18, 9)), rev(sq(48, 36, 8))]


def grid_rings():
    rs = np.random.RandomState(11)
    rings = [sq(0, 0, 200)]
    for iy in range(12):
        for ix in range(12):
            rings.append(rev(np.round(jitter_star(rs, 7, 12.0 + 16 * ix, 12.0 + 16 * iy, 2.0, 6.0) * 4) / 4))
    return rings


def cap_rings(extra):
    """N = CAP + extra slots: an outer star of CAP - 6 + extra vertices and one square hole."""
    n = CAP - 6 + extra
    outer = TM.star(45.0, 45.0, 44.0, 39.0, n // 2, 0.003) if n % 2 == 0 else TM.star_shaped(n, 9, r0=30.0)
    return [outer, rev(sq(40, 40, 10))]


# A hole 0.75 from the outer ring's left edge: as it stands the rings are apart; with a fringe of 2 the outer ring moves in by 1 and
# the hole's ring moves by 1 as well, and the two cross
SPIKE_HOLE = [sq(0, 0, 40), rev(sq(0.75, 10, 10))]

# name -> (rings, fill flags beyond CONCAVE, fringe, the route the fixture is FOR)
DRAWS = {
    "donut": ([sq(0, 0, 40), rev(sq(10, 10, 20))], 0, 1.0, TRIANGLES),
    "donut_hole_first": ([rev(sq(10, 10, 20)), sq(0, 0, 40)], 0, 1.0, TRIANGLES),
    "donut_cw": ([rev(sq(0, 0, 40)), sq(10, 10, 20)], 0, 1.0, TRIANGLES),
    "donut_same_nz": ([sq(0, 0, 40), sq(10, 10, 20)], 0, 1.0, NESTING),
    "donut_same_eo": ([sq(0, 0, 40), sq(10, 10, 20)], EO, 1.0, TRIANGLES),
    "donut_aa": ([sq(0, 0, 40), rev(sq(10, 10, 20))], AA, 1.0, TRIANGLES),
    "donut_same_eo_aa": ([sq(0, 0, 40), sq(10, 10, 20)], EO | AA, 1.5, TRIANGLES),
    "b": ([sq(0, 0, 40), rev(sq(5, 5, 10)), rev(sq(5, 22, 10))], 0, 1.0, TRIANGLES),
    "b_aa": ([sq(0, 0, 40), rev(sq(5, 5, 10)), rev(sq(5, 22, 10))], AA, 1.0, TRIANGLES),
    "row": ([sq(0, 0, 100)] + [rev(sq(5 + 12 * i, 40, 8)) for i in range(7)], 0, 1.0, TRIANGLES),
    "island": ([sq(0, 0, 40), rev(sq(5, 5, 30)), sq(10, 10, 10)], 0, 1.0, NESTING),
    "island_eo": ([sq(0, 0, 40), rev(sq(5, 5, 30)), sq(10, 10, 10)], EO, 1.0, NESTING),
    "separate": ([sq(0, 0, 10), sq(20, 0, 10)], 0, 1.0, NESTING),
    "touching": ([sq(0, 0, 40), rev(sq(10, 0, 10))], 0, 1.0, NOT_SIMPLE),
    "crossing": ([sq(0, 0, 40), rev(sq(30, 10, 20))], 0, 1.0, NOT_SIMPLE),
    "occluded": (OCCLUDED, 0, 1.0, TRIANGLES),
    "shared": (SHARED, 0, 1.0, TRIANGLES),
    "shared_rev_eo": ([rev(r) for r in SHARED], EO, 1.0, TRIANGLES),
    "comb": (COMB, 0, 1.0, TRIANGLES),
    "comb_eo_aa": (COMB, EO | AA, 1.0, TRIANGLES),
    "flat_hole": ([sq(0, 0, 40), np.array([(10, 10), (14, 12), (18, 14)], dtype=F)], 0, 1.0, DEGENERATE),
    "nan_hole": ([sq(0, 0, 40), np.array([(10, 10), (np.nan, 12), (18, 30)], dtype=F)], 0, 1.0, NONFINITE),
    "spike_hole": (SPIKE_HOLE, 0, 2.0, TRIANGLES),
    "spike_hole_aa": (SPIKE_HOLE, AA, 2.0, NOT_SIMPLE),
}
LARGE = {
    "grid": (grid_rings, 0, 1.0, TRIANGLES),
    "cap": (lambda: cap_rings(0), 0, 1.0, TRIANGLES),
    "cap_plus_1": (lambda: cap_rings(1), 0, 1.0, TOO_LONG),
}
NOT_IMAGED = ("nan_hole",)
_large = {}


def fixture(name):
    if name in LARGE:
        if name not in _large:
            make, flags, fringe, meant = LARGE[name]
            _large[name] = (make(), flags, fringe, meant)
        return _large[name]
    return DRAWS[name]


def draw_spec(name, color=COLOR):
    rings, flags, fringe, _ = fixture(name)
    return (rings, CONCAVE | flags, color, fringe)


def random_set(seed, even_odd):
    """A star-shaped outer of 5 .. 40 vertices and 1 .. 8 star holes on the quarter grid, sub-paths shuffled. Under even-odd the holes'
    orientations are random. Holes may meet each other or the outer ring: such a set is refused as NOT_SIMPLE or NESTING."""
    rs = np.random.RandomState(1000 + seed)
    q = lambda r: (np.round(r * 4) / 4).astype(F)
    rings = [q(jitter_star(rs, int(rs.randint(5, 41)), 45.0, 45.0, 30.0, 42.0))]
    centres = []
    for _ in range(int(rs.randint(1, 9))):
        for _ in range(6):   # a few tries to keep the holes apart; what still overlaps stays
            a, r = rs.uniform(0, 2 * np.pi), rs.uniform(0.0, 22.0)
            cx, cy = 45.0 + r * np.cos(a), 45.0 + r * np.sin(a)
            if all((cx - x) ** 2 + (cy - y) ** 2 >= 81.0 for x, y in centres):
                break
        centres.append((cx, cy))
        h = q(jitter_star(rs, int(rs.randint(5, 10)), cx, cy, 1.5, 4.5))
        rings.append(h if (even_odd and rs.randint(2)) else rev(h))
    order = rs.permutation(len(rings))
    return [rings[k] for k in order]


RANDOM_SEEDS = tuple(range(10))


def random_specs():
    return [(random_set(seed, eo), CONCAVE | (EO if eo else 0), COLOR ^ (0x00030507 * seed & 0x00FFFFFF), 1.0) for seed in RANDOM_SEEDS for eo in (False, True)]


def mixed_specs():
    """Triangulated and refused draws of one and several sub-paths between draws that make nothing."""
    return [
        draw_spec("donut"),
        ([TM.SQUARE], ENABLE | AA, 0xFF112233, 1.0),                       # a convex fill: nothing
        TM.ring_spec("l_cw_aa"),                                           # one ring: the single-ring rule
        draw_spec("b_aa"),
        ([], CONCAVE | AA, 0xFFFFFFFF, 1.0),                               # no sub-path: nothing
        draw_spec("island"), draw_spec("touching"),
        ([TM.star_shaped(12, 4), TM.SQUARE[:2]], CONCAVE, 0xFF00AA55, 1.0),   # a sub-path of 2 vertices: nothing at all
        draw_spec("donut_same_eo_aa"), draw_spec("spike_hole_aa"),
        TM.ring_spec("bowtie"), TM.ring_spec("blob"),
        draw_spec("shared"), draw_spec("flat_hole"), draw_spec("nan_hole"), draw_spec("separate"),
    ]


MIXED_ROUTES = [TRIANGLES, 0, TRIANGLES, TRIANGLES, 0, NESTING, NOT_SIMPLE, 0, TRIANGLES, NOT_SIMPLE, NOT_SIMPLE, TRIANGLES, TRIANGLES, DEGENERATE, NONFINITE, NESTING]
