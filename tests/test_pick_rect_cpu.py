"""CPU: the lane code of vgx_pick_rect (csrc/vgx_pick_rect.h through libvgx_hosttest.so: vgxt_pick_rect, a plain loop over queries, entries,
meshes and triangles) against the numpy statement of the specification (tests/pick_rect_model.py) on frames written by the reference, and
six relations that do not rest on the model. Exact everywhere; the GPU suite (tests/test_gpu_pick_rect.py) makes the same comparison on the
kernels."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import pick_rect_model as R

P = R.P
capi = R.capi
F = np.float32
NONE = R.NONE
PATTERN = 0x5A5A5A5A
SKIP, WINDOW, BY_DRAW = R.SKIP, R.WINDOW, R.BY_DRAW


@pytest.fixture(scope="module")
def host():
    path = os.path.join(R.CM.ROOT, "vg-renderer_amd", "libvgx_hosttest.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(path)
    lib.vgxt_pick_rect.restype = C.c_int
    lib.vgxt_pick_rect.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(capi.PickRectOut)]
    lib.vgxt_pick_rect_touch.restype = C.c_int
    lib.vgxt_pick_rect_touch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.vgxt_pick.restype = C.c_int
    lib.vgxt_pick.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vgxt_mesh_bounds.restype = None
    lib.vgxt_mesh_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


class Got:
    pass


def desc_of(f):
    f.host_arrays = getattr(f, "host_arrays", None) or (np.ascontiguousarray(f.pos, dtype=F), np.ascontiguousarray(f.color, dtype=np.uint32),
                                                          np.ascontiguousarray(f.idx, dtype=np.uint16), np.ascontiguousarray(f.meshes))
    pos, color, idx, meshes = f.host_arrays
    return capi.CacheDesc(pos.ctypes.data, color.ctypes.data, idx.ctypes.data, meshes.ctypes.data, meshes.shape[0], pos.shape[0], idx.shape[0])


def host_pick_rect(host, f, queries, cap=R.LIST_CAP, bounds=None, want=("top", "list", "count"), guard=2):
    """vgxt_pick_rect in calls of at most 64 queries, each into pattern-filled arrays with guard rows. Returns top, count and the list
    rows as the call left them (entries behind min(count, cap) still hold the pattern; an output that was not asked for is all pattern)."""
    d = desc_of(f)
    nq = queries.shape[0]
    g = Got()
    g.top = np.full(nq * 4, PATTERN, dtype=np.uint32).view(capi.pick_hit_dtype)
    g.count = np.full(nq, PATTERN, dtype=np.uint32)
    g.list = np.full((nq, cap), PATTERN, dtype=np.uint32)
    for a, b in R.chunks(nq):
        n = b - a
        q = np.ascontiguousarray(queries[a:b])
        top = np.full((n + guard) * 4, PATTERN, dtype=np.uint32)
        lst = np.full((n + guard) * max(cap, 1), PATTERN, dtype=np.uint32)
        cnt = np.full(n + guard, PATTERN, dtype=np.uint32)
        out = capi.PickRectOut(top.ctypes.data if "top" in want else None, lst.ctypes.data if "list" in want and cap else None,
                               cnt.ctypes.data if "count" in want else None, cap if "list" in want else 0, 0)
        assert host.vgxt_pick_rect(C.byref(d), None if bounds is None else bounds.ctypes.data, q.ctypes.data, n, C.byref(out)) == capi.VGX_OK
        assert np.all(top[n * 4:] == PATTERN) and np.all(lst[n * cap:] == PATTERN) and np.all(cnt[n:] == PATTERN)
        assert q.tobytes() == np.ascontiguousarray(queries[a:b]).tobytes()
        g.top[a:b] = top[:n * 4].view(capi.pick_hit_dtype)
        g.count[a:b] = cnt[:n]
        g.list[a:b] = lst[:n * cap].reshape(n, cap)
    return g


def host_bounds(host, f):
    d = desc_of(f)
    mb = np.zeros((max(f.nm, 1), 4), dtype=F)
    host.vgxt_mesh_bounds(d.pos, d.meshes, f.nm, mb.ctypes.data)
    return mb


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_equals_model(g, r, cap, sl=slice(None), want=("top", "list", "count")):
    ans = r.answer
    if "top" in want:
        bad = np.nonzero((g.top.view(np.uint32).reshape(-1, 4) != ans.top[sl].view(np.uint32).reshape(-1, 4)).any(axis=1))[0]
        assert bad.size == 0, (bad[:8], r.kind[sl][bad[:8]], g.top[bad[:4]], ans.top[sl][bad[:4]])
    else:
        assert np.all(g.top.view(np.uint32) == PATTERN)
    if "count" in want:
        bad = np.nonzero(g.count != ans.count[sl])[0]
        assert bad.size == 0, (bad[:8], r.kind[sl][bad[:8]], g.count[bad[:8]], ans.count[sl][bad[:8]])
    else:
        assert np.all(g.count == PATTERN)
    if "list" in want:
        wl = R.lists(ans, cap, PATTERN)[sl]
        bad = np.nonzero((g.list != wl).any(axis=1))[0]
        assert bad.size == 0, (bad[:8], r.kind[sl][bad[:8]], g.list[bad[:2]], wl[bad[:2]])
    else:
        assert np.all(g.list == PATTERN)


@pytest.mark.parametrize("name,n", R.CASES)
def test_lane_code_equals_model(host, name, n):
    r = R.frame(name, n)
    R.check_query_conditions(r)
    g = host_pick_rect(host, r.f, r.queries)
    assert_equals_model(g, r, R.LIST_CAP)
    # with the boxes handed in instead of computed by the call: the same bytes
    mb = host_bounds(host, r.f)
    assert np.array_equal(mb[:r.f.nm].view(np.uint32), r.boxes.view(np.uint32)) or np.array_equal(mb[:r.f.nm], r.boxes)
    gb = host_pick_rect(host, r.f, r.queries, bounds=mb)
    assert same(gb.top, g.top) and same(gb.count, g.count) and same(gb.list, g.list)


def test_frame_of_many_small_meshes(host):
    r = R.many_meshes()
    assert np.array_equal(host_bounds(host, r.f)[:r.f.nm], r.boxes)
    assert_equals_model(host_pick_rect(host, r.f, r.queries, cap=64), r, 64)


@pytest.mark.parametrize("want", [("list", "count"), ("top", "count"), ("top", "list"), ("count",)])
def test_null_outputs(host, want):
    r = R.frame("tiger", 65)
    sl = slice(0, 64)
    g = host_pick_rect(host, r.f, r.queries[sl], want=want)
    assert_equals_model(g, r, R.LIST_CAP, sl, want)


@pytest.mark.parametrize("cap", [0, 1, 64])
def test_list_capacities(host, cap):
    r = R.frame("tiger", 65)
    sl = slice(64, 128)
    g = host_pick_rect(host, r.f, r.queries[sl], cap=cap)
    assert_equals_model(g, r, cap, sl, ("top", "list", "count") if cap else ("top", "count"))


def test_host_argument_checks(host):
    r = R.frame("tiger", 65)
    d = desc_of(r.f)
    q = np.zeros(65, dtype=capi.pick_rect_query_dtype)
    top = np.full(66 * 4, PATTERN, dtype=np.uint32)
    lst = np.full(66 * 4, PATTERN, dtype=np.uint32)
    cnt = np.full(66, PATTERN, dtype=np.uint32)

    def call(desc=d, bounds=None, queries=q.ctypes.data, nq=1, top_p=top.ctypes.data, list_p=lst.ctypes.data, count_p=cnt.ctypes.data, cap=4, reserved=0, out=True):
        o = capi.PickRectOut(top_p, list_p, count_p, cap, reserved)
        return host.vgxt_pick_rect(C.byref(desc) if desc is not None else None, bounds, queries, nq, C.byref(o) if out else None)

    assert call(nq=65) == capi.VGX_E_RANGE  # the 65th query
    assert call(queries=None) == capi.VGX_E_INVALID_ARG
    assert call(desc=None) == capi.VGX_E_INVALID_ARG
    assert call(out=False) == capi.VGX_E_INVALID_ARG
    assert call(list_p=None) == capi.VGX_E_INVALID_ARG  # a capacity without a list
    assert call(reserved=1) == capi.VGX_E_INVALID_ARG
    assert call(queries=q.ctypes.data + 4) == capi.VGX_E_INVALID_ARG
    assert call(top_p=top.ctypes.data + 8) == capi.VGX_E_INVALID_ARG
    assert call(list_p=lst.ctypes.data + 2) == capi.VGX_E_INVALID_ARG
    assert call(count_p=cnt.ctypes.data + 1) == capi.VGX_E_INVALID_ARG
    assert call(bounds=r.f.host_arrays[0].ctypes.data + 8) == capi.VGX_E_INVALID_ARG
    big = capi.CacheDesc(d.pos, d.color, d.idx, d.meshes, 0xFFFFFFFF, d.num_vertices, d.num_indices)
    assert call(desc=big) == capi.VGX_E_RANGE
    assert np.all(top == PATTERN) and np.all(lst == PATTERN) and np.all(cnt == PATTERN)
    # valid: no queries (nothing written), no meshes (every count 0, every top "none"), everything NULL but the struct
    assert call(queries=None, nq=0) == capi.VGX_OK
    assert np.all(top == PATTERN) and np.all(cnt == PATTERN)
    assert call(top_p=None, list_p=None, count_p=None, cap=0) == capi.VGX_OK
    none = capi.CacheDesc(None, None, None, None, 0, 0, 0)
    q["x1"], q["y1"], q["mesh_end"] = 1, 1, NONE
    assert call(desc=none, nq=3) == capi.VGX_OK
    assert np.all(top[:12] == NONE) and np.all(top[12:] == PATTERN) and np.all(cnt[:3] == 0) and np.all(cnt[3:] == PATTERN) and np.all(lst == PATTERN)
    # a non-zero reserved word in a query selects nothing
    q2 = r.queries[r.kind == "square"][:2].copy()
    q2["reserved"][1] = 7
    g = host_pick_rect(host, r.f, q2)
    assert g.count[0] > 0 and g.count[1] == 0 and np.all(g.top[1:].view(np.uint32) == NONE)


# ---- (a) the degenerate rectangle is vgx_pick's point test -------------------------------------------------------------------
def point_queries(r):
    """The degenerate rectangles of the set with mesh_begin = 0 and neither WINDOW nor BY_DRAW, and the vgx_pick queries they are."""
    q = r.queries
    sel = np.nonzero((q["x0"] == q["x1"]) & (q["y0"] == q["y1"]) & (q["mesh_begin"] == 0) & ((q["flags"] & (WINDOW | BY_DRAW)) == 0) & (q["reserved"] == 0))[0]
    pq = np.zeros(sel.size, dtype=capi.pick_query_dtype)
    pq["x"], pq["y"], pq["mesh_end"], pq["flags"] = q["x0"][sel], q["y0"][sel], q["mesh_end"][sel], q["flags"][sel]
    return sel, pq


@pytest.mark.parametrize("name,n", R.CASES)
def test_degenerate_rectangle_is_the_point_pick(host, name, n):
    r = R.frame(name, n)
    sel, pq = point_queries(r)
    assert sel.size >= 40
    hits = np.zeros(sel.size, dtype=capi.pick_hit_dtype)
    d = desc_of(r.f)
    assert host.vgxt_pick(C.byref(d), None, pq.ctypes.data, sel.size, hits.ctypes.data) == capi.VGX_OK
    g = host_pick_rect(host, r.f, r.queries[sel])
    assert same(g.top, hits), np.nonzero((g.top.view(np.uint32).reshape(-1, 4) != hits.view(np.uint32).reshape(-1, 4)).any(axis=1))[0][:8]
    if r.key == R.BIG:
        assert 5 <= int((hits["mesh"] != NONE).sum()) < sel.size


# ---- (b), (c) the predicate against exact rational arithmetic, and its two forms ---------------------------------------------------
def fr(v):
    return Fraction(float(v))


def exact_touch(tri, rect):
    """A closed triangle with A != 0 meets a closed valid rectangle: a vertex in the rectangle, a rectangle corner in the triangle, or an
    edge that meets a side -- over the rationals, nothing rounds."""
    a, b, c = [(fr(tri[2 * k]), fr(tri[2 * k + 1])) for k in range(3)]
    x0, y0, x1, y1 = [fr(v) for v in rect]
    if not (x0 <= x1 and y0 <= y1):
        return False
    A = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if A == 0:
        return False
    if any(x0 <= p[0] <= x1 and y0 <= p[1] <= y1 for p in (a, b, c)):
        return True
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]

    def edge(u, v, p):
        return (v[0] - u[0]) * (p[1] - u[1]) - (v[1] - u[1]) * (p[0] - u[0])

    s = 1 if A > 0 else -1
    if any(all(s * edge(u, v, p) >= 0 for u, v in ((a, b), (b, c), (c, a))) for p in corners):
        return True

    def meet(p, q, u, v):
        d1, d2, d3, d4 = edge(u, v, p), edge(u, v, q), edge(p, q, u), edge(p, q, v)
        if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
            return True

        def on(u, v, p):  # p on the closed segment u v, given that it is collinear
            return min(u[0], v[0]) <= p[0] <= max(u[0], v[0]) and min(u[1], v[1]) <= p[1] <= max(u[1], v[1])
        return (d1 == 0 and on(u, v, p)) or (d2 == 0 and on(u, v, q)) or (d3 == 0 and on(p, q, u)) or (d4 == 0 and on(p, q, v))

    sides = [(corners[k], corners[(k + 1) % 4]) for k in range(4)]
    return any(meet(p, q, u, v) for p, q in sides for u, v in ((a, b), (b, c), (c, a)))


@pytest.fixture(scope="module")
def pairs():
    """2 000 (triangle, rectangle) pairs: 500 from the Tiger frame (rectangles beside, on and around the triangle's own vertices) and 500
    of each synthetic family of the header -- a 0..8 integer grid, 1/8-unit coordinates in 300..556, random binary32 in [512, 1024) --
    one pair in seven with a degenerate rectangle side, one in eleven with a degenerate triangle side."""
    rs = np.random.RandomState(5)
    T = R.frame("tiger", 65).f.tris
    out = []
    for g in rs.choice(np.nonzero(T.valid)[0], size=500, replace=False):
        tri = np.concatenate([T.a[g], T.b[g], T.c[g]]).astype(F)
        lo, hi = tri.reshape(3, 2).min(axis=0), tri.reshape(3, 2).max(axis=0)
        v = tri.reshape(3, 2)[g % 3]
        mode = g % 5
        if mode == 0:    # a corner of the rectangle on a vertex
            rect = [v[0] - 2, v[1] - 2, v[0], v[1]]
        elif mode == 1:  # a side through a vertex
            rect = [v[0], lo[1] - 1, v[0] + 3, hi[1] + 1]
        elif mode == 2:  # somewhere in the triangle's box, small against it
            c = lo + (hi - lo) * rs.uniform(0, 1, 2)
            w = (hi - lo) * rs.uniform(0, 0.2, 2)
            rect = [c[0] - w[0], c[1] - w[1], c[0] + w[0], c[1] + w[1]]
        elif mode == 3:  # beside it, up to its box and a little over
            w = (hi - lo) * rs.uniform(-0.2, 0.4)
            rect = [lo[0] - 5, lo[1] - 5, lo[0] + w[0], lo[1] + w[1]]
        else:            # a point: an edge's midpoint where binary32 holds it exactly, else a vertex
            u, w2 = tri.reshape(3, 2)[g % 3].astype(np.float64), tri.reshape(3, 2)[(g + 1) % 3].astype(np.float64)
            mid = (u + w2) / 2
            p = mid.astype(F) if np.array_equal(mid.astype(F).astype(np.float64), mid) else v
            rect = [p[0], p[1], p[0], p[1]]
        out.append((tri, np.array(rect, dtype=F)))
    for family in range(3):
        for k in range(500):
            if family == 0:
                pts = rs.randint(0, 9, size=10).astype(F)
            elif family == 1:
                pts = (300 + rs.randint(0, 2049, size=10) / 8.0).astype(F)
            else:
                pts = rs.uniform(512, 1024, size=10).astype(F)
            tri, rect = pts[:6].copy(), pts[6:].copy()
            rect = np.array([min(rect[0], rect[2]), min(rect[1], rect[3]), max(rect[0], rect[2]), max(rect[1], rect[3])], dtype=F)
            if k % 7 == 0:
                rect[2 + k % 2] = rect[k % 2]
            if k % 11 == 0:
                tri[2:4] = tri[0:2]
            out.append((tri, rect))
    return out


def lane_touch(host, tri, rect, four):
    tri, rect = np.ascontiguousarray(tri, dtype=F), np.ascontiguousarray(rect, dtype=F)
    return bool(host.vgxt_pick_rect_touch(tri.ctypes.data, rect.ctypes.data, 1 if four else 0))


def model_touch(tri, rect):
    return R.rect_valid(*rect) and bool(R.tri_touch(tri[0], tri[1], tri[2], tri[3], tri[4], tri[5], *rect))


def test_predicate_has_the_exact_answer(host, pairs):
    assert len(pairs) == 2000
    wrong, yes = [], 0
    for i, (tri, rect) in enumerate(pairs):
        exact = exact_touch(tri, rect)
        yes += exact
        got = (model_touch(tri, rect), lane_touch(host, tri, rect, True), lane_touch(host, tri, rect, False))
        if got != (exact, exact, exact):
            wrong.append((i, exact, got, tri.tolist(), rect.tolist()))
    assert not wrong, (len(wrong), wrong[:3])
    assert 0.3 * len(pairs) <= yes <= 0.7 * len(pairs), yes  # both outcomes, at least 30 % each


def test_one_corner_form_equals_four_corner_form(host, pairs):
    inf = np.inf
    extra = []
    for tri, _ in pairs[::25]:
        for rect in ([-inf, -inf, inf, inf], [-inf, tri[1], tri[0], inf], [tri[0], -inf, inf, tri[1]], [-inf, tri[1], inf, tri[1]], [tri[0], tri[1], tri[0], inf]):
            extra.append((tri, np.array(rect, dtype=F)))
    axis = np.array([4, 4, 8, 4, 4, 9], dtype=F)  # an edge along each axis: a zero difference meets an infinite corner
    extra += [(axis, np.array(rect, dtype=F)) for rect in ([-inf, -inf, inf, inf], [-inf, 0, 5, 5], [5, -inf, 6, 5], [0, 0, inf, inf], [5, 5, 5, inf])]
    differ = [(tri.tolist(), rect.tolist()) for tri, rect in list(pairs) + extra if lane_touch(host, tri, rect, False) != lane_touch(host, tri, rect, True)]
    assert not differ, (len(differ), differ[:3])
    differ = [(tri.tolist(), rect.tolist()) for tri, rect in extra if lane_touch(host, tri, rect, True) != model_touch(tri, rect)]
    assert not differ, (len(differ), differ[:3])


# ---- (d) window is a subset of crossing, crossing grows with the rectangle --------------------------------------------------------
def entries_of(host, f, q, cap=16384):
    g = host_pick_rect(host, f, q, cap=cap)
    assert np.all(g.count <= cap)
    return [set(g.list[i, :g.count[i]].tolist()) for i in range(q.shape[0])], g


def test_window_in_crossing_and_crossing_monotone(host):
    r = R.frame("tiger", 65)
    base = r.queries[(r.kind == "marquee") | (r.kind == "square") | (r.kind == "mid_run")].copy()
    cross = base.copy()
    cross["flags"] &= ~np.uint32(WINDOW)
    win = base.copy()
    win["flags"] |= np.uint32(WINDOW)
    grown = cross.copy()
    grown["x0"] -= F(7.5); grown["y0"] -= F(0.25); grown["x1"] += F(11); grown["y1"] += F(40)
    ec, gc = entries_of(host, r.f, cross)
    ew, _ = entries_of(host, r.f, win)
    eg, gg = entries_of(host, r.f, grown)
    assert all(w <= c for w, c in zip(ew, ec)) and all(c <= g for c, g in zip(ec, eg))
    assert sum(len(w) < len(c) for w, c in zip(ew, ec)) >= 10 and sum(len(c) < len(g) for c, g in zip(ec, eg)) >= 10
    assert sum(len(w) > 0 for w in ew) >= 10
    # the top of a larger crossing selection is at least as high
    height = lambda g: np.where(g.top["mesh"] == NONE, -1, g.top["mesh"].astype(np.int64))  # "none" lies below every mesh
    assert np.all(height(gc) <= height(gg))


# ---- (e) paging ------------------------------------------------------------------------------------------------------------
def test_pages_concatenate(host):
    r = R.frame("tiger", 65)
    f = r.f
    draw = f.meshes["draw"]
    sel = np.nonzero((r.answer.count > R.LIST_CAP) & (r.answer.count <= 400))[0]
    sel = np.concatenate([sel[(r.queries["flags"][sel] & BY_DRAW) != 0][:3], sel[(r.queries["flags"][sel] & BY_DRAW) == 0][:3]])
    assert sel.size == 6
    for i in sel:
        q = r.queries[i:i + 1].copy()
        whole, _ = host_pick_rect(host, f, q, cap=512).list, None
        want = whole[0, :r.answer.count[i]].tolist()
        assert want == r.answer.entries[i].tolist()
        got, pages = [], 0
        while True:
            g = host_pick_rect(host, f, q, cap=R.LIST_CAP)
            page = g.list[0, :min(int(g.count[0]), R.LIST_CAP)].tolist()
            got += page
            pages += 1
            if g.count[0] <= R.LIST_CAP:
                break
            last = page[-1]
            if q["flags"][0] & BY_DRAW:  # the end of the last listed run
                nxt = last + 1
                while nxt < f.nm and draw[nxt] == draw[last]:
                    nxt += 1
            else:
                nxt = last + 1
            q["mesh_begin"][0] = nxt
        assert got == want and pages >= 2, (int(i), pages)


# ---- (f) the infinite rectangle lists every instance that has something to touch ------------------------------------------------------
def test_infinite_rectangle_lists_the_instances(host):
    r = R.frame("tiger", 65)
    f, T = r.f, r.f.tris
    q = np.array([R._q(-np.inf, -np.inf, np.inf, np.inf, flags=BY_DRAW), R._q(-np.inf, -np.inf, np.inf, np.inf, flags=BY_DRAW | SKIP)], dtype=capi.pick_rect_query_dtype)
    ent, g = entries_of(host, f, q)
    draw = f.meshes["draw"]
    first = {}
    for m in range(f.nm - 1, -1, -1):
        first[int(draw[m])] = m  # instances are consecutive in a vgx_cache_submit frame: one run each
    for k, considered in enumerate((T.nondegenerate, T.nondegenerate & ~T.transparent)):
        want = {first[int(d)] for d in np.unique(draw[T.mesh[considered]])}
        assert ent[k] == want, (k, sorted(ent[k] ^ want)[:8])
        assert g.list[k, :g.count[k]].tolist() == sorted(want) and len(want) >= 40
    assert ent[1] <= ent[0]
