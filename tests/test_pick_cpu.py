"""CPU: the lane code of vgx_pick (csrc/vgx_pick.h through libvgx_hosttest.so: vgxt_pick, a plain loop over meshes and triangles)
against the numpy statement of the specification (tests/pick_model.py) on frames written by the reference, and the model's predicate
against exact rational arithmetic. Exact everywhere; the GPU suite (tests/test_gpu_pick.py) makes the same comparison on the kernels."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import pick_model as P

capi = P.capi
F = np.float32
NONE = P.NONE


@pytest.fixture(scope="module")
def host():
    path = os.path.join(P.CM.ROOT, "vg-renderer_amd", "libvgx_hosttest.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(path)
    lib.vgxt_pick.restype = C.c_int
    lib.vgxt_pick.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.vgxt_mesh_bounds.restype = None
    lib.vgxt_mesh_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def host_pick(host, pos, color, idx, meshes, queries, with_bounds=False, guard=2):
    """vgxt_pick in calls of at most 256 queries, each into a pattern-filled array whose entries behind nqueries must stay."""
    pos, color = np.ascontiguousarray(pos, dtype=F), np.ascontiguousarray(color, dtype=np.uint32)
    idx, meshes = np.ascontiguousarray(idx, dtype=np.uint16), np.ascontiguousarray(meshes)
    d = capi.CacheDesc(pos.ctypes.data, color.ctypes.data, idx.ctypes.data, meshes.ctypes.data, meshes.shape[0], pos.shape[0], idx.shape[0])
    mb = None
    if with_bounds:
        mb = np.zeros((max(meshes.shape[0], 1), 4), dtype=F)
        host.vgxt_mesh_bounds(pos.ctypes.data, meshes.ctypes.data, meshes.shape[0], mb.ctypes.data)
    out = np.zeros(queries.shape[0], dtype=capi.pick_hit_dtype)
    for a, b in P.chunks(queries.shape[0]):
        q = np.ascontiguousarray(queries[a:b])
        h = np.full((b - a + guard) * 4, 0x5A5A5A5A, dtype=np.uint32)
        assert host.vgxt_pick(C.byref(d), None if mb is None else mb.ctypes.data, q.ctypes.data, b - a, h.ctypes.data) == capi.VGX_OK
        assert np.all(h[(b - a) * 4:] == 0x5A5A5A5A)
        out[a:b] = h[:(b - a) * 4].view(capi.pick_hit_dtype)
    return out


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,n", P.CASES)
def test_lane_code_equals_model(host, name, n):
    f = P.frame(name, n)
    P.check_query_conditions(f)
    got = host_pick(host, f.pos, f.color, f.idx, f.meshes, f.queries)
    assert same(got, f.hits), np.nonzero(got.view(np.uint32).reshape(-1, 4) != f.hits.view(np.uint32).reshape(-1, 4))[0][:8]
    # with the boxes handed in instead of computed by the call: the same bytes
    assert same(host_pick(host, f.pos, f.color, f.idx, f.meshes, f.queries, with_bounds=True), got)


def exact_hit(a, b, c, p):
    """The rule of include/vgx.h over the rationals: every binary32 value is a rational number, nothing rounds."""
    (ax, ay), (bx, by), (cx, cy), (px, py) = [tuple(Fraction(float(v)) for v in pt) for pt in (a, b, c, p)]
    if not (min(ax, bx, cx) <= px <= max(ax, bx, cx) and min(ay, by, cy) <= py <= max(ay, by, cy)):
        return False
    A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    e = [(bx - ax) * (py - ay) - (by - ay) * (px - ax), (cx - bx) * (py - by) - (cy - by) * (px - bx), (ax - cx) * (py - cy) - (ay - cy) * (px - cx)]
    return (A > 0 and all(v >= 0 for v in e)) or (A < 0 and all(v <= 0 for v in e))


def test_predicate_has_the_exact_sign():
    """The claim of include/vgx.h, checked and not assumed: on the Tiger frame's own triangles the binary64 expressions give the
    answer exact rational arithmetic gives, for points that are vertices, points on edges (midpoints that binary32 represents
    exactly) and random points inside the triangle's box."""
    f = P.frame("tiger", 65)
    T = f.tris
    rs = np.random.RandomState(3)
    tri = rs.choice(np.nonzero(T.valid)[0], size=1500, replace=False)
    pairs = []
    for g in tri:
        a, b, c = T.a[g], T.b[g], T.c[g]
        pairs.append((g, a if g % 3 == 0 else (b if g % 3 == 1 else c), "vertex"))
        u, v = ((a, b), (b, c), (c, a))[g % 3]
        mid = ((u.astype(np.float64) + v.astype(np.float64)) / 2.0)
        if np.array_equal(mid.astype(F).astype(np.float64), mid):
            pairs.append((g, mid.astype(F), "edge"))
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        pairs.append((g, (lo + (hi - lo) * rs.uniform(0, 1, 2).astype(F)).astype(F), "random"))
    kinds = [k for _, _, k in pairs]
    assert len(pairs) >= 3000 and kinds.count("edge") >= 100, (len(pairs), kinds.count("edge"))
    wrong, hits = [], {"vertex": 0, "edge": 0, "random": 0}
    for g, p, kind in pairs:
        a, b, c = T.a[g], T.b[g], T.c[g]
        model = bool(P.tri_hit(a[0], a[1], b[0], b[1], c[0], c[1], p[0], p[1]))
        exact = exact_hit(a, b, c, p)
        hits[kind] += exact
        if model != exact:
            wrong.append((int(g), kind, model, exact))
    assert not wrong, (len(wrong), wrong[:5])
    # the geometric guarantees, from the exact side: a vertex or an edge point of a triangle with A != 0 hits it
    nd = {int(g) for g in tri if T.nondegenerate[g]}
    for g, p, kind in pairs:
        if kind != "random" and int(g) in nd:
            assert exact_hit(T.a[g], T.b[g], T.c[g], p), (int(g), kind)
    assert hits["random"] > 100  # both outcomes among the random points
    assert hits["random"] < kinds.count("random")


def test_click_through_walks_the_stack(host):
    """mesh_end = the previous hit's mesh: the picks enumerate the model's containing meshes from the top down, then "none"."""
    f = P.frame("tiger", 257)
    deep = np.nonzero((f.kind == "stacked") & (f.depth >= 2))[0][:6]
    assert deep.size == 6
    for qi in deep:
        x, y = f.queries["x"][qi], f.queries["y"][qi]
        want = np.unique(f.tris.mesh[P.containing(f.tris, x, y)])[::-1].tolist()
        got, end = [], NONE
        for _ in range(len(want) + 1):
            q = np.zeros(1, dtype=capi.pick_query_dtype)
            q["x"], q["y"], q["mesh_end"] = x, y, end
            h = host_pick(host, f.pos, f.color, f.idx, f.meshes, q)[0]
            if h["mesh"] == NONE:
                assert tuple(h) == (NONE, NONE, NONE, NONE)
                break
            assert h["draw"] == f.meshes["draw"][h["mesh"]] and h["subpath_kind"] == f.meshes["subpath_kind"][h["mesh"]]
            got.append(int(h["mesh"]))
            end = int(h["mesh"])
        assert got == want and len(got) >= 2


def test_skip_transparent(host):
    f = P.frame("tiger", 65)
    q = f.queries.copy()
    q["flags"] = capi.PICK_SKIP_TRANSPARENT
    want, _ = P.pick(f.tris, f.meshes, q)
    got = host_pick(host, f.pos, f.color, f.idx, f.meshes, q)
    assert same(got, want)
    hit, plain = got["mesh"] != NONE, f.hits["mesh"] != NONE
    assert not np.any(hit & ~plain) and 0 < int(hit.sum())  # a subset of the unflagged hits
    # every reported triangle has three non-zero alphas
    first = np.concatenate([[0], np.cumsum((f.meshes["num_indices"] // 3).astype(np.int64))])
    g = first[got["mesh"][hit].astype(np.int64)] + got["triangle"][hit].astype(np.int64)
    assert not f.tris.transparent[g].any()
    assert ((f.color[f.tris.v[g]] >> 24) != 0).all()
    # the flag does drop something: some unflagged top hit was a fringe triangle
    assert int((plain & ~same_rows(got, f.hits)).sum()) > 0
    # a query in a fill's interior (a centroid of a triangle without a transparent corner) still hits
    inner = np.nonzero(f.tris.nondegenerate & ~f.tris.transparent)[0][::997][:50]
    qi = np.zeros(inner.size, dtype=capi.pick_query_dtype)
    cen = (f.tris.a[inner].astype(np.float64) + f.tris.b[inner] + f.tris.c[inner]) / 3.0
    qi["x"], qi["y"], qi["mesh_end"], qi["flags"] = cen[:, 0].astype(F), cen[:, 1].astype(F), NONE, capi.PICK_SKIP_TRANSPARENT
    gi = host_pick(host, f.pos, f.color, f.idx, f.meshes, qi)
    wi, _ = P.pick(f.tris, f.meshes, qi)
    assert same(gi, wi) and int((gi["mesh"] != NONE).sum()) >= inner.size // 2


def same_rows(a, b):
    return (a.view(np.uint32).reshape(-1, 4) == b.view(np.uint32).reshape(-1, 4)).all(axis=1)


def malformed(f):
    """Hand-made tables on the real streams of a frame: an index >= num_vertices, num_indices % 3 != 0, a mesh of 0 indices."""
    out = []
    big = int(np.argmax(f.meshes["num_indices"]))
    # an index past the mesh's own vertices: num_vertices cut down, so that some triangles point behind it
    m = f.meshes.copy()
    m["num_vertices"][big] = max(3, int(m["num_vertices"][big]) // 2)
    out.append(("index", m))
    m = f.meshes.copy()
    m["num_indices"][big] -= 1  # the last triangle is now a remainder of two indices
    m["num_indices"][(big + 1) % f.nm] -= 2
    out.append(("remainder", m))
    m = f.meshes.copy()
    m["num_indices"][big] = 0
    out.append(("noindices", m))
    return out


def malformed_queries(f):
    """Centroids of triangles of the two meshes malformed() damages (the last triangle of each among them), in front of a slice of the
    frame's own set."""
    big = int(np.argmax(f.meshes["num_indices"]))
    T = f.tris
    g = np.concatenate([np.nonzero((T.mesh == m) & T.nondegenerate)[0] for m in (big, (big + 1) % f.nm)])
    g = np.unique(np.concatenate([g[::max(1, g.size // 150)], [np.nonzero(T.mesh == big)[0][-1], np.nonzero(T.mesh == (big + 1) % f.nm)[0][-1]]]))
    q = np.zeros(g.size, dtype=capi.pick_query_dtype)
    cen = (T.a[g].astype(np.float64) + T.b[g] + T.c[g]) / 3.0
    q["x"], q["y"], q["mesh_end"] = cen[:, 0].astype(F), cen[:, 1].astype(F), NONE
    return np.concatenate([q, f.queries[:64]])


def test_malformed_tables(host):
    f = P.frame("tiger", 65)
    q = malformed_queries(f)
    sound, _ = P.pick(f.tris, f.meshes, q)
    for what, meshes in malformed(f):
        T = P.triangles(f.pos, f.color, f.idx, meshes)
        assert what != "index" or int((~T.valid).sum()) > 0
        want, _ = P.pick(T, meshes, q)
        assert not same(want, sound), what  # the damage is where the queries look
        got = host_pick(host, f.pos, f.color, f.idx, meshes, q)
        assert same(got, want), what
        assert same(host_pick(host, f.pos, f.color, f.idx, meshes, q, with_bounds=True), got), what


def test_host_argument_checks(host):
    f = P.frame("tiger", 1)
    d = capi.CacheDesc(f.pos.ctypes.data, f.color.ctypes.data, f.idx.ctypes.data, f.meshes.ctypes.data, f.nm, f.nv, f.ni)
    q = np.zeros(257, dtype=capi.pick_query_dtype)
    h = np.zeros(257, dtype=capi.pick_hit_dtype)
    assert host.vgxt_pick(C.byref(d), None, q.ctypes.data, 257, h.ctypes.data) == capi.VGX_E_RANGE
    assert host.vgxt_pick(C.byref(d), None, None, 1, h.ctypes.data) == capi.VGX_E_INVALID_ARG
    assert host.vgxt_pick(C.byref(d), None, None, 0, None) == capi.VGX_OK
    d0 = capi.CacheDesc(None, None, None, None, 0, 0, 0)
    h[:] = (1, 2, 3, 4)
    assert host.vgxt_pick(C.byref(d0), None, q.ctypes.data, 3, h.ctypes.data) == capi.VGX_OK
    assert np.all(h[:3].view(np.uint32) == NONE) and tuple(h[3]) == (1, 2, 3, 4)
