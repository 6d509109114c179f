"""vgx_pick: a numpy statement of the specification in include/vgx.h, the frames and query sets the CPU and GPU tests share, and the
conditions those query sets must meet (tests/test_pick_cpu.py: the lane code through libvgx_hosttest.so; tests/test_gpu_pick.py: the
kernels).

The frames are the reference's: oracle.cache_submit over the instances of tests/cache_cull_model.py (imported, not edited). The model
knows nothing of mesh boxes: per query it runs the triangle's own float32 box test and the float64 edge expressions over the
triangles of the frame. To stay quick on frames of millions of triangles it looks only at the triangles of the query's vertical
strip: strip(x) is a monotone function, a triangle is listed in every strip from strip(min x) to strip(max x), and min x <= px <= max x
implies strip(min x) <= strip(px) <= strip(max x), so no triangle that passes the box test is ever left out. Every comparison of
results is exact.
"""
import functools

import numpy as np

import cache_cull_model as CM

capi = CM.capi
oracle = CM.oracle
F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
NSTRIPS = 512


# ---- the specification -----------------------------------------------------------------------------------------------
def edge_exprs(ax, ay, bx, by, cx, cy, px, py):
    """A, e0, e1, e2 in binary64, every difference taken after widening; numpy never fuses a multiply and an add."""
    ax, ay, bx, by, cx, cy, px, py = (np.asarray(v, dtype=F).astype(D) for v in (ax, ay, bx, by, cx, cy, px, py))
    with np.errstate(all="ignore"):
        A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        e0 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        e1 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
        e2 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
    return A, e0, e1, e2


def tri_hit(ax, ay, bx, by, cx, cy, px, py):
    """The point-in-triangle rule on arrays of float32 (px, py may be scalars)."""
    ax, ay, bx, by, cx, cy = (np.asarray(v, dtype=F) for v in (ax, ay, bx, by, cx, cy))
    px, py = F(px), F(py)
    with np.errstate(all="ignore"):
        lox, hix = np.minimum(np.minimum(ax, bx), cx), np.maximum(np.maximum(ax, bx), cx)  # np.minimum hands a NaN on: the compare is false
        loy, hiy = np.minimum(np.minimum(ay, by), cy), np.maximum(np.maximum(ay, by), cy)
        box = (px >= lox) & (px <= hix) & (py >= loy) & (py <= hiy)
        A, e0, e1, e2 = edge_exprs(ax, ay, bx, by, cx, cy, px, py)
        return box & (((A > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((A < 0) & (e0 <= 0) & (e1 <= 0) & (e2 <= 0)))


class Tris:
    """Every triangle of a mesh stream: mesh, t (index within the mesh), the three corners, valid (all indices < num_vertices),
    transparent (a corner of alpha 0), nondegenerate (A != 0 and not NaN), v (global vertex numbers, 0 where invalid)."""


def triangles(pos, color, idx, meshes):
    T = Tris()
    nm = meshes.shape[0]
    nt = (meshes["num_indices"] // 3).astype(np.int64)
    T.mesh = np.repeat(np.arange(nm, dtype=np.int64), nt)
    start = np.concatenate([[0], np.cumsum(nt)])[:-1]
    T.t = np.arange(int(nt.sum()), dtype=np.int64) - np.repeat(start, nt)
    at = meshes["first_index"].astype(np.int64)[T.mesh] + 3 * T.t
    local = np.stack([idx[at + k].astype(np.int64) for k in range(3)], axis=1) if T.t.size else np.zeros((0, 3), dtype=np.int64)
    T.valid = (local < meshes["num_vertices"].astype(np.int64)[T.mesh][:, None]).all(axis=1)
    T.v = np.where(T.valid[:, None], meshes["first_vertex"].astype(np.int64)[T.mesh][:, None] + local, 0)
    p = np.ascontiguousarray(pos, dtype=F).reshape(-1, 2)
    if p.shape[0] == 0:
        p = np.zeros((1, 2), dtype=F)
        color = np.zeros(1, dtype=np.uint32)
    T.a, T.b, T.c = p[T.v[:, 0]], p[T.v[:, 1]], p[T.v[:, 2]]
    T.transparent = ((np.asarray(color, dtype=np.uint32)[T.v] >> 24) == 0).any(axis=1)
    A = edge_exprs(T.a[:, 0], T.a[:, 1], T.b[:, 0], T.b[:, 1], T.c[:, 0], T.c[:, 1], 0, 0)[0]
    T.nondegenerate = T.valid & (A != 0) & ~np.isnan(A)
    # the strips (see the module text). Triangles with a NaN corner can pass no box test and are left out
    with np.errstate(all="ignore"):
        lox = np.minimum(np.minimum(T.a[:, 0], T.b[:, 0]), T.c[:, 0])
        hix = np.maximum(np.maximum(T.a[:, 0], T.b[:, 0]), T.c[:, 0])
    use = T.valid & ~np.isnan(lox) & ~np.isnan(hix)
    fin = use & np.isfinite(lox) & np.isfinite(hix)
    T.x0 = float(lox[fin].min()) if fin.any() else 0.0
    x1 = float(hix[fin].max()) if fin.any() else 1.0
    T.cell = max((x1 - T.x0) / NSTRIPS, 1e-30)
    ids = np.nonzero(use)[0]
    s0, s1 = strip(T, lox[ids]), strip(T, hix[ids])
    cnt = s1 - s0 + 1
    rep = np.repeat(ids, cnt)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    st = np.repeat(s0, cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt))
    order = np.argsort(st, kind="stable")  # stable: triangles stay ascending inside a strip
    T.strip_tris = rep[order]
    T.strip_begin = np.searchsorted(st[order], np.arange(NSTRIPS + 1))
    return T


def strip(T, x):
    """Monotone in x: float32 -> float64 exactly, a subtraction, a division by a positive number, floor and clip."""
    with np.errstate(all="ignore"):
        return np.clip(np.floor((np.asarray(x, dtype=F).astype(D) - T.x0) / T.cell), 0, NSTRIPS - 1).astype(np.int64)


def containing(T, x, y, flags=0, mesh_end=NONE):
    """Global triangle numbers (ascending = painter's order) of the triangles of meshes < mesh_end that the point hits."""
    x, y = F(x), F(y)
    if np.isnan(x) or np.isnan(y):
        return np.zeros(0, dtype=np.int64)
    s = int(strip(T, x))
    ids = T.strip_tris[T.strip_begin[s]:T.strip_begin[s + 1]]
    ids = ids[T.mesh[ids] < mesh_end]
    if flags & capi.PICK_SKIP_TRANSPARENT:
        ids = ids[~T.transparent[ids]]
    a, b, c = T.a[ids], T.b[ids], T.c[ids]
    return ids[tri_hit(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1], x, y)]


def pick(T, meshes, queries):
    """hits (capi.pick_hit_dtype) of the specification; also the number of distinct containing meshes per query."""
    hits = np.full(queries.shape[0], NONE, dtype=np.uint32).repeat(4).view(capi.pick_hit_dtype)
    depth = np.zeros(queries.shape[0], dtype=np.int64)
    for q in range(queries.shape[0]):
        ids = containing(T, queries["x"][q], queries["y"][q], int(queries["flags"][q]), int(queries["mesh_end"][q]))
        if ids.size:
            g = int(ids[-1])  # ascending in (mesh, t): the last one is the largest mesh's largest triangle
            m = int(T.mesh[g])
            hits[q] = (m, int(T.t[g]), int(meshes["draw"][m]), int(meshes["subpath_kind"][m]))
            depth[q] = np.unique(T.mesh[ids]).size
    return hits, depth


# ---- frames -----------------------------------------------------------------------------------------------------------
CASES = (("tiger", 1), ("tiger", 65), ("tiger", 257), ("walk", 1), ("walk", 65), ("empty", 65))
BIG = ("tiger", 257)  # the frame the query-set conditions are asserted on


class Frame:
    pass


@functools.lru_cache(maxsize=None)
def frame(name, n):
    """The reference's frame of the finite-matrix instances of cache_cull_model.scene (a non-finite matrix gives NaN positions, whose
    boxes are unspecified), its triangles, its query set and the model's answer: computed once per session, never changed."""
    empty = name == "empty"
    c, inst, _, _ = CM.scene("tiger" if empty else name, n)
    f = Frame()
    f.case, f.key = c, (name, n)
    f.inst = inst[CM.finite_mask(inst)]
    fr = oracle.cache_submit(c.cache, f.inst)
    f.pos, f.color, f.idx = fr.pos, fr.color, fr.idx
    f.meshes = CM.with_empty_meshes(fr.meshes)[0] if empty else fr.meshes
    f.nm, f.nv, f.ni = f.meshes.shape[0], fr.pos.shape[0], fr.idx.shape[0]
    f.tris = triangles(f.pos, f.color, f.idx, f.meshes)
    f.queries, f.kind = make_queries(f)
    f.hits, f.depth = pick(f.tris, f.meshes, f.queries)
    return f


# ---- query sets -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_local_points(c, want=12):
    """Local-space points of the cache that at least three of its meshes contain (interior centroids, the model counting)."""
    T = triangles(c.cache.pos, c.cache.color, c.cache.idx, c.cache.meshes)
    rs = np.random.RandomState(2)
    inner = np.nonzero(T.nondegenerate & ~T.transparent)[0]
    out = []
    for g in rs.permutation(inner)[:600]:
        cen = ((T.a[g].astype(D) + T.b[g] + T.c[g]) / 3.0).astype(F)
        if np.unique(T.mesh[containing(T, cen[0], cen[1])]).size >= 3:
            out.append((cen[0], cen[1]))
            if len(out) == want:
                break
    return out


def make_queries(f, seed=11):
    """(queries, kind) with kind in 'vertex', 'outside', 'centroid', 'stacked', 'nan', 'inf', 'end0'. See check_query_conditions."""
    T, c = f.tris, f.case
    rs = np.random.RandomState(seed + f.nm)
    pts, kinds = [], []
    # every 997th vertex of the frame that belongs to a non-degenerate triangle
    in_nd = np.zeros(max(f.nv, 1), dtype=bool)
    in_nd[T.v[T.nondegenerate].reshape(-1)] = True
    for v in range(0, f.nv, 997):
        if in_nd[v]:
            pts.append((f.pos[v, 0], f.pos[v, 1]))
            kinds.append("vertex")
    # triangle centroids rounded to binary32: the model decides
    nd = np.nonzero(T.nondegenerate)[0]
    for g in rs.choice(nd, size=min(100, nd.size), replace=False) if nd.size else []:
        cen = (T.a[g].astype(D) + T.b[g].astype(D) + T.c[g].astype(D)) / 3.0
        pts.append((F(cen[0]), F(cen[1])))
        kinds.append("centroid")
    # over the middle of whole-drawing instances, where several of the drawing's meshes lie on top of each other
    whole = np.nonzero(f.inst["num_meshes"] == c.nm)[0]
    deep = deep_local_points(c)
    for k in range(40 if whole.size and len(deep) else 0):
        x, y = CM.xform(f.inst["mtx"][whole[k % whole.size]], *deep[(k // max(whole.size, 1) + k) % len(deep)])
        pts.append((x, y))
        kinds.append("stacked")
    # outside the frame's box: at least an eighth of everything, so that the misses keep their share
    lo, hi = f.pos.min(axis=0).astype(D), f.pos.max(axis=0).astype(D)
    ext = float(max(hi[0] - lo[0], hi[1] - lo[1], 1.0))
    for k in range((len(pts) + 3) // 8 + 8):
        side, u, d = k % 4, rs.uniform(-0.2, 1.2), rs.uniform(0.001, 0.5) * ext
        x = lo[0] + u * (hi[0] - lo[0]) if side < 2 else (lo[0] - d if side == 2 else hi[0] + d)
        y = (lo[1] - d if side == 0 else hi[1] + d) if side < 2 else lo[1] + u * (hi[1] - lo[1])
        pts.append((F(x), F(y)))
        kinds.append("outside")
    q = np.zeros(len(pts) + 3, dtype=capi.pick_query_dtype)
    q["mesh_end"] = NONE
    q["x"][:len(pts)] = [p[0] for p in pts]
    q["y"][:len(pts)] = [p[1] for p in pts]
    n = len(pts)
    v0 = pts[0] if kinds and kinds[0] == "vertex" else (F(0), F(0))
    q["x"][n], q["y"][n] = np.nan, v0[1]
    q["x"][n + 1], q["y"][n + 1] = np.inf, -np.inf
    q["x"][n + 2], q["y"][n + 2], q["mesh_end"][n + 2] = v0[0], v0[1], 0  # a vertex that hits, behind mesh_end = 0
    kinds += ["nan", "inf", "end0"]
    order = rs.permutation(q.shape[0])  # the kinds mixed through the 256-query calls
    return q[order], np.array(kinds, dtype=object)[order]


def check_query_conditions(f):
    """On the model's output alone, before the product's answer is looked at."""
    hit = f.hits["mesh"] != NONE
    k = f.kind
    assert hit[k == "vertex"].all(), "a vertex of a non-degenerate triangle hits it"
    assert not hit[k == "outside"].any()
    assert not hit[(k == "nan") | (k == "inf") | (k == "end0")].any()
    assert int((k == "nan").sum()) == 1 and int((k == "inf").sum()) == 1 and int((k == "end0").sum()) == 1
    if f.key == BIG:
        assert int((k == "vertex").sum()) >= 100 and int((k == "centroid").sum()) == 100
        assert int(((k == "stacked") & (f.depth >= 2)).sum()) >= 20, int(((k == "stacked") & (f.depth >= 2)).sum())
        assert int(hit.sum()) * 3 >= hit.size and int((~hit).sum()) * 10 >= hit.size, (int(hit.sum()), hit.size)


def chunks(n, size=capi.PICK_MAX_QUERIES):
    return [(a, min(a + size, n)) for a in range(0, n, size)]
