"""vgx_pick_rect: a numpy statement of the specification in include/vgx.h, the query sets the CPU and GPU tests share, and the conditions
those query sets must meet (tests/test_pick_rect_cpu.py: the lane code through libvgx_hosttest.so; tests/test_gpu_pick_rect.py: the
kernels).

The frames, their triangles and the mesh boxes are those of tests/pick_model.py and tests/cache_cull_model.py (imported, not edited). The
model knows nothing of the mesh-box prefilter: per query it runs the binary32 box overlap over ALL triangles of the frame at once, then
the binary64 edge expressions at the four corners of the rectangle on what is left -- the four-corner form of the header, whatever the
product evaluates. Every comparison of results is exact.
"""
import functools

import numpy as np

import pick_model as P

CM = P.CM
capi = P.capi
F = np.float32
D = np.float64
NONE = P.NONE
SKIP, WINDOW, BY_DRAW = capi.PICK_SKIP_TRANSPARENT, capi.PICK_RECT_WINDOW, capi.PICK_RECT_BY_DRAW
CASES = (("tiger", 65), ("tiger", 257), ("walk", 65), ("empty", 65))
BIG = ("tiger", 257)  # the frame the query-set conditions are asserted on
LIST_CAP = 8          # the capacity the conditions speak of
TOL = 2.0             # half the side of a tolerance square


# ---- the specification -----------------------------------------------------------------------------------------------
def rect_valid(x0, y0, x1, y1):
    return bool(F(x0) <= F(x1)) and bool(F(y0) <= F(y1))  # a NaN fails


def tri_touch(ax, ay, bx, by, cx, cy, x0, y0, x1, y1):
    """Steps 2 to 4 on arrays of float32 corners and one rectangle: the box overlap, A, and per edge "some corner of R passes"."""
    ax, ay, bx, by, cx, cy = (np.asarray(v, dtype=F) for v in (ax, ay, bx, by, cx, cy))
    x0, y0, x1, y1 = F(x0), F(y0), F(x1), F(y1)
    with np.errstate(all="ignore"):
        lox, hix = np.minimum(np.minimum(ax, bx), cx), np.maximum(np.maximum(ax, bx), cx)
        loy, hiy = np.minimum(np.minimum(ay, by), cy), np.maximum(np.maximum(ay, by), cy)
        box = (x1 >= lox) & (x0 <= hix) & (y1 >= loy) & (y0 <= hiy)
        passed = np.zeros((3,) + ax.shape, dtype=bool)
        for px, py in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
            A, e0, e1, e2 = P.edge_exprs(ax, ay, bx, by, cx, cy, px, py)  # vgx_pick's expressions: e_k is edge k at the corner
            for k, e in enumerate((e0, e1, e2)):
                passed[k] |= ((A > 0) & (e >= 0)) | ((A < 0) & (e <= 0))
        return box & passed.all(axis=0)


def tri_boxes(T):
    if not hasattr(T, "rect_boxes"):
        with np.errstate(all="ignore"):
            T.rect_boxes = (np.minimum(np.minimum(T.a[:, 0], T.b[:, 0]), T.c[:, 0]), np.minimum(np.minimum(T.a[:, 1], T.b[:, 1]), T.c[:, 1]),
                            np.maximum(np.maximum(T.a[:, 0], T.b[:, 0]), T.c[:, 0]), np.maximum(np.maximum(T.a[:, 1], T.b[:, 1]), T.c[:, 1]))
    return T.rect_boxes


def touching(T, q):
    """Global numbers (ascending in (mesh, t)) of the considered triangles of the query's range that touch its rectangle; nm unknown here:
    the caller's range clips mesh_end."""
    x0, y0, x1, y1 = F(q["x0"]), F(q["y0"]), F(q["x1"]), F(q["y1"])
    if not rect_valid(x0, y0, x1, y1) or int(q["reserved"]) != 0:
        return np.zeros(0, dtype=np.int64)
    # the valid triangles of the whole frame that touch this rectangle: the same for every range and flag word, so kept per rectangle
    memo = T.__dict__.setdefault("rect_memo", {})
    key = (x0.tobytes(), y0.tobytes(), x1.tobytes(), y1.tobytes())
    if key not in memo:
        lox, loy, hix, hiy = tri_boxes(T)
        with np.errstate(all="ignore"):
            ids = np.nonzero(T.valid & (x1 >= lox) & (x0 <= hix) & (y1 >= loy) & (y0 <= hiy))[0]
        a, b, c = T.a[ids], T.b[ids], T.c[ids]
        memo[key] = ids[tri_touch(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1], x0, y0, x1, y1)]
    ids = memo[key]
    ids = ids[(T.mesh[ids] >= int(q["mesh_begin"])) & (T.mesh[ids] < int(q["mesh_end"]))]
    if int(q["flags"]) & SKIP:
        ids = ids[~T.transparent[ids]]
    return ids


class Answer:
    """top (capi.pick_hit_dtype [nq]), count (uint32 [nq]), entries (per query the full ascending list, uint32)."""


def pick_rect(T, meshes, boxes, queries):
    nq, nm = queries.shape[0], meshes.shape[0]
    r = Answer()
    r.top = np.full(nq, NONE, dtype=np.uint32).repeat(4).view(capi.pick_hit_dtype)
    r.count = np.zeros(nq, dtype=np.uint32)
    r.entries = []
    draw = meshes["draw"]
    for i in range(nq):
        q = queries[i]
        fl = int(q["flags"])
        b, e = int(q["mesh_begin"]), min(int(q["mesh_end"]), nm)
        ids = touching(T, q)
        valid = rect_valid(q["x0"], q["y0"], q["x1"], q["y1"]) and int(q["reserved"]) == 0
        if not valid or b >= e:
            r.entries.append(np.zeros(0, dtype=np.uint32))
            continue
        touch = np.zeros(nm, dtype=bool)
        touch[T.mesh[ids]] = True
        with np.errstate(all="ignore"):
            inside = (boxes[:, 0] >= F(q["x0"])) & (boxes[:, 2] <= F(q["x1"])) & (boxes[:, 1] >= F(q["y0"])) & (boxes[:, 3] <= F(q["y1"]))
        ms = np.arange(b, e)
        if fl & BY_DRAW:
            heads = np.nonzero(np.concatenate([[True], draw[b + 1:e] != draw[b:e - 1]]))[0]  # runs of the RANGE
            any_touch = np.logical_or.reduceat(touch[b:e], heads)
            all_inside = np.logical_and.reduceat(inside[b:e], heads)
            sel = any_touch & (all_inside if fl & WINDOW else True)
            entries = (b + heads[sel]).astype(np.uint32)
            run_sel = np.repeat(sel, np.diff(np.concatenate([heads, [e - b]])))
            tops = ms[touch[b:e] & run_sel]
        else:
            sel = touch[b:e] & (inside[b:e] if fl & WINDOW else True)
            entries = ms[sel].astype(np.uint32)
            tops = ms[sel]
        r.entries.append(entries)
        r.count[i] = entries.size
        if tops.size:
            m = int(tops[-1])
            g = int(ids[T.mesh[ids] == m][-1])
            r.top[i] = (m, int(T.t[g]), int(draw[m]), int(meshes["subpath_kind"][m]))
    return r


def lists(r, cap, pattern):
    """What out->list holds after a call with list_cap = cap on an array filled with `pattern`."""
    out = np.full((len(r.entries), cap), pattern, dtype=np.uint32)
    for i, e in enumerate(r.entries):
        out[i, :min(e.size, cap)] = e[:cap]
    return out


# ---- frames and query sets ---------------------------------------------------------------------------------------------------
class RectFrame:
    pass


def _q(x0, y0, x1, y1, flags=0, begin=0, end=NONE, reserved=0):
    return (F(x0), F(y0), F(x1), F(y1), begin, end, flags, reserved)


def make_queries(f, seed=17):
    """(queries, kind, pair): kind names what a query is; pair[i] is the query it is compared with in check_query_conditions (-1: none)."""
    T = f.tris
    rs = np.random.RandomState(seed + f.nm)
    rows, kinds, pairs = [], [], []

    def add(row, kind, pair=-1):
        rows.append(row)
        kinds.append(kind)
        pairs.append(pair)
        return len(rows) - 1

    # degenerate rectangles at the frame's point queries, hits and misses: vgx_pick's test
    for k in rs.permutation(f.queries.shape[0])[:40]:
        x, y = f.queries["x"][k], f.queries["y"][k]
        add(_q(x, y, x, y, flags=int(f.queries["flags"][k]), end=int(f.queries["mesh_end"][k])), "point")
    # tolerance squares around vertices
    for v in rs.permutation(f.nv)[:30] if f.nv else []:
        x, y = f.pos[v]
        add(_q(x - TOL, y - TOL, x + TOL, y + TOL, flags=(0, SKIP, BY_DRAW)[int(v) % 3]), "square")
    # ... and around points 1.5 units off a triangle's edge that the point test misses, with the degenerate rectangle at their centre
    nd = np.nonzero(T.nondegenerate)[0]
    found = 0
    for g in rs.permutation(nd)[:400]:
        u, v = T.a[g].astype(D), T.b[g].astype(D)
        d = v - u
        n = np.array([d[1], -d[0]]) / max(np.hypot(d[0], d[1]), 1e-30)
        for s in (1.0, -1.0):
            p = ((u + v) / 2.0 + s * 1.5 * n).astype(F)
            if found < 10 and np.isfinite(p).all() and P.containing(T, p[0], p[1]).size == 0:
                c = add(_q(p[0], p[1], p[0], p[1]), "off_point")
                add(_q(p[0] - TOL, p[1] - TOL, p[0] + TOL, p[1] + TOL), "off_square", c)
                found += 1
                break
    # marquees of 1/64, 1/16, 1/4 and all of the frame's box, each under all eight flag combinations
    lo = f.pos.min(axis=0).astype(D) if f.nv else np.zeros(2)
    hi = f.pos.max(axis=0).astype(D) if f.nv else np.ones(2)
    ext = hi - lo
    for frac, cx, cy in ((8, 0.30, 0.30), (8, 0.55, 0.45), (4, 0.30, 0.35), (4, 0.60, 0.55), (2, 0.35, 0.35), (2, 0.60, 0.60), (1, 0.5, 0.5)):
        w = ext / frac
        c = lo + ext * (cx, cy)
        r = (c[0] - w[0] / 2, c[1] - w[1] / 2, c[0] + w[0] / 2, c[1] + w[1] / 2)
        base = len(rows)
        for fl in range(8):
            # pair: the same rectangle without WINDOW (bit 1); the BY_DRAW comparison finds its partner as pair - or + 4
            add(_q(*r, flags=fl), "marquee", base + (fl & ~WINDOW) if fl & WINDOW else -1)
    # a side exactly on a vertex coordinate, touching from outside: the frame's extreme vertices, and a corner on some vertex
    if f.nv:
        for axis, side in ((0, 0), (0, 1), (1, 0), (1, 1)):
            v = int(np.argmin(f.pos[:, axis]) if side == 0 else np.argmax(f.pos[:, axis]))
            x, y = f.pos[v]
            if axis == 0:
                add(_q(x - 10 if side == 0 else x, y - 1, x if side == 0 else x + 10, y + 1), "on_side")
            else:
                add(_q(x - 1, y - 10 if side == 0 else y, x + 1, y if side == 0 else y + 10), "on_side")
        in_nd = np.unique(T.v[T.nondegenerate].reshape(-1))
        for v in rs.permutation(in_nd)[:4]:
            x, y = f.pos[v]
            add(_q(x - 3, y - 3, x, y), "on_corner")
    # strictly inside one large triangle: no corner of either shape lies in the other's box corners
    if nd.size:
        A = np.abs(P.edge_exprs(T.a[nd, 0], T.a[nd, 1], T.b[nd, 0], T.b[nd, 1], T.c[nd, 0], T.c[nd, 1], 0, 0)[0])
        g = int(nd[np.argmax(A)])
        cen = (T.a[g].astype(D) + T.b[g] + T.c[g]) / 3.0
        lo3, hi3 = np.minimum(np.minimum(T.a[g], T.b[g]), T.c[g]).astype(D), np.maximum(np.maximum(T.a[g], T.b[g]), T.c[g]).astype(D)
        h = (hi3 - lo3) / 64.0
        add(_q(cen[0] - h[0], cen[1] - h[1], cen[0] + h[0], cen[1] + h[1], begin=int(T.mesh[g]), end=int(T.mesh[g]) + 1), "in_triangle")
    add(_q(-np.inf, -np.inf, np.inf, np.inf), "infinite")
    add(_q(-np.inf, -np.inf, np.inf, np.inf, flags=BY_DRAW | WINDOW), "infinite")
    # nothing selected: inverted, NaN, outside the frame, an empty range, a reserved word
    add(_q(hi[0], lo[1], lo[0], hi[1]), "inverted")
    add(_q(lo[0], hi[1], hi[0], lo[1], flags=BY_DRAW), "inverted")
    add(_q(np.nan, lo[1], hi[0], hi[1]), "nan")
    add(_q(lo[0], lo[1], hi[0], np.nan, flags=WINDOW), "nan")
    big = float(max(ext.max(), 1.0))
    for k in range(6):
        dx, dy = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1))[k]
        c = (lo + hi) / 2 + np.array([dx, dy]) * (ext / 2 + 0.3 * big)
        add(_q(c[0] - 0.2 * big, c[1] - 0.2 * big, c[0] + 0.2 * big, c[1] + 0.2 * big, flags=k & 7), "outside")
    add(_q(lo[0], lo[1], hi[0], hi[1], begin=f.nm // 2, end=f.nm // 2), "empty_range")
    add(_q(lo[0], lo[1], hi[0], hi[1], begin=f.nm // 2 + 1, end=f.nm // 2, flags=BY_DRAW), "empty_range")
    add(_q(lo[0], lo[1], hi[0], hi[1], reserved=1), "reserved")
    # ranges that start and end in the middle of a run, over the whole frame's box
    draw = f.meshes["draw"]
    heads = np.nonzero(np.concatenate([[True], draw[1:] != draw[:-1]]))[0] if f.nm else np.zeros(0, dtype=np.int64)
    length = np.diff(np.concatenate([heads, [f.nm]]))
    long_runs = np.nonzero(length >= 3)[0]
    for k in range(min(4, long_runs.size // 2)):
        r0, r1 = long_runs[k], long_runs[long_runs.size - 1 - k]
        if r0 >= r1:
            break
        begin, end = int(heads[r0] + length[r0] // 2), int(heads[r1] + (length[r1] + 1) // 2)
        for fl in (BY_DRAW, BY_DRAW | WINDOW, 0)[:3 if k < 2 else 2]:
            add(_q(lo[0], lo[1], hi[0], hi[1], flags=fl, begin=begin, end=end), "mid_run")
    q = np.array(rows, dtype=capi.pick_rect_query_dtype)
    assert q.shape[0] <= 3 * capi.PICK_RECT_MAX_QUERIES, q.shape[0]
    order = rs.permutation(q.shape[0])  # the kinds mixed inside a call
    inv = np.argsort(order)
    pair = np.array(pairs, dtype=np.int64)
    return q[order], np.array(kinds, dtype=object)[order], np.where(pair[order] >= 0, inv[np.maximum(pair[order], 0)], -1)


@functools.lru_cache(maxsize=None)
def frame(name, n):
    """pick_model's frame with its boxes, the rectangle queries and the model's answer: computed once per session, never changed."""
    r = RectFrame()
    r.f = f = P.frame(name, n)
    r.key = f.key
    r.boxes = CM.mesh_boxes(f.pos, f.meshes)
    r.queries, r.kind, r.pair = make_queries(f)
    r.answer = pick_rect(f.tris, f.meshes, r.boxes, r.queries)
    return r


MANY = 132000  # meshes of the synthetic frame: more than the 131 072 that k_pickr_finish takes in one step


@functools.lru_cache(maxsize=None)
def many_meshes(n=MANY, cols=400, per_draw=5):
    """A hand-made frame of n one-triangle meshes on a grid of unit cells, `per_draw` consecutive meshes to a draw: the smallest shape at
    which the per-query walk over the blocks of 64 meshes takes a second step and carries the first step's count into it. Queries: the
    whole frame and a large part of it (all four entry rules), and 4 x 4 cells that straddle mesh 131 072, listed with room to spare."""
    m = np.arange(n)
    x, y = (m % cols).astype(F), (m // cols).astype(F)
    pos = np.stack([np.stack([x, y], axis=1), np.stack([x + F(0.75), y], axis=1), np.stack([x, y + F(0.75)], axis=1)], axis=1).reshape(-1, 2)
    meshes = np.zeros(n, dtype=capi.mesh_dtype)
    meshes["first_vertex"], meshes["first_index"], meshes["num_vertices"], meshes["num_indices"], meshes["draw"] = 3 * m, 3 * m, 3, 3, m // per_draw
    r = RectFrame()
    r.f = f = P.Frame()
    f.key, f.pos, f.color, f.idx, f.meshes = ("many", n), np.ascontiguousarray(pos, dtype=F), np.full(3 * n, 0xFF336699, dtype=np.uint32), np.tile(np.arange(3, dtype=np.uint16), n), meshes
    f.nm, f.nv, f.ni = n, 3 * n, 3 * n
    f.tris = P.triangles(f.pos, f.color, f.idx, f.meshes)
    r.key = f.key
    r.boxes = np.concatenate([pos.reshape(n, 3, 2).min(axis=1), pos.reshape(n, 3, 2).max(axis=1)], axis=1).astype(F)
    rows = n // cols
    q = []
    for fl in (0, WINDOW, BY_DRAW, BY_DRAW | WINDOW):
        q.append(_q(-1, -1, cols + 1, rows + 1, flags=fl))
        q.append(_q(10.5, 5.5, 200.25, 300.25, flags=fl))
        q.append(_q(-0.5, rows - 4.5, 3.9, rows + 1, flags=fl))  # rows 326 .. 329 of 330: meshes 130 400 .. 131 999
    q.append(_q(-0.5, rows - 4.5, 3.9, rows + 1, begin=131072 - 64 - 3))
    r.queries = np.array(q, dtype=capi.pick_rect_query_dtype)
    r.kind = np.array(["many"] * len(q), dtype=object)
    r.answer = pick_rect(f.tris, f.meshes, r.boxes, r.queries)
    e = r.answer.entries[2]
    assert r.answer.count[0] == n and 0 < int((e < 131072).sum()) < e.size <= 64 and 0 < r.answer.count[5] < r.answer.count[2]
    return r


def check_query_conditions(r):
    """On the model's output alone, before the product's answer is looked at."""
    k, cnt, q = r.kind, r.answer.count.astype(np.int64), r.queries
    for kind in ("outside", "inverted", "nan", "empty_range", "reserved"):
        assert int((k == kind).sum()) >= 1 and not cnt[k == kind].any(), kind
        assert np.all(r.answer.top.view(np.uint32).reshape(-1, 4)[k == kind] == NONE), kind
    assert q.shape[0] <= 192
    if r.key != BIG:
        return
    assert int((cnt > LIST_CAP).sum()) >= 10 and int(((cnt > 0) & (cnt <= LIST_CAP)).sum()) >= 10, (int((cnt > LIST_CAP).sum()), int(((cnt > 0) & (cnt <= LIST_CAP)).sum()))
    win = np.nonzero((k == "marquee") & (r.pair >= 0))[0]
    fewer = [i for i in win if 0 < cnt[i] < cnt[r.pair[i]]]
    assert len(fewer) >= 10, len(fewer)
    # BY_DRAW against by mesh: the same rectangle and the same other flags
    by_key = {(q["x0"][i], q["y0"][i], q["x1"][i], q["y1"][i], int(q["flags"][i])): i for i in np.nonzero(k == "marquee")[0]}
    grouped = [i for (x0, y0, x1, y1, fl), i in by_key.items() if fl & BY_DRAW and cnt[i] < cnt[by_key[(x0, y0, x1, y1, fl & ~BY_DRAW)]]]
    assert len(grouped) >= 10, len(grouped)
    off = np.nonzero(k == "off_square")[0]
    assert off.size == 10 and not cnt[r.pair[off]].any()
    assert int((cnt[off] > 0).sum()) >= 5, int((cnt[off] > 0).sum())
    assert cnt[k == "square"].all() and cnt[k == "on_side"].all() and cnt[k == "on_corner"].all() and cnt[k == "in_triangle"].all()
    assert int((k == "mid_run").sum()) >= 6 and cnt[k == "mid_run"].all()
    assert int((k == "point").sum()) == 40 and 5 <= int((cnt[k == "point"] > 0).sum()) <= 38


def chunks(n, size=capi.PICK_RECT_MAX_QUERIES):
    return [(a, min(a + size, n)) for a in range(0, n, size)]
