"""vgx_pick_frame: a numpy statement of the specification in include/vgx.h, the frames and query sets the CPU and GPU tests share, and the
conditions those query sets must meet (tests/test_pick_frame_cpu.py: the lane code through libvgx_hosttest.so;
tests/test_gpu_pick_frame.py: the kernels).

The rule is built on the models it names: coverage of a triangle is raster_model.cover (cover_many below is the same statement over many
triangles at one point, and the CPU test holds the two together), the winding number and the box of a contour mesh are
raster_concave_model.winding / mesh_box, and draw type, scissor and region are read as raster_frame_model.render reads them. Per query the
model looks at the triangles of the point's vertical strip (pick_model.triangles: a superset of what passes the box test), then walks the
covered meshes in ascending order with the stamp. Every comparison of results is exact, in all four words.

A second check does not rest on this model: id_frame() gives the frame whose image, drawn by vgx_raster_concave, holds at every pixel the
mesh a pick at the pixel's centre must report (relation (a) of the header).
"""
import functools

import numpy as np

import cache_cull_model as CM
import pick_model as PM
import raster_concave_model as K
import raster_frame_model as M
import raster_model as R
import raster_textured_model as T

capi = R.capi
F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
CLIP = M.CLIP
SKIP = capi.PICK_SKIP_TRANSPARENT
WIDE = (0, 0, 65535, 65535)  # the largest draw scissor there is: frame pixels 0 .. 65534
LIMIT = 2147483648.0


# ---- the specification ------------------------------------------------------------------------------------------------------
def edge_many(u, v, s, px, py):
    """raster_model.edge for the directed edges u[k] -> v[k] ([n, 2] float32) of triangles of orientation s[k] at ONE sample."""
    u_lo = (u[:, 0] < v[:, 0]) | ((u[:, 0] == v[:, 0]) & (u[:, 1] <= v[:, 1]))
    lo, hi = np.where(u_lo[:, None], u, v).astype(D), np.where(u_lo[:, None], v, u).astype(D)
    g = (hi[:, 0] - lo[:, 0]) * (py - lo[:, 1]) - (hi[:, 1] - lo[:, 1]) * (px - lo[:, 0])
    f = np.where(u_lo, g, -g)
    same = (np.ascontiguousarray(u).view(np.uint32) == np.ascontiguousarray(v).view(np.uint32)).all(axis=1)
    E = s * np.where(same, 0.0, f)
    dx, dy = s * (v[:, 0].astype(D) - u[:, 0].astype(D)), s * (v[:, 1].astype(D) - u[:, 1].astype(D))
    tie = (dy > 0) | ((dy == 0) & (dx < 0))
    return E, (E > 0) | ((E == 0) & tie)


def cover_many(a, b, c, px, py):
    """(covered, zero) per triangle (a, b, c: [n, 2] float32) at the sample (px, py): raster_model.cover's rule; zero = an edge value is
    0 inside the triangle's box."""
    if a.shape[0] == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
    with np.errstate(all="ignore"):
        ad, bd, cd = a.astype(D), b.astype(D), c.astype(D)
        A = (bd[:, 0] - ad[:, 0]) * (cd[:, 1] - ad[:, 1]) - (bd[:, 1] - ad[:, 1]) * (cd[:, 0] - ad[:, 0])
        s = np.where(A > 0, 1.0, np.where(A < 0, -1.0, 0.0))
        lo, hi = np.minimum(np.minimum(a, b), c).astype(D), np.maximum(np.maximum(a, b), c).astype(D)
        box = (px >= lo[:, 0]) & (px <= hi[:, 0]) & (py >= lo[:, 1]) & (py <= hi[:, 1])
        E0, k0 = edge_many(a, b, s, px, py)
        E1, k1 = edge_many(b, c, s, px, py)
        E2, k2 = edge_many(c, a, s, px, py)
        S = (E0 + E1) + E2
        live = s != 0.0
        return live & box & k0 & k1 & k2 & (S > 0), live & box & ((E0 == 0) | (E1 == 0) | (E2 == 0))


class Prepared:
    """What the rule reads of a frame, computed once: the triangles of its triangle meshes (contour meshes emptied), the boxes, per mesh the
    draw's type, scissor and region, and the valid edges of its contour meshes."""


@functools.lru_cache(maxsize=None)
def _prepare_cached(key):
    return prepare(frame(key))


def prepare(fr):
    p = Prepared()
    meshes = fr.meshes.copy()
    p.contour = (meshes["subpath_kind"] >> 28) == capi.MESH_CONTOURS
    meshes["num_indices"][p.contour] = 0
    p.tris = PM.triangles(fr.pos, fr.color, fr.idx, meshes)
    p.first = np.concatenate([[0], np.cumsum((meshes["num_indices"] // 3).astype(np.int64))])
    with np.errstate(all="ignore"):  # the y extent of every triangle: the rule's own box test, taken first to keep a strip's work small
        p.ylo = np.minimum(np.minimum(p.tris.a[:, 1], p.tris.b[:, 1]), p.tris.c[:, 1]).astype(D)
        p.yhi = np.maximum(np.maximum(p.tris.a[:, 1], p.tris.b[:, 1]), p.tris.c[:, 1]).astype(D)
    p.boxes = CM.mesh_boxes(np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2), fr.meshes).astype(D)
    d = fr.meshes["draw"].astype(np.int64)
    p.valid = d < fr.draws.shape[0]
    dd = np.where(p.valid, d, 0)
    nd = fr.draws.shape[0]
    types = ((fr.draws["state_key"] >> 16) & 0xF).astype(np.int64) if nd else np.zeros(1, dtype=np.int64)
    ds = fr.dstate if nd else np.zeros(1, dtype=capi.draw_state_dtype)
    p.clip = types[dd] == CLIP
    sc = ds["scissor"].astype(np.int64)[dd]
    p.rect = np.stack([sc[:, 0], sc[:, 1], sc[:, 0] + sc[:, 2], sc[:, 1] + sc[:, 3]], axis=1)
    p.f, p.n, p.rule = (ds[k].astype(np.int64)[dd] for k in ("clip_first_draw", "clip_num_draws", "clip_rule"))
    p.tested = ~p.clip & (p.f != NONE) & (p.n != 0)
    p.draw = d
    p.edges = {int(m): K.mesh_edges(fr, int(m)) for m in np.nonzero(p.contour)[0]}
    return p


class Answer:
    """hits: capi.pick_hit_dtype per query. status: what dev_status holds. stack[q]: every hit mesh of the query's point under its flags,
    mesh_end ignored, descending (click-through). Per query, for the conditions: passed_in / refused_in / passed_out (a covered mesh under a
    tested draw), cut (a mesh covers the point by the rule but its draw's scissor cuts it), contour (the hit is a contour mesh), zero (an edge
    value of a candidate triangle is 0), stamper (the clip mesh whose stamp the reported hit was tested against, -1: none; see
    check_conditions for `stack_clip`)."""


def pick(fr, queries, mesh_begin=0, mesh_end=None, prep=None):
    p = prep or prepare(fr)
    nq = queries.shape[0]
    end = fr.nm if mesh_end is None else min(mesh_end, fr.nm)
    a = Answer()
    a.hits = np.full(nq, NONE, dtype=np.uint32).repeat(4).view(capi.pick_hit_dtype)
    a.stack = [[] for _ in range(nq)]
    for k in ("passed_in", "refused_in", "passed_out", "cut", "contour", "zero"):
        setattr(a, k, np.zeros(nq, dtype=bool))
    a.stamper = np.full(nq, -1, dtype=np.int64)  # the clip mesh whose stamp the reported hit was tested against
    a.status = capi.VGX_E_INVALID_ARG if mesh_begin < end and not p.valid[mesh_begin:end].all() else capi.VGX_OK
    if a.status != capi.VGX_OK or nq == 0:
        return a
    px, py = queries["x"].astype(F).astype(D), queries["y"].astype(F).astype(D)
    with np.errstate(all="ignore"):
        point = (np.abs(px) < LIMIT) & (np.abs(py) < LIMIT)
    X, Y = np.floor(np.where(point, px, 0)).astype(np.int64), np.floor(np.where(point, py, 0)).astype(np.int64)
    # contour meshes: all queries of a mesh at once
    ccov = {}
    for m, (u, v) in p.edges.items():
        if not (mesh_begin <= m < end) or int(fr.meshes["num_vertices"][m]) == 0:
            continue
        b, r = p.boxes[m], p.rect[m]
        with np.errstate(all="ignore"):
            inb = point & (px >= b[0]) & (px <= b[2]) & (py >= b[1]) & (py <= b[3])
        ins = (X >= r[0]) & (X < r[2]) & (Y >= r[1]) & (Y < r[3])
        sel = np.nonzero(inb)[0]
        if sel.size == 0:
            continue
        W = K.winding(u, v, px[sel], py[sel])
        cov = ((W & 1) != 0) if int(fr.meshes["subpath_kind"][m]) & capi.CONTOUR_EVEN_ODD else (W != 0)
        full = np.zeros(nq, dtype=bool)
        full[sel] = cov
        a.cut |= full & ~ins
        ccov[m] = full & ins
    Tr = p.tris
    alpha0 = {m: (int(fr.color[int(fr.meshes["first_vertex"][m])]) >> 24) == 0 for m in ccov}
    for q in range(nq):
        if not point[q]:
            continue
        flags, qend = int(queries["flags"][q]), int(queries["mesh_end"][q])
        ids = Tr.strip_tris[Tr.strip_begin[int(PM.strip(Tr, F(queries["x"][q])))]:Tr.strip_begin[int(PM.strip(Tr, F(queries["x"][q]))) + 1]]
        ids = ids[(p.ylo[ids] <= py[q]) & (py[q] <= p.yhi[ids])]
        ids = ids[(Tr.mesh[ids] >= mesh_begin) & (Tr.mesh[ids] < end)]
        cov, zero = cover_many(Tr.a[ids], Tr.b[ids], Tr.c[ids], px[q], py[q])
        a.zero[q] = bool(zero.any())
        ids = ids[cov]
        ms = Tr.mesh[ids]
        r, b = p.rect[ms], p.boxes[ms]
        ins = (X[q] >= r[:, 0]) & (X[q] < r[:, 2]) & (Y[q] >= r[:, 1]) & (Y[q] < r[:, 3])
        inb = (px[q] >= b[:, 0]) & (px[q] <= b[:, 2]) & (py[q] >= b[:, 1]) & (py[q] <= b[:, 3])
        a.cut[q] |= bool((~ins).any())
        ids, ms = ids[ins & inb], ms[ins & inb]
        # under the flag a triangle with an alpha-0 corner is skipped -- but not for a clip mesh: stamping is not the query's
        if flags & SKIP:
            keep = ~Tr.transparent[ids] | p.clip[ms]
            ids, ms = ids[keep], ms[keep]
        top = {}
        for g, m in zip(ids.tolist(), ms.tolist()):
            top[m] = int(Tr.t[g])  # ascending: the last one stays
        for m, full in ccov.items():
            if full[q] and not ((flags & SKIP) and alpha0[m] and not p.clip[m]):
                top[m] = NONE
        S, best = None, None
        for m in sorted(top):
            if p.clip[m]:
                S = (int(p.draw[m]), m)
                continue
            if p.tested[m]:
                member = S is not None and S[0] >= p.f[m] and S[0] - p.f[m] < p.n[m]
                passed = member == (p.rule[m] == 0)
                if p.rule[m] == 0:
                    a.passed_in[q] |= passed
                    a.refused_in[q] |= not passed
                else:
                    a.passed_out[q] |= passed
                if not passed:
                    continue
            a.stack[q].append(m)
            if m < qend:
                best = (m, top[m], S[1] if (S is not None and p.tested[m]) else -1)
        a.stack[q].reverse()
        if best is not None:
            m = best[0]
            a.hits[q] = (m, best[1], int(fr.meshes["draw"][m]), int(fr.meshes["subpath_kind"][m]))
            a.contour[q] = bool(p.contour[m])
            a.stamper[q] = best[2]
    return a


# ---- the ID frame of relation (a) ----------------------------------------------------------------------------------------------
def id_frame(fr, skip_transparent=False):
    """(frame, target): the same streams with every vertex colour of mesh m set to 0xFF000000 | (m + 1), every non-Clip draw retyped to 0,
    the kinds TEXT and TRILIST rewritten to FILL, for vgx_raster_concave over a clear of 0 under a target scissor that cuts nothing.
    skip_transparent: the frame VGX_PICK_SKIP_TRANSPARENT sees -- under a non-Clip draw the first index of every triangle with an alpha-0
    corner becomes 0xFFFF (the raster skips it) and a contour mesh of an alpha-0 colour loses its indices."""
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    color, idx, meshes = fr.color.copy(), fr.idx.copy(), fr.meshes.copy()
    draws = fr.draws.copy()
    nd = draws.shape[0]
    types = (draws["state_key"] >> 16) & 0xF
    draws["state_key"] = np.where(types == CLIP, draws["state_key"], draws["state_key"] & np.uint32(0xFFF00000))  # type 0, handle 0
    for m in range(fr.nm):
        me = fr.meshes[m]
        fv, nv, fi, ni = int(me["first_vertex"]), int(me["num_vertices"]), int(me["first_index"]), int(me["num_indices"])
        assert nv < 65535 and (m + 1 == fr.nm or fv + nv <= int(fr.meshes["first_vertex"][m + 1]))
        kind = int(me["subpath_kind"]) >> 28
        clip = int(me["draw"]) < nd and int(types[int(me["draw"])]) == CLIP
        if skip_transparent and not clip and nv:
            if kind == capi.MESH_CONTOURS:
                if (int(fr.color[fv]) >> 24) == 0:
                    meshes["num_indices"][m] = 0
            else:
                tri = fr.idx[fi:fi + ni // 3 * 3].astype(np.int64).reshape(-1, 3)
                ok = (tri < nv).all(axis=1)
                a0 = ((fr.color[fv + np.where(ok[:, None], tri, 0)] >> 24) == 0).any(axis=1) & ok
                idx[fi + 3 * np.nonzero(a0)[0]] = 0xFFFF
        color[fv:fv + nv] = 0xFF000000 | (m + 1)
        if kind in (R.TEXT, R.TRILIST):
            meshes["subpath_kind"][m] = (int(me["subpath_kind"]) & 0x0FFFFFFF) | (capi.MESH_FILL << 28)
    g = R.make(fr.name, pos, color, idx, meshes, None)
    g.draws, g.dstate = draws, fr.dstate
    g.uv, g.images = np.full((max(g.nv, 1), 2), np.nan, dtype=F), []
    g.gradients, g.patterns = np.zeros(0, dtype=capi.paint_dtype), np.zeros(0, dtype=capi.paint_dtype)
    t = fr.target
    return g, R.Target(t.width, t.height, t.stride, t.x0, t.y0, None, clear=0)


def decode_ids(image, tgt):
    """[height, width] int64: the mesh of every pixel of an ID image, -1 where nothing was drawn."""
    v = image[:tgt.height, :tgt.width].astype(np.int64)
    assert ((v == 0) | ((v >> 24) == 0xFF)).all()
    return np.where(v == 0, -1, (v & 0xFFFFFF) - 1)


def centre_queries(tgt, flags=0):
    """One query per pixel of the target, row by row, at the pixel's centre, mesh_end = all."""
    j, i = np.mgrid[0:tgt.height, 0:tgt.width]
    q = np.zeros(i.size, dtype=capi.pick_query_dtype)
    q["x"], q["y"] = (i.reshape(-1) + tgt.x0).astype(D) + 0.5, (j.reshape(-1) + tgt.y0).astype(D) + 0.5
    q["mesh_end"], q["flags"] = NONE, flags
    return q


# ---- frames ------------------------------------------------------------------------------------------------------------------
CONCAVE = ("state", "crowd", "centres", "aa_seam", "odd", "star300")
FRAMED = ("clips", "lattice_clip", "stack_clip")
IMAGES = tuple(("concave", n) for n in CONCAVE) + tuple(("frame", n) for n in FRAMED) + (("textured", "state"),)   # frames with a target
STREAMS = (("pick", "walk", 1), ("pick", "tiger", 257), ("pick", "empty", 65))                                       # the reference's frames, all PLAIN
ALL = IMAGES + STREAMS
TIGER = ("pick", "tiger", 257)


def plain_state(fr, scissor=WIDE):
    """A draw table for a bare mesh stream: every draw of type 0, no region, one scissor."""
    nd = int(fr.meshes["draw"].max()) + 1 if fr.nm else 0
    fr.draws = np.zeros(nd, dtype=capi.draw_dtype)
    fr.dstate = np.array([M.state(scissor=scissor)] * nd, dtype=capi.draw_state_dtype) if nd else np.zeros(0, dtype=capi.draw_state_dtype)
    return fr


@functools.lru_cache(maxsize=None)
def frame(key):
    """The shared frames by key, never changed: ("concave" | "frame" | "textured", name) are the raster models' own, with their targets;
    ("pick", name, n) is pick_model's frame under an all-PLAIN draw table, without a target."""
    if key[0] == "concave":
        return K.frame(key[1])
    if key[0] == "frame":
        return M.frame(key[1])
    if key[0] == "textured":
        return T.frame(key[1])
    f = PM.frame(key[1], key[2])
    g = R.make("%s%d" % key[1:], f.pos, f.color, f.idx, f.meshes, None)
    g.pick = f
    return plain_state(g)


def frame_box(fr):
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    fin = pos[np.isfinite(pos).all(axis=1)]
    if fin.shape[0] == 0:
        return 0.0, 0.0, 1.0, 1.0
    return float(fin[:, 0].min()), float(fin[:, 1].min()), float(fin[:, 0].max()), float(fin[:, 1].max())


def off_centre_points(fr, seed, nvert=120, nmid=120, nrand=240):
    """Mesh vertices, midpoints of triangle and contour edges, seeded random points in the frame's box; then NaN, +-inf, +-2^31."""
    rs = np.random.RandomState(seed)
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    pts = []
    used = np.zeros(max(fr.nv, 1), dtype=bool)
    mids = []
    for m in range(fr.nm):
        me = fr.meshes[m]
        fv, nv, fi, ni = int(me["first_vertex"]), int(me["num_vertices"]), int(me["first_index"]), int(me["num_indices"])
        per = 2 if (int(me["subpath_kind"]) >> 28) == capi.MESH_CONTOURS else 3
        e = fr.idx[fi:fi + ni // per * per].astype(np.int64).reshape(-1, per)
        e = e[(e < nv).all(axis=1)]
        used[fv + e.reshape(-1)] = True
        if e.shape[0]:
            pick_e = e[rs.randint(0, e.shape[0], size=min(4, e.shape[0]))]
            mids += [(fv + int(r[0]), fv + int(r[1])) for r in pick_e]
    vs = np.nonzero(used)[0]
    if vs.size:
        for v in rs.choice(vs, size=min(nvert, vs.size), replace=False):
            pts.append((pos[v, 0], pos[v, 1]))
        for k in rs.permutation(len(mids))[:nmid]:
            u, v = pos[mids[k][0]].astype(D), pos[mids[k][1]].astype(D)
            pts.append((F((u[0] + v[0]) / 2), F((u[1] + v[1]) / 2)))
    x0, y0, x1, y1 = frame_box(fr)
    for _ in range(nrand):
        pts.append((F(rs.uniform(x0 - 2, x1 + 2)), F(rs.uniform(y0 - 2, y1 + 2))))
    c = pts[0] if pts else (F(0), F(0))
    pts += [(np.nan, c[1]), (c[0], np.nan), (np.inf, c[1]), (c[0], -np.inf), (F(2147483648.0), c[1]), (c[0], F(-2147483648.0)), (F(2147483520.0), F(-2147483520.0))]
    return np.array(pts, dtype=F)


class QuerySet:
    """queries: capi.pick_query_dtype; centres: how many of them, in front, are the target's pixel centres (flags 0, mesh_end all)."""


@functools.lru_cache(maxsize=None)
def query_set(key):
    """The shared query set of a frame: every pixel centre of its target (when it has one), then the off-centre points four times over --
    flags 0 and VGX_PICK_SKIP_TRANSPARENT, each with mesh_end = all and with a per-query mesh_end drawn from below, inside and above the
    range (0, a mesh of the frame, the end, beyond)."""
    fr = frame(key)
    qs = QuerySet()
    parts = []
    qs.centres = 0
    if fr.target is not None:
        parts.append(centre_queries(fr.target))
        qs.centres = parts[0].shape[0]
    if key[0] == "pick":
        parts.append(fr.pick.queries.copy())
    pts = off_centre_points(fr, seed=5 + len(key[1]))
    rs = np.random.RandomState(17)
    for flags in (0, SKIP):
        for limited in (False, True):
            q = np.zeros(pts.shape[0], dtype=capi.pick_query_dtype)
            q["x"], q["y"], q["flags"], q["mesh_end"] = pts[:, 0], pts[:, 1], flags, NONE
            if limited:
                ends = np.concatenate([[0, fr.nm, fr.nm + 7, max(fr.nm - 1, 0)], rs.randint(0, fr.nm + 1, size=pts.shape[0])])
                q["mesh_end"] = ends[rs.permutation(ends.shape[0])[:pts.shape[0]]]
            parts.append(q)
    qs.queries = np.concatenate(parts)
    return qs


@functools.lru_cache(maxsize=None)
def expected(key):
    """The model's answer to the frame's query set over the whole range: computed once per session, never changed."""
    return pick(frame(key), query_set(key).queries, prep=_prepare_cached(key))


def chunks(n, size=capi.PICK_MAX_QUERIES):
    return PM.chunks(n, size)


# ---- what the query sets must exercise ----------------------------------------------------------------------------------------
def pick_rule_hits(fr, prep, queries):
    """Per query: does vgx_pick's rule (closed triangles, no state) hit anything?"""
    Tr = prep.tris
    return np.array([PM.containing(Tr, queries["x"][q], queries["y"][q]).size > 0 for q in range(queries.shape[0])])


def check_conditions(key):
    """On the model's output alone, before the product's answer is looked at."""
    fr, qs, a = frame(key), query_set(key), expected(key)
    hit = a.hits["mesh"] != NONE
    bad = ~(np.abs(qs.queries["x"].astype(D)) < LIMIT) | ~(np.abs(qs.queries["y"].astype(D)) < LIMIT)
    assert int(bad.sum()) >= 24 and not hit[bad].any()   # NaN, +-inf and +-2^31 are in every set, and none of them hits
    if fr.nm and key != ("pick", "empty", 65):
        assert hit.any() and (~hit & ~bad).any()
    has_clip = fr.draws.shape[0] and (((fr.draws["state_key"] >> 16) & 0xF) == CLIP).any()
    if key in (("concave", "state"), ("frame", "clips"), ("textured", "state")):
        assert a.passed_in.any() and a.refused_in.any() and a.passed_out.any()
        prep = _prepare_cached(key)
        cut = np.nonzero(a.cut)[0]
        assert cut.size and pick_rule_hits(fr, prep, qs.queries[cut[:400]]).any()   # cut by a draw scissor where vgx_pick's rule hits
    if key in (("frame", "lattice_clip"), ("frame", "stack_clip")):
        assert has_clip and a.passed_in.any()
    if key[0] == "concave":
        assert a.contour.any()
        assert (a.hits["triangle"][a.contour] == NONE).all()
    if key in (("frame", "lattice_clip"), ("concave", "aa_seam")):
        assert a.zero[:qs.centres].any()   # a pixel centre on a shared edge of two triangles: the tie rule decides
    if key == ("concave", "centres"):       # ... and on the edges of a contour mesh (every vertex of the frame is a pixel centre)
        on_vertex = [q for q in range(qs.centres) if (fr.pos == (qs.queries["x"][q], qs.queries["y"][q])).all(axis=1).any()]
        assert len(on_vertex) >= 6 and hit[on_vertex].any() and not hit[on_vertex].all()
    if key == ("frame", "stack_clip"):
        # a covering clip mesh and a hit tested against it with at least 256 meshes of the same tile between them: whatever subset of those
        # the call makes candidates, all of them cover the tile, so the two lie in different chunks of 256 candidates
        far = (a.stamper >= 0) & (a.hits["mesh"].astype(np.int64) - a.stamper > 256) & hit
        assert far.any()
