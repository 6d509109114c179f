"""vgx_pick_commands: a numpy statement of the specification in include/vgx.h. Not collected by pytest.

Coverage is not restated: a command is, to the rule, mesh c under draw c of the equivalent frame (raster_commands_model.equivalent_frame),
so the triangles, their coverage at a point (pick_frame_model.cover_many: raster_model.cover over many triangles), type, scissor and region
are read from pick_frame_model.prepare of that frame. What is stated here is what the call adds: the validity of a record, the
(cmd_end, tri_end) limit, the triangle of the answer and the way from it to the mesh that owns it. id_scene() gives the table whose
image, drawn by vgx_raster_commands, holds at every pixel the (command, triangle) a pick at the pixel's centre must report (relation
(a) of the header); frame_queries() the vgx_pick_frame queries of relation (b)."""
import numpy as np

import pick_frame_model as PF
import pick_model as PM
import raster_commands_model as CM

capi = CM.capi
F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
SKIP = capi.PICK_SKIP_TRANSPARENT
CLIP = CM.CLIP


def record_valid(sc, k):
    """The checks of the record itself: handles and what they name are not looked at, and no UV is needed."""
    c = sc.cmds[k]
    if int(c["type"]) > 3 or int(c["reserved"]) != 0 or int(c["num_vertices"]) > 65536:
        return False
    if int(c["first_vertex"]) + int(c["num_vertices"]) > sc.nv or int(c["first_index"]) + int(c["num_indices"]) > sc.ni:
        return False
    return not (int(c["clip_first_cmd"]) != NONE and int(c["clip_first_cmd"]) + int(c["clip_num_cmds"]) > sc.n)


def status(sc):
    return capi.VGX_OK if all(record_valid(sc, k) for k in range(sc.n)) else capi.VGX_E_INVALID_ARG


def owner(meshes, p):
    """The smallest m with first_index + num_indices > p, provided first_index <= p; else NONE. Word for word, no search."""
    for m in range(meshes.shape[0]):
        if int(meshes["first_index"][m]) + int(meshes["num_indices"][m]) > p:
            return m if int(meshes["first_index"][m]) <= p else NONE
    return NONE


def queries(points, cmd_end=NONE, tri_end=0, flags=0, reserved=0):
    pts = np.asarray(points, dtype=F).reshape(-1, 2)
    q = np.zeros(pts.shape[0], dtype=capi.pick_cmd_query_dtype)
    q["x"], q["y"], q["cmd_end"], q["tri_end"], q["flags"], q["reserved"] = pts[:, 0], pts[:, 1], cmd_end, tri_end, flags, reserved
    return q


def centre_queries(tgt, flags=0):
    """One query per pixel of the target, row by row, at the pixel's centre, no limit."""
    q16 = PF.centre_queries(tgt, flags)
    return queries(np.stack([q16["x"], q16["y"]], axis=1), flags=flags)


def frame_queries(q):
    """The vgx_pick_frame queries of relation (b): mesh_end = cmd_end (tri_end must be 0 for the relation to hold)."""
    out = np.zeros(q.shape[0], dtype=capi.pick_query_dtype)
    out["x"], out["y"], out["mesh_end"], out["flags"] = q["x"], q["y"], q["cmd_end"], q["flags"]
    return out


class Answer:
    """hits: capi.pick_cmd_hit_dtype per query. status: what dev_status holds. stack[q]: every hit (command, largest triangle) of the
    query's point under its flags, the limit ignored, descending. Per query: passed_in / refused_in / passed_out (a covered command under a
    tested region)."""


def prepare(sc):
    return PF.prepare(CM.equivalent_frame(sc))


def pick(sc, q, meshes=None, prep=None):
    nq = q.shape[0]
    a = Answer()
    a.hits = np.full(nq, NONE, dtype=np.uint32).repeat(4).view(capi.pick_cmd_hit_dtype)
    a.stack = [[] for _ in range(nq)]
    a.passed_in, a.refused_in, a.passed_out = (np.zeros(nq, dtype=bool) for _ in range(3))
    a.status = status(sc)
    if a.status != capi.VGX_OK or nq == 0 or sc.n == 0:
        return a
    p = prep or prepare(sc)
    Tr = p.tris
    px, py = q["x"].astype(F).astype(D), q["y"].astype(F).astype(D)
    with np.errstate(all="ignore"):
        point = (np.abs(px) < PF.LIMIT) & (np.abs(py) < PF.LIMIT) & (q["reserved"] == 0)
    X, Y = np.floor(np.where(point, px, 0)).astype(np.int64), np.floor(np.where(point, py, 0)).astype(np.int64)
    for k in range(nq):
        if not point[k]:
            continue
        flags, cend, tend = int(q["flags"][k]), int(q["cmd_end"][k]), int(q["tri_end"][k])
        s = int(PM.strip(Tr, F(q["x"][k])))
        ids = Tr.strip_tris[Tr.strip_begin[s]:Tr.strip_begin[s + 1]]
        ids = ids[(p.ylo[ids] <= py[k]) & (py[k] <= p.yhi[ids])]
        ids = ids[PF.cover_many(Tr.a[ids], Tr.b[ids], Tr.c[ids], px[k], py[k])[0]]
        cs, ts = Tr.mesh[ids], Tr.t[ids]
        r = p.rect[cs]
        ins = (X[k] >= r[:, 0]) & (X[k] < r[:, 2]) & (Y[k] >= r[:, 1]) & (Y[k] < r[:, 3])
        ids, cs, ts = ids[ins], cs[ins], ts[ins]
        below = (cs < cend) | ((cs == cend) & (ts < tend))
        counts = p.clip[cs] | ~(Tr.transparent[ids] & bool(flags & SKIP))   # limit aside: the click-through stack
        top_all, top = {}, {}
        for c, t, lim in zip(cs[counts].tolist(), ts[counts].tolist(), (below | p.clip[cs])[counts].tolist()):
            top_all[c] = max(top_all.get(c, -1), t)
            if lim:
                top[c] = max(top.get(c, -1), t)
        S, best = None, None
        for c in sorted(top_all):
            if p.clip[c]:
                S = c
                continue
            if p.tested[c]:
                member = S is not None and S >= p.f[c] and S - p.f[c] < p.n[c]
                passed = member == (p.rule[c] == 0)
                if p.rule[c] == 0:
                    a.passed_in[k] |= passed
                    a.refused_in[k] |= not passed
                else:
                    a.passed_out[k] |= passed
                if not passed:
                    continue
            a.stack[k].append((c, top_all[c]))
            if c in top:
                best = (c, top[c])
        a.stack[k].reverse()
        if best is not None:
            m = NONE if meshes is None else owner(meshes, int(sc.cmds["first_index"][best[0]]) + 3 * best[1])
            a.hits[k] = (best[0], best[1], m, NONE if m == NONE else int(meshes["draw"][m]))
    return a


# ---- the ID table of relation (a) ------------------------------------------------------------------------------------------------------
def id_scene(sc):
    """(scene, first): every triangle of the real table de-indexed to three vertices of its own (NaN positions for a triangle an index
    >= num_vertices skips), coloured 0xFF000000 | (g + 1), g = first[c] + t; every non-Clip command retyped to 0 on a white image with
    constant UV; the target clears to 0."""
    pos, color, idx, cmds = [], [], [], sc.cmds[:sc.n].copy()
    first = np.concatenate([[0], np.cumsum((cmds["num_indices"] // 3).astype(np.int64))])
    assert int(first[-1]) + 1 < (1 << 24)
    for c in range(sc.n):
        fv, fi, nv, nt = int(cmds["first_vertex"][c]), int(cmds["first_index"][c]), int(cmds["num_vertices"][c]), int(cmds["num_indices"][c]) // 3
        assert 3 * nt <= 65536
        cmds["first_vertex"][c], cmds["first_index"][c], cmds["num_vertices"][c], cmds["num_indices"][c] = len(color), len(idx), 3 * nt, 3 * nt
        if int(cmds["type"][c]) != CLIP:
            cmds["type"][c], cmds["handle"][c] = 0, 0
        for t in range(nt):
            i = [int(v) for v in sc.idx[fi + 3 * t:fi + 3 * t + 3]]
            ok = max(i) < nv
            pos += [tuple(sc.pos[fv + v]) if ok else (np.nan, np.nan) for v in i]
            color += [0xFF000000 | (int(first[c]) + t + 1)] * 3
            idx += [3 * t, 3 * t + 1, 3 * t + 2]
    t = sc.target
    tgt = type(t)(t.width, t.height, t.stride, t.x0, t.y0, None, clear=0)
    g = CM.Scene(sc.name + "_ids", np.array(pos, dtype=F).reshape(-1, 2), np.array(color, dtype=np.uint32), np.array(idx, dtype=np.uint16), cmds, tgt,
                 uv=np.full((max(len(color), 1), 2), 0.5, dtype=F)[:len(color)], images=[CM.white_image()])
    return g, first


def decode_ids(image, tgt, first):
    """([height, width] command, [height, width] triangle) as int64 of an ID image, -1 where nothing was drawn."""
    v = image[:tgt.height, :tgt.width].astype(np.int64)
    assert ((v == 0) | ((v >> 24) == 0xFF)).all()
    g = (v & 0xFFFFFF) - 1
    c = np.searchsorted(first, np.maximum(g, 0), side="right") - 1
    return np.where(v == 0, -1, c), np.where(v == 0, -1, g - first[c])
