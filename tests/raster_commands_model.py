"""numpy statement of vgx_raster_commands (include/vgx.h): a draw-command table over command-relative index streams. Not collected by
pytest. The PIXELS are not restated: the rule is vgx_raster_painted's with command c playing mesh c and draw c, so the image of a scene
is raster_painted_model.render of its equivalent frame (oracle A of the tests), which has no precondition on the ranges. What is stated
here is what the call adds: the validity of a record, the chunks, and the bin entries (pairs of a chunk of 64 triangles and a tile)."""
import math

import numpy as np

import raster_frame_model as M
import raster_model as R
import raster_painted_model as P
import raster_textured_model as T

capi = R.capi
F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
CHUNK = capi.RASTER_CHUNK
TILE = capi.RASTER_TILE
TEXTURED, GRADIENT, PATTERN, CLIP = 0, 1, 2, 3


class Scene:
    """Streams, table, images, paint tables (None: no vgx_raster_paints is handed in) and target. uv: [nv, 2] float32 / int16 or None."""

    def __init__(self, name, pos, color, idx, cmds, tgt, uv=None, images=(), gradients=None, patterns=None, real=None):
        self.name = name
        self.pos, self.color = np.ascontiguousarray(pos, dtype=F).reshape(-1, 2), np.ascontiguousarray(color, dtype=np.uint32)
        self.idx, self.cmds = np.ascontiguousarray(idx, dtype=np.uint16), np.ascontiguousarray(cmds, dtype=capi.raster_cmd_dtype)
        self.uv = None if uv is None else np.ascontiguousarray(uv)
        self.images, self.gradients, self.patterns = list(images), gradients, patterns
        self.target = tgt
        self.real = real  # the count dev_num_cmds holds, or None
        self.nv, self.ni = self.pos.shape[0], self.idx.shape[0]

    @property
    def n(self):
        return self.cmds.shape[0] if self.real is None else min(self.real, self.cmds.shape[0])

    def uv_bytes(self):
        return 0 if self.uv is None else (8 if self.uv.dtype == np.float32 else 4)

    def with_cmds(self, cmds, name=None, real=None):
        return Scene(name or self.name, self.pos, self.color, self.idx, cmds, self.target, self.uv, self.images, self.gradients, self.patterns, real)


def cmd(first_vertex, first_index, num_vertices, num_indices, typ=TEXTURED, handle=0, scissor=M.BIG, rule=0, region=None, reserved=0):
    f, n = (NONE, 0) if region is None else region
    return (first_vertex, first_index, num_vertices, num_indices, typ, handle, tuple(scissor), rule, f, n, reserved)


class Builder:
    """Commands by hand: each add() appends vertices and command-relative indices and one record over them."""

    def __init__(self):
        self.pos, self.color, self.uv, self.idx, self.cmds = [], [], [], [], []

    def add(self, verts, colors, indices, uvs=None, **kw):
        colors = [colors] * len(verts) if isinstance(colors, int) else colors
        self.cmds.append(cmd(len(self.pos), len(self.idx), len(verts), len(indices), **kw))
        self.pos += [tuple(v) for v in verts]
        self.color += list(colors)
        self.uv += [(0.5, 0.5)] * len(verts) if uvs is None else [tuple(u) for u in uvs]
        self.idx += list(indices)
        return len(self.cmds) - 1

    def scene(self, name, tgt, uv_dtype=F, images=None, **kw):
        images = [white_image()] if images is None else images
        uv = np.array(self.uv, dtype=D).reshape(-1, 2)
        uv = uv.astype(F) if uv_dtype == F else np.round(uv * 32767.0).astype(np.int16)
        return Scene(name, np.array(self.pos, dtype=F).reshape(-1, 2), np.array(self.color, dtype=np.uint32), np.array(self.idx, dtype=np.uint16),
                     np.array(self.cmds, dtype=capi.raster_cmd_dtype), tgt, uv=uv, images=images, **kw)


def white_image():
    return T.Image(np.full((2, 2), 0xFFFFFFFF, dtype=np.uint32), 2, capi.IMAGE_NEAREST)


# ---- oracle A: the equivalent frame --------------------------------------------------------------------------------------------------
def equivalent_frame(sc):
    """One mesh of kind TRILIST and one draw per command: meshes[c] = the command's ranges, draws[c].state_key = type << 16 | handle,
    draw_state[c] = scissor, rule and the command range as a draw range."""
    c = sc.cmds[:sc.n]
    meshes = np.zeros(sc.n, dtype=capi.mesh_dtype)
    for k in ("first_vertex", "first_index", "num_vertices", "num_indices"):
        meshes[k] = c[k]
    meshes["draw"] = np.arange(sc.n)
    meshes["subpath_kind"] = capi.MESH_TRILIST << 28
    f = R.make(sc.name, sc.pos, sc.color, sc.idx, meshes, sc.target)
    f.draws = np.zeros(sc.n, dtype=capi.draw_dtype)
    f.draws["state_key"] = (c["type"].astype(np.uint32) << 16) | (c["handle"] & 0xFFFF)
    f.dstate = np.zeros(sc.n, dtype=capi.draw_state_dtype)
    f.dstate["scissor"], f.dstate["clip_rule"], f.dstate["clip_first_draw"], f.dstate["clip_num_draws"] = c["scissor"], c["clip_rule"], c["clip_first_cmd"], c["clip_num_cmds"]
    f.uv = sc.uv if sc.uv is not None else np.full((sc.nv, 2), 0.5, dtype=F)
    f.images = sc.images
    f.gradients = sc.gradients if sc.gradients is not None else P.table([])
    f.patterns = sc.patterns if sc.patterns is not None else P.table([])
    return f


# ---- what the call adds --------------------------------------------------------------------------------------------------------------
def record_valid(sc, k):
    """The checks of the record itself; those of the handle and of what it names are vgx_raster_painted's, on the equivalent frame."""
    c = sc.cmds[k]
    if int(c["type"]) > 3 or int(c["reserved"]) != 0 or int(c["num_vertices"]) > 65536:
        return False
    if int(c["first_vertex"]) + int(c["num_vertices"]) > sc.nv or int(c["first_index"]) + int(c["num_indices"]) > sc.ni:
        return False
    if int(c["clip_first_cmd"]) != NONE and int(c["clip_first_cmd"]) + int(c["clip_num_cmds"]) > sc.n:
        return False
    return not (int(c["type"]) == TEXTURED and sc.uv is None)


def status(sc):
    """What dev_status holds for a target whose scissor is not empty (VGX_E_GROWN aside)."""
    if not all(record_valid(sc, k) for k in range(sc.n)):
        return capi.VGX_E_INVALID_ARG
    return P.status(equivalent_frame(sc))


def render(sc, tgt=None, image=None):
    tgt = sc.target if tgt is None else tgt
    image = tgt.background() if image is None else image
    sx0, sy0, sx1, sy1 = tgt.scissor
    if sx0 >= sx1 or sy0 >= sy1 or status(sc) != capi.VGX_OK:
        return image
    return P.render(equivalent_frame(sc), tgt, image)


def span(lo, hi, origin, c0, c1):
    """vgx_raster_span: the pixels of [c0, c1) whose sample may lie in [lo, hi], inclusive, or None."""
    base = D(origin) + 0.5
    dlo, dhi = D(lo) - base, D(hi) - base
    fa, fb = float(c0), float(c1) - 1.0
    if dlo > fa:
        fa = math.floor(dlo)
    if dhi < fb:
        fb = math.ceil(dhi)
    if not fa <= fb:
        return None
    return int(fa), int(fb)


def triangle_tiles(a, b, c, tgt, rect):
    """The inclusive tile rectangle of a triangle inside rect (image pixels, half open), or None: A == 0 or NaN, or the box misses."""
    ax, ay, bx, by, cx, cy = (D(v) for v in (*a, *b, *c))
    with np.errstate(all="ignore"):
        A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    if not (A > 0 or A < 0):
        return None
    xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
    i = span(min(xs), max(xs), tgt.x0, rect[0], rect[2])
    j = span(min(ys), max(ys), tgt.y0, rect[1], rect[3])
    if i is None or j is None:
        return None
    return i[0] // TILE, j[0] // TILE, i[1] // TILE, j[1] // TILE


def chunks(sc, tgt=None):
    """[(command, first triangle, rectangle of tiles or None)] in ascending (command, chunk) order; commands whose two scissors leave
    nothing have none."""
    tgt = sc.target if tgt is None else tgt
    out = []
    for k in range(sc.n):
        c = sc.cmds[k]
        rect = M.draw_rect(tgt, c["scissor"])
        if rect[0] >= rect[2] or rect[1] >= rect[3]:
            continue
        nt = int(c["num_indices"]) // 3
        fv, fi, nv = int(c["first_vertex"]), int(c["first_index"]), int(c["num_vertices"])
        for t0 in range(0, nt, CHUNK):
            r = None
            for t in range(t0, min(t0 + CHUNK, nt)):
                i = [int(v) for v in sc.idx[fi + 3 * t:fi + 3 * t + 3]]
                if max(i) >= nv:
                    continue
                tr = triangle_tiles(*(sc.pos[fv + v] for v in i), tgt, rect)
                if tr is not None:
                    r = tr if r is None else (min(r[0], tr[0]), min(r[1], tr[1]), max(r[2], tr[2]), max(r[3], tr[3]))
            out.append((k, t0, r))
    return out


def totals(sc, tgt=None):
    """(chunks, bin entries) of a valid scene."""
    ch = chunks(sc, tgt)
    return len(ch), sum((r[2] - r[0] + 1) * (r[3] - r[1] + 1) for _, _, r in ch if r is not None)


def tile_run(sc, tx, ty, tgt=None):
    """The chunk ordinals whose rectangle holds tile (tx, ty), ascending: the tile's run of bin entries."""
    return [n for n, (_, _, r) in enumerate(chunks(sc, tgt)) if r is not None and r[0] <= tx <= r[2] and r[1] <= ty <= r[3]]


def submit_order(draw_cmds, clip_cmds):
    """vgx_submit_order in Python: the loop of src/vg.cpp:1162-1219."""
    out = []
    prev, landed = NONE, NONE
    for c in draw_cmds:
        c = c.copy()
        f, n = int(c["clip_first_cmd"]), int(c["clip_num_cmds"])
        if f != prev:
            prev, landed = f, NONE
            if f != NONE and n > 0:
                landed = len(out)
                for j in range(n):
                    cc = clip_cmds[f + j].copy()
                    cc["type"], cc["clip_first_cmd"], cc["clip_num_cmds"] = CLIP, NONE, 0
                    out.append(cc)
        if f != NONE and n > 0:
            c["clip_first_cmd"] = landed
        out.append(c)
    return np.array(out, dtype=capi.raster_cmd_dtype) if out else np.zeros(0, dtype=capi.raster_cmd_dtype)
