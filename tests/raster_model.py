"""vgx_raster: a numpy statement of the specification in include/vgx.h, the frames the CPU and GPU tests share, and the conditions
those frames must meet (tests/test_raster_cpu.py: the lane code through libvgx_hosttest.so; tests/test_gpu_raster.py: the kernels).

The model goes triangle by triangle in ascending (mesh, triangle) order and, per triangle, over the pixels of its box at once: float64
arrays for the edge values, integers for the blend. It knows nothing of mesh boxes, tiles or bins. numpy never fuses a multiply and
an add. Every comparison of images is exact.

The `tiger` frame. pick_model.frame("tiger", 1) is ONE instance of a ONE-mesh range of the cache (128 vertices, 23 x 39 pixels): no
200 x 160 window is cut by it on four sides and nothing in it is blended three times. It is rendered all the same (frame "tiger1"),
and the frame the conditions are asserted on is one instance of the WHOLE drawing of the same cache, scaled so that the window lies
inside it.
"""
import functools

import numpy as np

import cache_cull_model as CM
import pick_model as PM

capi = CM.capi
oracle = CM.oracle
F = np.float32
D = np.float64
PATTERN = 0x5A5A5A5A
TEXT, TRILIST = 7, 6


class Target:
    """vgx_raster_target without the pointer."""

    def __init__(self, width, height, stride, x0, y0, scissor=None, clear=None):
        self.width, self.height, self.stride, self.x0, self.y0 = width, height, stride, x0, y0
        self.scissor = (0, 0, width, height) if scissor is None else tuple(scissor)
        self.clear = clear  # None: no VGX_RASTER_CLEAR

    def with_clear(self, color):
        return Target(self.width, self.height, self.stride, self.x0, self.y0, self.scissor, color)

    def rows(self):
        return max(self.height, 1)

    def background(self):
        """[rows, stride] uint32: guard values in the stride padding, a picture that is not flat inside (so that blending over it shows)."""
        j, i = np.mgrid[0:self.rows(), 0:self.stride]
        img = ((i * 7 + j * 13) & 255) | (((i * 3 + j * 5) & 255) << 8) | (((i + j * 11) & 255) << 16) | (((i * 5 + j) & 255) << 24)
        img = img.astype(np.uint32)
        img[:, self.width:] = PATTERN
        return img

    def struct(self, ptr):
        return capi.RasterTarget(ptr, self.width, self.height, self.stride, self.x0, self.y0, (capi.C.c_uint32 * 4)(*self.scissor),
                                 capi.RASTER_CLEAR if self.clear is not None else 0, self.clear or 0)


# ---- the specification -----------------------------------------------------------------------------------------------
def edge(u, v, s, px, py):
    """(E, accept) of the directed edge u -> v (float32 pairs) of a triangle of orientation s at the samples px, py (float64 arrays)."""
    u_lo = bool(u[0] < v[0] or (u[0] == v[0] and u[1] <= v[1]))
    lo, hi = (u, v) if u_lo else (v, u)
    g = (D(hi[0]) - D(lo[0])) * (py - D(lo[1])) - (D(hi[1]) - D(lo[1])) * (px - D(lo[0]))
    f = g if u_lo else -g
    if u.tobytes() == v.tobytes():
        f = np.zeros_like(g)
    E = s * f
    dx, dy = s * (D(v[0]) - D(u[0])), s * (D(v[1]) - D(u[1]))
    tie = bool(dy > 0 or (dy == 0 and dx < 0))
    return E, (E > 0) | ((E == 0) & tie)


def orientation(a, b, c):
    """s = +1 / -1, or 0 when the triangle covers nothing (A == 0 or NaN)."""
    ax, ay, bx, by, cx, cy = (D(v) for v in (a[0], a[1], b[0], b[1], c[0], c[1]))
    with np.errstate(all="ignore"):
        A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    return 1.0 if A > 0 else (-1.0 if A < 0 else 0.0)


def cover(a, b, c, px, py):
    """(covered, E0, E1, E2, S, any_zero) at the samples; a, b, c float32 pairs; None when the triangle covers nothing."""
    s = orientation(a, b, c)
    if s == 0.0:
        return None
    with np.errstate(all="ignore"):
        box = ((px >= D(min(a[0], b[0], c[0]))) & (px <= D(max(a[0], b[0], c[0]))) & (py >= D(min(a[1], b[1], c[1]))) & (py <= D(max(a[1], b[1], c[1]))))
        E0, k0 = edge(a, b, s, px, py)
        E1, k1 = edge(b, c, s, px, py)
        E2, k2 = edge(c, a, s, px, py)
        S = (E0 + E1) + E2
    return box & k0 & k1 & k2 & (S > 0), E0, E1, E2, S, box & ((E0 == 0) | (E1 == 0) | (E2 == 0))


def div255(x):
    return (x + 127) // 255


def blend(dst, src, a):
    """dst uint32 array, src: four int64 arrays (r, g, b, a as the rule's q), a = src[3]."""
    out = np.zeros(dst.shape, dtype=np.int64)
    ia = 255 - a
    for ch in range(4):
        d = ((dst >> np.uint32(8 * ch)) & np.uint32(255)).astype(np.int64)
        s = src[ch] if ch < 3 else np.full(a.shape, 255, dtype=np.int64)
        out |= div255(s * a + d * ia) << (8 * ch)
    return out.astype(np.uint32)


class Stats:
    """What check_conditions looks at: per pixel how often it was blended (in all, and per mesh when asked), samples with an Ek == 0
    inside a triangle's box, pixels blended with 0 < a < 255 by a triangle whose vertex alphas differ."""

    def __init__(self, tgt, per_mesh=False):
        self.blends = np.zeros((tgt.rows(), tgt.stride), dtype=np.int32)
        self.per_mesh = {} if per_mesh else None
        self.edge_zero = 0
        self.fringe = np.zeros((tgt.rows(), tgt.stride), dtype=bool)


def render(fr, tgt, image, mesh_begin=0, mesh_end=None, order=None, stats=None, skip_mesh=None):
    """Draws into `image` ([rows, stride] uint32, changed in place) and returns it. order: the meshes of the range in another order
    (the conditions only); skip_mesh: a mesh to leave out (the conditions only)."""
    sx0, sy0, sx1, sy1 = tgt.scissor
    if tgt.clear is not None:
        image[sy0:sy1, sx0:sx1] = np.uint32(tgt.clear)
    if sx0 >= sx1 or sy0 >= sy1:
        return image
    nm = fr.meshes.shape[0]
    end = nm if mesh_end is None else min(mesh_end, nm)
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    for m in (range(mesh_begin, end) if order is None else order):
        me = fr.meshes[m]
        if (int(me["subpath_kind"]) >> 28) in (TEXT, TRILIST) or m == skip_mesh:
            continue
        nt, nv, fv, fi = int(me["num_indices"]) // 3, int(me["num_vertices"]), int(me["first_vertex"]), int(me["first_index"])
        if nt == 0:
            continue
        ids = fr.idx[fi:fi + 3 * nt].astype(np.int64).reshape(-1, 3)
        valid = (ids < nv).all(axis=1)
        safe = np.where(valid[:, None], ids, 0) + (fv if nv else 0)
        P = pos[safe] if pos.shape[0] else np.zeros((nt, 3, 2), dtype=F)
        C = fr.color[safe] if pos.shape[0] else np.zeros((nt, 3), dtype=np.uint32)
        # a generous pixel range per triangle (two pixels more than the box on every side), clipped to the scissor: the rule's own box
        # test decides. NaN boxes get nothing, as the rule says
        with np.errstate(all="ignore"):
            lo, hi = P.min(axis=1).astype(D), P.max(axis=1).astype(D)
            ok = valid & ~np.isnan(lo).any(axis=1) & ~np.isnan(hi).any(axis=1)
            i0 = np.clip(np.floor(np.where(ok, lo[:, 0], 0) - tgt.x0) - 2, sx0, sx1).astype(np.int64)
            i1 = np.clip(np.ceil(np.where(ok, hi[:, 0], 0) - tgt.x0) + 2, sx0, sx1).astype(np.int64)
            j0 = np.clip(np.floor(np.where(ok, lo[:, 1], 0) - tgt.y0) - 2, sy0, sy1).astype(np.int64)
            j1 = np.clip(np.ceil(np.where(ok, hi[:, 1], 0) - tgt.y0) + 2, sy0, sy1).astype(np.int64)
        for t in np.nonzero(ok & (i0 < i1) & (j0 < j1))[0]:
            a, b, c = P[t, 0], P[t, 1], P[t, 2]
            py, px = np.mgrid[j0[t]:j1[t], i0[t]:i1[t]]
            px, py = (px + tgt.x0).astype(D) + 0.5, (py + tgt.y0).astype(D) + 0.5
            got = cover(a, b, c, px, py)
            if got is None:
                continue
            cov, E0, E1, E2, S, zero = got
            if stats is not None:
                stats.edge_zero += int(zero.sum())
            if not cov.any():
                continue
            with np.errstate(all="ignore"):
                q = []
                for ch in range(4):
                    ca, cb, cc = (D((int(C[t, k]) >> (8 * ch)) & 255) for k in range(3))
                    v = ((E1 * ca + E2 * cb) + E0 * cc) / S
                    q.append(np.minimum(np.where(cov, v + 0.5, 0).astype(np.int64), 255))
            view = image[j0[t]:j1[t], i0[t]:i1[t]]
            hit = cov & (q[3] != 0)
            view[hit] = blend(view, q, q[3])[hit]
            if stats is not None:
                stats.blends[j0[t]:j1[t], i0[t]:i1[t]] += hit
                if stats.per_mesh is not None:
                    stats.per_mesh.setdefault(m, np.zeros(stats.blends.shape, dtype=np.int32))[j0[t]:j1[t], i0[t]:i1[t]] += hit
                alphas = [int(C[t, k]) >> 24 for k in range(3)]
                if min(alphas) != max(alphas):
                    stats.fringe[j0[t]:j1[t], i0[t]:i1[t]] |= hit & (q[3] > 0) & (q[3] < 255)
    return image


def bin_entries(fr, tgt, mesh_begin=0, mesh_end=None):
    """Pairs of a drawn mesh of the range and a 16 x 16 tile its box reaches inside the scissor (what vgx_raster_reserve is told):
    computed here with a pixel more on every side, so an upper bound of what the call counts."""
    sx0, sy0, sx1, sy1 = tgt.scissor
    boxes = CM.mesh_boxes(fr.pos, fr.meshes)
    n = 0
    for m in range(mesh_begin, fr.meshes.shape[0] if mesh_end is None else min(mesh_end, fr.meshes.shape[0])):
        if (int(fr.meshes["subpath_kind"][m]) >> 28) in (TEXT, TRILIST) or int(fr.meshes["num_indices"][m]) < 3:
            continue
        b = boxes[m].astype(D)
        i0, i1 = max(np.floor(b[0] - tgt.x0) - 1, sx0), min(np.ceil(b[2] - tgt.x0) + 1, sx1 - 1)
        j0, j1 = max(np.floor(b[1] - tgt.y0) - 1, sy0), min(np.ceil(b[3] - tgt.y0) + 1, sy1 - 1)
        if i0 <= i1 and j0 <= j1:
            n += (int(i1) // 16 - int(i0) // 16 + 1) * (int(j1) // 16 - int(j0) // 16 + 1)
    return n


# ---- frames ---------------------------------------------------------------------------------------------------------
class Frame:
    def desc(self, ptrs=None):
        p = ptrs or [a.ctypes.data for a in (self.pos, self.color, self.idx, self.meshes)]
        return capi.CacheDesc(p[0], p[1], p[2], p[3], self.nm, self.nv, self.ni)


def make(name, pos, color, idx, meshes, tgt):
    f = Frame()
    f.name = name
    f.pos, f.color = np.ascontiguousarray(pos, dtype=F).reshape(-1, 2), np.ascontiguousarray(color, dtype=np.uint32)
    f.idx, f.meshes = np.ascontiguousarray(idx, dtype=np.uint16), np.ascontiguousarray(meshes, dtype=capi.mesh_dtype)
    f.nm, f.nv, f.ni = f.meshes.shape[0], f.pos.shape[0], f.idx.shape[0]
    f.target = tgt
    return f


class Builder:
    """Mesh streams by hand."""

    def __init__(self):
        self.pos, self.color, self.idx, self.meshes = [], [], [], []

    def mesh(self, verts, colors, indices, kind=0, num_vertices=None):
        colors = [colors] * len(verts) if isinstance(colors, int) else colors
        self.meshes.append((len(self.pos), len(self.idx), len(verts) if num_vertices is None else num_vertices, len(indices), len(self.meshes), kind << 28))
        self.pos += [tuple(v) for v in verts]
        self.color += list(colors)
        self.idx += list(indices)
        return len(self.meshes) - 1

    def frame(self, name, tgt):
        return make(name, np.array(self.pos, dtype=F), np.array(self.color, dtype=np.uint32), np.array(self.idx, dtype=np.uint16),
                    np.array(self.meshes, dtype=capi.mesh_dtype), tgt)


def lattice():
    """Shared edges and vertices exactly through pixel centres: every coordinate is a half-integer, like every sample."""
    b = Builder()
    f_out = {}
    # 0: a convex fan around a centre that is a pixel centre, every spoke through pixel centres; per-vertex colours, alpha 128
    ring = [(20.5, 4.5), (30.5, 8.5), (36.5, 18.5), (32.5, 30.5), (20.5, 36.5), (8.5, 30.5), (4.5, 18.5), (10.5, 8.5)]
    cols = [0x80000000 | ((37 * k) & 255) | (((91 * k + 40) & 255) << 8) | (((53 * k + 90) & 255) << 16) for k in range(9)]
    fan = [i for k in range(8) for i in (0, 1 + k, 1 + (k + 1) % 8)]
    m = b.mesh([(20.5, 18.5)] + ring, cols, fan)
    f_out[m] = ring
    # 1: 4 x 4 quads of 6 x 6 pixels, corners on pixel centres, diagonals through pixel centres; the two triangles of a quad and the quads
    # among each other wound both ways, one diagonal or the other
    verts = [(40.5 + 6 * i, 6.5 + 6 * j) for j in range(5) for i in range(5)]
    ind = []
    for j in range(4):
        for i in range(4):
            v00, v10, v01, v11 = 5 * j + i, 5 * j + i + 1, 5 * j + 5 + i, 5 * j + 6 + i
            if (i + j) % 2:
                tris = [(v00, v10, v11), (v00, v01, v11)] if i % 2 else [(v00, v10, v11), (v00, v11, v01)]
            else:
                tris = [(v10, v01, v00), (v10, v11, v01)] if j % 2 else [(v10, v00, v01), (v10, v11, v01)]
            ind += [k for t in tris for k in t]
    m = b.mesh(verts, 0x8040C0FF, ind)
    f_out[m] = [(40.5, 6.5), (64.5, 6.5), (64.5, 30.5), (40.5, 30.5)]
    # 2: the same square as a quad of kind TEXT over the fan: it must leave no trace
    f_text = b.mesh([(6.5, 6.5), (34.5, 6.5), (34.5, 34.5), (6.5, 34.5)], 0xFF00FF00, [0, 1, 2, 0, 2, 3], kind=TEXT)
    # 3: a sound quad (over the lattice of 1, translucent) and, in the same mesh, what the rule skips: a zero-area triangle, a triangle
    # with an index >= num_vertices (vertex 6 exists in the stream, the mesh claims 6 vertices), a NaN vertex, and an index remainder
    verts = [(46.5, 12.5), (60.5, 14.5), (58.5, 27.5), (44.5, 24.5), (50.5, 2.5), (np.nan, 20.5), (70.5, 33.5)]
    ind = [0, 1, 2, 0, 2, 3,  0, 4, 4,  0, 1, 6,  0, 5, 2,  4, 1]
    m = b.mesh(verts, 0x802020E0, ind, kind=1, num_vertices=6)
    f_out[m] = [verts[k] for k in range(4)]
    # 4: a fan around an inner vertex and a triangle beside it, wound both ways, with edges through pixel centres at slopes of 1 / 2,
    # 1 / 4 and 1; every vertex its own colour
    verts = [(6.5, 40.5), (30.5, 40.5), (38.5, 44.5), (30.5, 52.5), (6.5, 52.5), (14.5, 44.5)]
    m = b.mesh(verts, [0x80FF0000, 0x8000FF00, 0x800000FF, 0x80FFFF00, 0x80FF00FF, 0x8000FFFF], [0, 1, 5, 5, 0, 4,  1, 2, 3, 5, 3, 1, 5, 3, 4])
    f_out[m] = [verts[k] for k in (0, 1, 2, 3, 4)]
    f = b.frame("lattice", Target(77, 59, 80, 0, 0))
    f.outline, f.text_mesh = f_out, f_text
    return f


def stack():
    """300 small translucent meshes (a triangle or a quad each) over one 16 x 16 tile: more than 256 meshes and more than 256
    triangles on one tile."""
    rs = np.random.RandomState(8)
    b = Builder()
    for k in range(300):
        c = rs.uniform(6, 10, 2) + 16
        r = rs.uniform(1.5, 5.9)
        n = 3 + k % 2
        ang = rs.uniform(0, 6.28) + np.arange(n) * 6.28318 / n
        verts = [(c[0] + r * np.cos(t), c[1] + r * np.sin(t)) for t in ang]
        col = [int(rs.randint(40, 200)) << 24 | int(rs.randint(0, 1 << 24)) for _ in range(n)]
        b.mesh(verts, col if k % 3 else col[0], [0, 1, 2] if n == 3 else [0, 1, 2, 0, 2, 3], kind=k % 2)
    return b.frame("stack", Target(48, 48, 48, 0, 0))


def long_stroke():
    """One Round-join AA stroke of the reference: a mesh of more than 600 triangles that crosses many tiles."""
    ps, d = CM.wl.random_walk_polylines(n=1, nseg=100)
    d = d.copy()
    d["stroke_color"] = 0x802060FF
    r = oracle.tessellate(ps, d)
    lo, hi = np.floor(r.pos.min(axis=0)).astype(int), np.ceil(r.pos.max(axis=0)).astype(int)
    w, h = int(hi[0] - lo[0]) + 6, int(hi[1] - lo[1]) + 6
    return make("long", r.pos, r.color, r.idx, r.meshes, Target(w, h, w + 5, int(lo[0]) - 3, int(lo[1]) - 3))


TIGER_MTX = [0.4, 0.0, 0.0, 0.4, -150.0, -120.0]


def tiger():
    """The whole Tiger of cache_cull_model's cache as ONE instance (see the module text), 0.4 x: about 355 x 307 pixels from (-150, -96).
    The 200 x 160 window starts at (-40, -30), inside the drawing, and its scissor lies strictly inside the image."""
    c = CM.case("tiger")
    inst = np.zeros(1, dtype=capi.cache_instance_dtype)
    inst["num_meshes"], inst["color"] = c.nm, 0xC0336699
    inst["mtx"][0] = TIGER_MTX
    fr = oracle.cache_submit(c.cache, inst)
    return make("tiger", fr.pos, fr.color, fr.idx, fr.meshes, Target(200, 160, 208, -40, -30, scissor=(3, 5, 191, 149)))


def tiger1():
    f = PM.frame("tiger", 1)
    lo = np.floor(f.pos.min(axis=0)).astype(int)
    return make("tiger1", f.pos, f.color, f.idx, f.meshes, Target(21, 45, 24, int(lo[0]) - 2, int(lo[1]) + 3, scissor=(1, 0, 21, 44)))


NAMES = ("lattice", "stack", "long", "tiger", "tiger1")
_MAKERS = {"lattice": lattice, "stack": stack, "long": long_stroke, "tiger": tiger, "tiger1": tiger1}


@functools.lru_cache(maxsize=None)
def frame(name):
    return _MAKERS[name]()


@functools.lru_cache(maxsize=None)
def _expected(name, clear):
    f = frame(name)
    tgt = f.target.with_clear(0xFF102030) if clear else f.target
    img = render(f, tgt, tgt.background())
    img.setflags(write=False)
    return img


def expected(name, clear=False):
    """The model's image of a frame over its target's background: computed once per session, never changed."""
    return _expected(name, bool(clear))


def guards_intact(tgt, image):
    """The stride padding, and everything outside the scissor, is what the background had there."""
    bg = tgt.background()
    out = np.ones(bg.shape, dtype=bool)
    sx0, sy0, sx1, sy1 = tgt.scissor
    out[sy0:sy1, sx0:sx1] = False
    return bool(np.array_equal(image[out], bg[out]))


# ---- conditions: each frame does what it is for --------------------------------------------------------------------------
def inside_polygon(poly, x, y):
    """Strictly inside a convex polygon given either way round; exact: every coordinate is a half-integer."""
    sign = None
    res = np.ones(x.shape, dtype=bool)
    for k in range(len(poly)):
        (ux, uy), (vx, vy) = poly[k], poly[(k + 1) % len(poly)]
        e = (vx - ux) * (y - uy) - (vy - uy) * (x - ux)
        if sign is None:
            cx, cy = np.mean([p[0] for p in poly]), np.mean([p[1] for p in poly])
            sign = 1.0 if (vx - ux) * (cy - uy) - (vy - uy) * (cx - ux) > 0 else -1.0
        res &= (sign * e) > 0
    return res


@functools.lru_cache(maxsize=None)
def check_conditions(name):
    """On the model alone, before anything of the product is looked at."""
    f = frame(name)
    tgt = f.target
    if name == "lattice":
        st = Stats(tgt, per_mesh=True)
        img = render(f, tgt, tgt.background(), stats=st)
        assert np.array_equal(img, expected(name))
        assert st.edge_zero >= 50, st.edge_zero
        j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
        x, y = i + tgt.x0 + 0.5, j + tgt.y0 + 0.5
        for m, poly in f.outline.items():  # exactly once inside the union, never twice anywhere, never outside
            cnt = st.per_mesh[m]
            ins = inside_polygon(poly, x, y) & (i < tgt.width)
            assert int(ins.sum()) > 100 and np.all(cnt[ins] == 1), (m, np.unique(cnt[ins]))
            assert cnt.max() == 1 and not np.any(cnt[~ins & ~on_boundary_band(poly, x, y)]), m
        T = PM.triangles(f.pos, f.color, f.idx, f.meshes)
        A = PM.edge_exprs(T.a[:, 0], T.a[:, 1], T.b[:, 0], T.b[:, 1], T.c[:, 0], T.c[:, 1], 0, 0)[0]
        assert (A[T.valid] > 0).any() and (A[T.valid] < 0).any()                     # both windings
        assert int((T.valid & (A == 0)).sum()) == 1                                  # one zero-area triangle
        assert int((~T.valid).sum()) == 1                                            # one index >= num_vertices
        assert int((f.meshes["num_indices"] % 3 != 0).sum()) == 1                    # one remainder
        assert int(np.isnan(f.pos).any(axis=1).sum()) == 1 and int((T.valid & np.isnan(A)).sum()) == 1  # one NaN vertex, in one triangle
        assert (int(f.meshes["subpath_kind"][f.text_mesh]) >> 28) == TEXT and f.text_mesh not in st.per_mesh
        as_fill = f.meshes.copy()
        as_fill["subpath_kind"][f.text_mesh] = 0
        g = make("x", f.pos, f.color, f.idx, as_fill, tgt)
        assert not np.array_equal(render(g, tgt, tgt.background()), img)             # drawn, the TEXT mesh would show
    elif name == "stack":
        st = Stats(tgt)
        render(f, tgt, tgt.background(), stats=st)
        assert f.nm == 300 and int((f.meshes["num_indices"] // 3).sum()) > 256
        assert f.pos.min() >= 16 and f.pos.max() <= 32                               # one tile
        assert st.blends.max() > 30
        rev = render(f, tgt, tgt.background(), order=range(f.nm - 1, -1, -1))
        assert not np.array_equal(rev, expected(name))                               # the order matters
    elif name == "long":
        assert f.nm == 1 and int(f.meshes["num_indices"][0]) // 3 >= 600 and (int(f.meshes["subpath_kind"][0]) >> 28) == 3
        st = Stats(tgt)
        render(f, tgt, tgt.background(), stats=st)
        tj, ti = np.nonzero(st.blends)
        assert np.unique((tj // 16) * 1024 + ti // 16).size >= 12
        assert st.blends.max() >= 2                                                  # the joins overlap: the order inside a mesh shows
    elif name == "tiger":
        st = Stats(tgt)
        img = render(f, tgt, tgt.background(), stats=st)
        assert np.array_equal(img, expected(name))
        assert st.blends.max() >= 3
        assert st.fringe.any()
        sx0, sy0, sx1, sy1 = tgt.scissor
        assert 0 < sx0 and 0 < sy0 and sx1 < tgt.width and sy1 < tgt.height and tgt.stride > tgt.width and tgt.x0 < 0 and tgt.y0 < 0
        assert tgt.width % 16 and all(v % 16 for v in tgt.scissor)  # (160 rows are ten tiles; the scissor cuts the first and the last)
        for edge_px in (st.blends[sy0:sy1, sx0], st.blends[sy0:sy1, sx1 - 1], st.blends[sy0, sx0:sx1], st.blends[sy1 - 1, sx0:sx1]):
            assert edge_px.any()                                                     # cut on all four sides
        assert guards_intact(tgt, img)
    return True


def on_boundary_band(poly, x, y):
    """Samples ON the outline (the tie rule decides them; they are neither required nor forbidden)."""
    res = np.zeros(x.shape, dtype=bool)
    for k in range(len(poly)):
        (ux, uy), (vx, vy) = poly[k], poly[(k + 1) % len(poly)]
        e = (vx - ux) * (y - uy) - (vy - uy) * (x - ux)
        res |= (e == 0) & (x >= min(ux, vx)) & (x <= max(ux, vx)) & (y >= min(uy, vy)) & (y <= max(uy, vy))
    return res
