"""vgx_raster_concave: a numpy statement of what include/vgx.h adds to vgx_raster_painted -- a mesh of kind VGX_MESH_CONTOURS is filled by
the winding number of its directed edges -- the frames the CPU and GPU tests share, and the conditions those frames must meet
(tests/test_raster_concave_cpu.py: the lane code through libvgx_hosttest.so; tests/test_gpu_raster_concave.py: the kernels).

The model is built ON raster_painted_model, not beside it: `covered` states the winding rule per sample, and `lower` replaces every
contour mesh by one small flat triangle around each covered sample (the sample is its centroid, it reaches no other sample), at the
mesh's place in the stream and under the mesh's draw. The painted model then draws the lowered frame: blend, clip stamp, In / Out, both
scissors, gradient, pattern and painter's order are its statements, applied to "a covered sample of vertex colour c" exactly as the
header words it. The producer (vgx_concave_contours) is stated in tests/test_concave_contours_cpu.py, on the concave oracle helpers of
tests/test_gpu_concave.py (libtess2's boundary contours, the reference's strokerConcaveFillEndAA). Every comparison of images is exact.
"""
import numpy as np

import raster_frame_model as M
import raster_model as R
import raster_painted_model as P
import raster_textured_model as T

capi = R.capi
F = np.float32
D = np.float64
CLEAR = P.CLEAR
CONTOURS = capi.MESH_CONTOURS
EVEN_ODD = capi.CONTOUR_EVEN_ODD
GRADIENT, PATTERN, CLIP = P.GRADIENT, P.PATTERN, P.CLIP


# ---- the specification ------------------------------------------------------------------------------------------------------
def is_contours(fr, m):
    return (int(fr.meshes["subpath_kind"][m]) >> 28) == CONTOURS


def mesh_edges(fr, m):
    """The valid directed edges of contour mesh m as ([n, 2] float32 u, [n, 2] float32 v)."""
    me = fr.meshes[m]
    ne, nv, fv, fi = int(me["num_indices"]) // 2, int(me["num_vertices"]), int(me["first_vertex"]), int(me["first_index"])
    ids = fr.idx[fi:fi + 2 * ne].astype(np.int64).reshape(-1, 2)
    ids = ids[(ids < nv).all(axis=1)]
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    return pos[fv + ids[:, 0]], pos[fv + ids[:, 1]]


def winding(u, v, px, py):
    """W at the samples (float64 arrays) over the directed edges u[k] -> v[k] (float32 pairs): int32."""
    W = np.zeros(px.shape, dtype=np.int32)
    with np.errstate(all="ignore"):
        for a, b in zip(u, v):
            up = (D(a[1]) < py) & (py <= D(b[1]))
            dn = (D(b[1]) < py) & (py <= D(a[1]))
            if not (up.any() or dn.any()):
                continue
            E, _ = R.edge(a, b, 1.0, px, py)  # s = +1: the canonical value of u -> v itself
            W += (up & (E < 0)).astype(np.int32) - (dn & (E > 0)).astype(np.int32)
    return W


def mesh_box(fr, m):
    me = fr.meshes[m]
    nv, fv = int(me["num_vertices"]), int(me["first_vertex"])
    p = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)[fv:fv + nv]
    return None if nv == 0 else (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max())


def covered(fr, m, tgt, stats=None):
    """[rows, stride] bool: the samples of the image contour mesh m covers (the scissors come later, with every other rule)."""
    j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
    px, py = (i + tgt.x0).astype(D) + 0.5, (j + tgt.y0).astype(D) + 0.5
    box = mesh_box(fr, m)
    if box is None:
        return np.zeros(px.shape, dtype=bool)
    u, v = mesh_edges(fr, m)
    W = winding(u, v, px, py)
    if stats is not None:
        stats[m] = W
    with np.errstate(all="ignore"):
        inbox = (px >= D(box[0])) & (px <= D(box[2])) & (py >= D(box[1])) & (py <= D(box[3]))
    rule = (W & 1) != 0 if int(fr.meshes["subpath_kind"][m]) & EVEN_ODD else W != 0
    cov = inbox & rule
    cov[:, tgt.width:] = False
    cov[tgt.height:] = False
    return cov


def lower(fr, tgt, mesh_begin=0, mesh_end=None, windings=None):
    """The frame with every contour mesh of the range replaced by one flat triangle per covered sample. Returns (frame, map): map[k] =
    the mesh of `fr` that mesh k of the result stands for. Meshes outside the range are dropped (the caller draws the whole result)."""
    end = fr.nm if mesh_end is None else min(mesh_end, fr.nm)
    pos, col, idx, uv, meshes, back = [], [], [], [], [], []
    nv = ni = 0
    fpos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    for m in range(mesh_begin, end):
        me = fr.meshes[m]
        if is_contours(fr, m):
            jj, ii = np.nonzero(covered(fr, m, tgt, windings))
            n = jj.size
            assert 3 * n < 65536
            sx, sy = (ii + tgt.x0).astype(D) + 0.5, (jj + tgt.y0).astype(D) + 0.5
            p = np.stack([sx - 0.25, sy - 0.25, sx + 0.375, sy - 0.125, sx - 0.125, sy + 0.375], axis=1).reshape(-1, 2)
            assert np.array_equal(p.astype(F).astype(D), p)
            c = int(fr.color[int(me["first_vertex"])]) if n else 0
            pos.append(p.astype(F)); col.append(np.full(3 * n, c, dtype=np.uint32)); idx.append(np.arange(3 * n, dtype=np.uint16))
            uv.append(np.full((3 * n, 2), np.nan, dtype=fr.uv.dtype) if fr.uv.dtype == np.float32 else np.zeros((3 * n, 2), dtype=fr.uv.dtype))
            meshes.append((nv, ni, 3 * n, 3 * n, int(me["draw"]), capi.MESH_FILL << 28))
            nv += 3 * n; ni += 3 * n
        else:
            a, k, b, q = int(me["first_vertex"]), int(me["num_vertices"]), int(me["first_index"]), int(me["num_indices"])
            pos.append(fpos[a:a + k]); col.append(fr.color[a:a + k]); idx.append(fr.idx[b:b + q]); uv.append(fr.uv[a:a + k])
            meshes.append((nv, ni, k, q, int(me["draw"]), int(me["subpath_kind"])))
            nv += k; ni += q
        back.append(m)
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    g = R.make(fr.name, cat(pos, np.zeros((0, 2), F)), cat(col, np.zeros(0, np.uint32)), cat(idx, np.zeros(0, np.uint16)),
               np.array(meshes, dtype=capi.mesh_dtype), tgt)
    g.draws, g.dstate, g.images, g.gradients, g.patterns = fr.draws, fr.dstate, fr.images, fr.gradients, fr.patterns
    g.uv = np.ascontiguousarray(cat(uv, np.zeros((0, 2), fr.uv.dtype)))
    if g.nv == 0:
        g.pos, g.color, g.uv = np.zeros((1, 2), F), np.zeros(1, np.uint32), np.zeros((1, 2), fr.uv.dtype)
    return g, back


def status(fr, mesh_begin=0, mesh_end=None):
    """What dev_status holds (VGX_E_GROWN aside): the painted level's, which looks at draws, handles and tables, never at a kind's indices."""
    return P.status(fr, mesh_begin, mesh_end)


def render(fr, tgt, image, mesh_begin=0, mesh_end=None, stats=None):
    """Draws into `image` ([rows, stride] uint32, changed in place) and returns it."""
    if status(fr, mesh_begin, mesh_end) != capi.VGX_OK:
        return image
    g, back = lower(fr, tgt, mesh_begin, mesh_end)
    if stats is not None:
        stats.back = back
    return P.render(g, tgt, image, stats=stats)


def without_contours(fr):
    """The frame with its contour meshes emptied (0 vertices, 0 indices): what the four older raster calls must draw."""
    g = R.make(fr.name, fr.pos, fr.color, fr.idx, fr.meshes.copy(), fr.target)
    g.draws, g.dstate, g.uv, g.images, g.gradients, g.patterns = fr.draws, fr.dstate, fr.uv, fr.images, fr.gradients, fr.patterns
    for m in range(g.nm):
        if is_contours(g, m):
            g.meshes["num_vertices"][m] = 0
            g.meshes["num_indices"][m] = 0
            g.meshes["subpath_kind"][m] = 0
    return g


# ---- which edges does a tile keep? (the conditions only: the kernel's rule, restated) ---------------------------------------------
def tile_keeps(tgt, tx, ty, u, v):
    """Edge u -> v against tile (tx, ty) of a target whose scissor is the image: (min y, max y] meets the tile's sample rows and min x
    does not exceed its largest sample x."""
    py0, py1 = tgt.y0 + 16 * ty + 0.5, tgt.y0 + min(16 * ty + 15, tgt.height - 1) + 0.5
    px1 = tgt.x0 + min(16 * tx + 15, tgt.width - 1) + 0.5
    lo, hi = min(u[1], v[1]), max(u[1], v[1])
    return bool(lo < hi and lo < py1 and hi >= py0 and min(u[0], v[0]) <= px1)


# ---- frames -----------------------------------------------------------------------------------------------------------------
def ring_indices(counts, first=0):
    """The closed rings of consecutive vertex runs of the given lengths: edge (i, i + 1), the closing edge included."""
    out = []
    for n in counts:
        for k in range(n):
            out += [first + k, first + (k + 1) % n]
        first += n
    return out


class Builder(R.Builder):
    def contours(self, rings, color, even_odd=False, indices=None, num_vertices=None):
        verts = [tuple(p) for r in rings for p in r]
        m = self.mesh(verts, color, ring_indices([len(r) for r in rings]) if indices is None else indices, kind=CONTOURS, num_vertices=num_vertices)
        if even_odd:
            a = self.meshes[m]
            self.meshes[m] = a[:5] + (a[5] | EVEN_ODD,)
        return m


def finish(fr, mesh_draw=None, types=None, states=None, handles=None, uv=None, images=(), gradients=(), patterns=()):
    """Defaults: every mesh under one colour draw without a scissor."""
    mesh_draw = [0] * fr.nm if mesh_draw is None else mesh_draw
    types = [0] if types is None else types
    states = [M.state()] * len(types) if states is None else states
    handles = [0] * len(types) if handles is None else handles
    uv = np.full((fr.nv, 2), np.nan, dtype=F) if uv is None else uv
    return P.finish(fr, mesh_draw, types, states, handles, uv, list(images), list(gradients), list(patterns))


def star(cx, cy, r0, r1, points, phase=0.0):
    a = phase + np.arange(2 * points) * (np.pi / points)
    rad = np.where(np.arange(2 * points) % 2 == 0, r0, r1)
    return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], axis=1).astype(F)


def star_polygon(cx, cy, r, n, step, phase=0.0):
    """{n / step}: n vertices on a circle joined every `step`-th: self-intersecting, winding numbers up to `step`."""
    a = phase + (np.arange(n) * step % n) * (2 * np.pi / n)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).astype(F)


def star300():
    """Inside ONE 16 x 16 tile (x, y in 16 .. 32): a 300-edge star (NonZero), then a {151 / 50} star polygon (EvenOdd). With the flushes
    454 records: W is carried across the 256-record batch, in the middle of the first mesh's edges."""
    b = Builder()
    b.mesh(M.quad(17.25, 17.5, 31.0, 30.75), 0xFF405060, M.QUAD)
    b.contours([star(24.1, 24.3, 7.4, 3.2, 150, 0.01)], 0xC03070F0)
    b.contours([star_polygon(23.9, 23.8, 7.7, 151, 50, 0.02)], 0xA0F0C020, even_odd=True)
    return finish(b.frame("star300", R.Target(48, 48, 48, 0, 0)))


BLOB = [(3.3, 4.2), (40.5, 2.7), (84.2, 5.9), (86.6, 44.1), (83.7, 85.3), (50.2, 86.8), (44.6, 70.3), (38.1, 87.4), (4.9, 84.6), (2.2, 40.8),
        (9.7, 30.4), (2.9, 20.6)]


def inner():
    """A concave shape over 6 x 6 tiles on a target with negative origin and padded stride: tiles deep inside hold no edge of it (all
    kept edges lie to their left), and its last edges are culled from most tiles."""
    b = Builder()
    b.contours([np.array(BLOB, dtype=F) - F(6.0)], 0xD020C060)
    b.contours([np.array(BLOB, dtype=F)[::-1] * F(0.4) + F(20.0)], 0x80F04020, even_odd=True)   # clockwise input
    return finish(b.frame("inner", R.Target(90, 88, 93, -7, -5)))


def crowd():
    """300 small translucent meshes on one tile (x, y in 16 .. 32), in turn: a triangle mesh, a NonZero contour pentagon, an EvenOdd
    pentagram."""
    rs = np.random.RandomState(41)
    b = Builder()
    for k in range(300):
        c = rs.uniform(6, 10, 2) + 16
        r = rs.uniform(1.5, 5.9)
        col = int(rs.randint(40, 200)) << 24 | int(rs.randint(0, 1 << 24))
        if k % 3 == 0:
            ang = rs.uniform(0, 6.28) + np.arange(3) * 6.28318 / 3
            b.mesh([(c[0] + r * np.cos(t), c[1] + r * np.sin(t)) for t in ang], col, [0, 1, 2])
        elif k % 3 == 1:
            b.contours([star_polygon(c[0], c[1], r, 5, 1, rs.uniform(0, 6.28))], col)
        else:
            b.contours([star_polygon(c[0], c[1], r, 5, 2, rs.uniform(0, 6.28))], col, even_odd=True)
    return finish(b.frame("crowd", R.Target(48, 48, 48, 0, 0)))


L_SHAPE = [(4.5, 4.5), (20.5, 4.5), (20.5, 10.5), (11.5, 10.5), (11.5, 21.5), (4.5, 21.5)]


def centres():
    """Vertices and horizontal / vertical edges exactly on pixel centres (every coordinate a half-integer); a ring with its reversed
    duplicate (everything cancels); a diamond whose vertices are pixel centres."""
    b = Builder()
    b.contours([L_SHAPE], 0x80FF8040)
    ring = [(24.5, 3.5), (33.5, 5.5), (30.5, 14.5), (23.5, 11.5)]
    b.contours([ring, ring[::-1]], 0xFFFFFFFF)
    b.contours([[(28.5, 16.5), (34.5, 22.5), (28.5, 28.5), (22.5, 22.5)]], 0x8040C0FF)
    return finish(b.frame("centres", R.Target(40, 32, 41, 0, 0)))


def aa_seam():
    """The AA pair of a rectangle at integer coordinates with fringe 1, built by hand: the moved contour and the fringe's inner edge lie
    ON pixel centres, colour alpha 128: a sample drawn twice, or not at all, shows."""
    b = Builder()
    x0, y0, x1, y1 = 4.0, 4.0, 20.0, 14.0
    inn = M.quad(x0 + 0.5, y0 + 0.5, x1 - 0.5, y1 - 0.5)
    out = M.quad(x0 - 0.5, y0 - 0.5, x1 + 0.5, y1 + 0.5)
    verts, cols, idx = [], [], []
    for k in range(4):
        verts += [inn[k], out[k]]
        cols += [0x80FF8040, 0x00FF8040]
        i0, i2 = 2 * k, 2 * ((k + 1) % 4)
        idx += [i0, i2, i0 + 1, i2, i2 + 1, i0 + 1]
    b.mesh(verts, cols, idx, kind=capi.MESH_CONCAVE_FILL_AA)
    b.contours([inn], 0x80FF8040)
    return finish(b.frame("aa_seam", R.Target(26, 20, 27, 0, 0)))


def odd():
    """A trailing odd index, an out-of-range index (its edge is skipped: the ring stays open and the box clause bounds the half-line), an
    open polyline, a mesh of zero vertices with indices, a mesh of one horizontal edge."""
    b = Builder()
    sq = M.quad(3.25, 3.5, 12.75, 11.25)
    b.contours([sq], 0xFF20A0E0, indices=ring_indices([4]) + [2])
    b.contours([M.quad(16.25, 3.5, 27.5, 12.25) + [(40.0, 8.0)]], 0xC0E0A020, indices=[0, 1, 1, 7, 2, 3, 3, 0], num_vertices=4)
    b.contours([[(5.25, 15.5), (9.5, 27.25), (14.75, 16.25)]], 0xFFA020E0, indices=[0, 1, 1, 2])
    b.contours([M.quad(20.0, 16.0, 30.0, 26.0)], 0xFFFFFFFF, num_vertices=0)
    b.contours([[(2.0, 29.5), (30.0, 29.5)]], 0xFFFFFFFF, indices=[0, 1, 1, 0])
    return finish(b.frame("odd", R.Target(34, 32, 36, 0, 0)))


STATE_VARIANTS = ("no_scissor", "no_in", "no_out", "no_stamp_mesh", "flat")
NOTCH = lambda x, y, w, h: [(x, y), (x + w, y), (x + w, y + h), (x + 0.6 * w, y + h), (x + 0.5 * w, y + 0.4 * h), (x + 0.4 * w, y + h), (x, y + h)]


def state_frame(variant=None):
    """Contour meshes under the state of a frame: AS the clip region, under In and Out, under a draw scissor, under a gradient, a pattern
    and a Textured draw. `variant` takes one piece away (the conditions only)."""
    b = Builder()
    mesh_draw, ty, st, hd = [], [], [], []

    def draw(typ, s, handle=0):
        ty.append(typ); st.append(s); hd.append(handle)
        return len(ty) - 1

    G, Pt = (0, 0) if variant == "flat" else (GRADIENT, PATTERN)
    b.mesh(M.quad(-5.0, -5.0, 70.0, 60.0), 0xFF605040, M.QUAD)                                            # 0 an opaque backdrop
    mesh_draw.append(draw(0, M.state()))
    clip_a = draw(CLIP, M.state(), 0xFFFF)                                                                  # 1 region A: a contour mesh stamps
    b.contours([NOTCH(6.25, 4.5, 24.0, 12.0)], 0xFF000000, indices=[] if variant == "no_stamp_mesh" else None)
    mesh_draw.append(clip_a)
    b.contours([NOTCH(2.5, 3.25, 34.0, 16.0)], 0xC0F0E010)                                                  # 2 a contour mesh tested In against A
    mesh_draw.append(draw(0, M.state(region=None if variant == "no_in" else (clip_a, 1), rule=0)))
    clip_b = draw(CLIP, M.state(), 0xFFFF)                                                                  # 3 region B: a triangle mesh stamps
    b.mesh(M.quad(40.5, 3.25, 52.25, 20.5), 0xFF000000, M.QUAD)
    mesh_draw.append(clip_b)
    b.contours([star(48.0, 12.0, 11.0, 5.0, 7, 0.3)], 0xFF40E0A0, even_odd=True)                           # 4 a gradient star tested Out against B
    mesh_draw.append(draw(G, M.state(region=None if variant == "no_out" else (clip_b, 1), rule=1), 0))
    b.contours([NOTCH(3.25, 21.5, 30.0, 14.0)], 0xE0FFFFFF)                                                 # 5 a pattern cut by its draw's scissor
    mesh_draw.append(draw(Pt, M.state(scissor=M.BIG if variant == "no_scissor" else (9, 24, 19, 7)), 0))
    b.contours([star(48.0, 30.0, 8.0, 3.0, 5, 0.1)], 0xB02060FF)                                            # 6 under a Textured draw: flat
    mesh_draw.append(draw(0, M.state(), 0))
    fr = b.frame("state", R.Target(64, 40, 67, 0, 0, scissor=(1, 1, 63, 39)))
    images = [T.Image(T.texels(4, 4, 4, 8, [255, 120]), 4, 0)]
    g0 = P.radial_paint(P.IDENT, 48.0, 12.0, 2.0, 12.0, 0xFFFF40FF, 0xC040FF40)
    p = P.pattern_paint(P.IDENT, 4.0, 22.0, 9.0, 9.0, 0.25, 0)
    return finish(fr, mesh_draw, ty, st, hd, images=images, gradients=[g0], patterns=[p])


CLASS_LAYOUT = {(0, 0): "f", (1, 0): "c", (2, 0): "t", (3, 0): "ct", (0, 1): "g", (1, 1): "cg", (2, 1): "tp", (3, 1): "ctp", (0, 2): "C", (1, 2): "", (2, 2): "fc", (3, 2): "p"}


def classes():
    """4 x 3 tiles, every mesh well inside one tile: flat, sampled (t), painted (g, p) and contour meshes (c; C = a gradient contour mesh)
    in every combination of the three per-tile bits the level can meet."""
    b = Builder()
    mesh_draw, uvs = [], []
    sorts = {"f": 0, "t": 1, "g": 2, "p": 3, "c": 0, "C": 2}
    for (tx, ty), what in sorted(CLASS_LAYOUT.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        for k, ch in enumerate(what):
            x, y = 16 * tx + 2.25 + 2 * k, 16 * ty + 2.5 + 2 * k
            if ch in "cC":
                b.contours([NOTCH(x, y, 8.5, 7.25)], 0xC0E06030)
                uvs += [(np.nan, np.nan)] * 7
            else:
                b.mesh(M.quad(x, y, x + 8.5, y + 7.25), [0xFF3060C0, 0xC0FFFFFF, 0xFFC06030, 0xE0FFFFFF], M.QUAD, kind=R.TEXT if ch == "t" else 1)
                uvs += [(0, 0), (1.5, 0), (1.5, 1.5), (0, 1.5)] if ch == "t" else [(np.nan, np.nan)] * 4
            mesh_draw.append(sorts[ch])
    fr = b.frame("classes", R.Target(64, 48, 64, 0, 0))
    images = [T.Image(T.texels(4, 4, 4, 23, [255, 160]), 4, 0)]
    g = P.linear_paint(P.IDENT, 0.0, 0.0, 64.0, 48.0, 0xFF00FFFF, 0xFFFF0040)
    p = P.pattern_paint(P.IDENT, 0.0, 0.0, 5.0, 5.0, 0.3, 0)
    return finish(fr, mesh_draw, [0, 0, GRADIENT, PATTERN], None, None, np.array(uvs, dtype=F), images, [g], [p])


NAMES = ("star300", "inner", "crowd", "centres", "aa_seam", "odd", "state", "classes")
_MAKERS = {"star300": star300, "inner": inner, "crowd": crowd, "centres": centres, "aa_seam": aa_seam, "odd": odd, "state": state_frame, "classes": classes}
_frames, _images, _checked = {}, {}, {}


def frame(name):
    if name not in _frames:
        _frames[name] = _MAKERS[name]()
    return _frames[name]


def expected(name, clear=False):
    """The model's image of a frame over its target's background: computed once per session, never changed."""
    key = (name, bool(clear))
    if key not in _images:
        f = frame(name)
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        img = render(f, tgt, tgt.background())
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def tiles_of(fr, m):
    x0, y0, x1, y1 = mesh_box(fr, m)
    t = fr.target
    return {(tx, ty) for tx in range(int(x0 - t.x0) // 16, int(x1 - t.x0) // 16 + 1) for ty in range(int(y0 - t.y0) // 16, int(y1 - t.y0) // 16 + 1)}


# ---- conditions: each frame does what it is for, decided on the model alone ----------------------------------------------------
def check_conditions(name):
    if name in _checked:
        return True
    f = frame(name)
    tgt = f.target
    st = P.Stats(tgt)
    img = render(f, tgt, tgt.background(), stats=st)
    assert np.array_equal(img, expected(name)) and R.guards_intact(tgt, img) and status(f) == capi.VGX_OK
    assert tgt.width <= 96 and tgt.height <= 96 and f.nm <= 400
    changed = img != tgt.background()
    cm = [m for m in range(f.nm) if is_contours(f, m)]
    assert cm
    hits = lambda m: int(st.per_mesh[m].sum()) if m in st.per_mesh else 0
    if name == "star300":
        assert all(tiles_of(f, m) == {(1, 1)} for m in range(f.nm))
        ne = [int(f.meshes["num_indices"][m]) // 2 for m in cm]
        assert ne == [300, 151] and 2 + ne[0] > 256                       # (the quad's two triangles come first)
        u, v = mesh_edges(f, 1)
        assert sum(tile_keeps(tgt, 1, 1, a, b) for a, b in zip(u, v)) == 300   # nothing of it is culled: the batch boundary falls inside the mesh
        W = {}
        covered(f, 2, tgt, W)
        assert np.abs(W[2]).max() >= 30 and hits(1) > 60 and hits(2) > 40         # deep winding, parity decides
    elif name == "inner":
        assert tgt.stride > tgt.width and tgt.x0 < 0 and tgt.y0 < 0
        u, v = mesh_edges(f, 0)
        deep = [(tx, ty) for tx in range(6) for ty in range(6) if st.per_mesh[0][16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].all()
                and not any(min(a[0], b[0]) - tgt.x0 < 16 * tx + 16 and max(a[0], b[0]) - tgt.x0 > 16 * tx
                            and min(a[1], b[1]) - tgt.y0 < 16 * ty + 16 and max(a[1], b[1]) - tgt.y0 > 16 * ty for a, b in zip(u, v))]
        assert len(deep) >= 4                                              # covered whole, and no edge's box meets them
        for tx, ty in deep:
            kept = [(a, b) for a, b in zip(u, v) if tile_keeps(tgt, tx, ty, a, b)]
            assert kept and all(max(a[0], b[0]) - tgt.x0 <= 16 * tx for a, b in kept)   # what they keep lies to their left
        culled = [t for t in tiles_of(f, 0) if not tile_keeps(tgt, t[0], t[1], u[-1], v[-1]) and not tile_keeps(tgt, t[0], t[1], u[-2], v[-2])]
        assert len(culled) >= 10                                           # the last edges are culled there: the flush still has to fire
        assert hits(1) > 300 and len(BLOB) == 12
    elif name == "crowd":
        assert f.nm > 256 and all(tiles_of(f, m) == {(1, 1)} for m in range(f.nm))
        for s in range(3):
            mine = [m for m in range(f.nm) if m % 3 == s]
            assert min(mine) < 256 < max(mine) and sum(hits(m) for m in mine) > 1000
    elif name == "centres":
        assert (f.pos * 2 == np.round(f.pos * 2)).all() and ((f.pos * 2) % 2 == 1).all()
        assert hits(1) == 0 and hits(0) > 150 and hits(2) > 50
        j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
        x, y = i + 0.5, j + 0.5
        got = st.per_mesh[0] > 0   # the two rectangles of the L: ties on the right and bottom edges in, on the left and top edges out
        assert np.array_equal(got, ((x > 4.5) & (x <= 20.5) & (y > 4.5) & (y <= 10.5)) | ((x > 4.5) & (x <= 11.5) & (y > 4.5) & (y <= 21.5)))
        assert not got[4, 5] and not got[5, 4] and got[21, 5] and got[5, 20] and got[10, 19] and not got[11, 19]
    elif name == "aa_seam":
        assert st.blends.max() == 1
        assert np.all(st.blends[4:14, 4:20] == 1) and np.all(st.per_mesh[1][5:14, 5:20] == 1) and hits(1) == 15 * 9   # the interior takes the seam's right and bottom
        assert st.per_mesh[0][4:14, 4].all() and st.per_mesh[0][4, 4:20].all()   # ... and the fringe its left and top, all of them pixel centres
    elif name == "odd":
        assert hits(0) > 60 and hits(3) == 0 and hits(4) == 0
        box = mesh_box(f, 1)
        got = st.per_mesh[1] > 0
        assert got.any() and not got[:, int(np.ceil(box[2])):].any()       # the open ring's half-line ends at the box
        W = {}
        covered(f, 1, tgt, W)
        assert (W[1][:, int(np.ceil(box[2])) + 1:tgt.width] != 0).any()     # ... where W alone would go on
        assert hits(2) > 20
    elif name == "state":
        for v in STATE_VARIANTS:
            other = render(state_frame(v), tgt, tgt.background())
            assert int((other != img).sum()) >= 1, v
        assert st.stamped.any() and hits(1) == 0 and hits(3) == 0
        for m in (2, 4, 5, 6):
            assert hits(m) > 20, m
        assert hits(2) < int(covered(f, 2, tgt).sum()) and hits(4) < int(covered(f, 4, tgt).sum()) and hits(5) < int(covered(f, 5, tgt).sum())
    elif name == "classes":
        seen = set()
        for t, what in CLASS_LAYOUT.items():
            bits = ("c" in what or "C" in what, "t" in what, "g" in what or "p" in what or "C" in what)
            seen.add(bits)
            assert not what or changed[16 * t[1]:16 * t[1] + 16, 16 * t[0]:16 * t[0] + 16].any()
        assert len(seen) == 8 and all(len(tiles_of(f, m)) == 1 for m in range(f.nm))
    _checked[name] = True
    return True
