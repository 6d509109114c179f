"""vgx_raster_textured: a numpy statement of what include/vgx.h adds to vgx_raster_frame -- meshes of kind TEXT and TRILIST are drawn,
and under a draw of type 0 their colour is the vertex colour times a texel of the image the draw names -- the frames the CPU and GPU
tests share, and the conditions those frames must meet (tests/test_raster_textured_cpu.py: the lane code through libvgx_hosttest.so;
tests/test_gpu_raster_textured.py: the kernels).

Coverage and blend are raster_model's functions, the draw's rectangle and the status are raster_frame_model's; this module adds the
sampling rule and the loop that applies it. Like its two bases it goes triangle by triangle in ascending (mesh, triangle) order and
knows nothing of mesh boxes, tiles or bins. Every comparison of images is exact.
"""
import struct

import numpy as np

import cmdlist_util as cu
import raster_frame_model as M
import raster_model as R

capi = R.capi
F = np.float32
D = np.float64
NONE = M.NONE
CLIP = M.CLIP
NEAREST, CLAMP_U, CLAMP_V = capi.IMAGE_NEAREST, capi.IMAGE_CLAMP_U, capi.IMAGE_CLAMP_V
CLEAR = 0xFF102030
UV_GUARD = 0x5A  # the byte a UV stream holds where no sampled mesh has a vertex


class Image:
    """vgx_raster_image without the pointer: pixels is [height, stride] uint32."""

    def __init__(self, pixels, width, flags=0):
        self.pixels = np.ascontiguousarray(pixels, dtype=np.uint32)
        self.height, self.stride = self.pixels.shape
        self.width, self.flags = int(width), int(flags)

    def with_flags(self, flags):
        return Image(self.pixels, self.width, flags)

    def white(self):
        return Image(np.full(self.pixels.shape, 0xFFFFFFFF, dtype=np.uint32), self.width, self.flags)


def image_valid(im):
    return im is not None and 1 <= im.width <= 16384 and 1 <= im.height <= 16384 and im.stride >= im.width


def sampled(fr, m):
    """Mesh m is of kind TEXT / TRILIST and its draw (inside the table) has type 0."""
    d = int(fr.meshes["draw"][m])
    return (int(fr.meshes["subpath_kind"][m]) >> 28) in (R.TEXT, R.TRILIST) and ((int(fr.draws["state_key"][d]) >> 16) & 0xF) == 0


def status(fr, mesh_begin=0, mesh_end=None, images=None):
    """What dev_status holds for a target whose scissor is not empty (VGX_E_GROWN aside). images: instead of the frame's."""
    if M.status(fr, mesh_begin, mesh_end) != capi.VGX_OK:
        return capi.VGX_E_INVALID_ARG
    images = fr.images if images is None else images
    for m in range(mesh_begin, fr.nm if mesh_end is None else min(mesh_end, fr.nm)):
        if sampled(fr, m):
            h = int(fr.draws["state_key"][int(fr.meshes["draw"][m])]) & 0xFFFF
            if h >= len(images) or not image_valid(images[h]):
                return capi.VGX_E_INVALID_ARG
    return capi.VGX_OK


def div255(x):
    return (x + 127) // 255


def wrap(i, W, clamp):
    return np.clip(i, 0, W - 1) if clamp else np.mod(i, W)  # numpy's remainder has the sign of the divisor: Euclidean for W > 0


def sample(im, U, V, ok, stats=None):
    """The texel channels (four int64 arrays) of image `im` at the texel coordinates U, V (float64 arrays) where ok."""
    U, V = np.where(ok, U, 0.0), np.where(ok, V, 0.0)
    cu_, cv_ = bool(im.flags & CLAMP_U), bool(im.flags & CLAMP_V)
    if im.flags & NEAREST:
        ix, iy = np.floor(U).astype(np.int64), np.floor(V).astype(np.int64)
        if stats is not None:
            stats.note_raw(ix[ok], iy[ok], im)
        x, y = wrap(ix, im.width, cu_), wrap(iy, im.height, cv_)
        if stats is not None:
            stats.texels.update(zip(x[ok].tolist(), y[ok].tolist()))
        c = im.pixels[y, x].astype(np.int64)
        return [(c >> (8 * ch)) & 255 for ch in range(4)]
    Tx = np.floor((U - 0.5) * 256.0 + 0.5).astype(np.int64)
    Ty = np.floor((V - 0.5) * 256.0 + 0.5).astype(np.int64)
    x0r, y0r, wx, wy = Tx >> 8, Ty >> 8, Tx & 255, Ty & 255
    if stats is not None:
        stats.note_raw(np.concatenate([x0r[ok], x0r[ok] + 1]), np.concatenate([y0r[ok], y0r[ok] + 1]), im)
        stats.fractional += int(((wx != 0) & ok).sum()) + int(((wy != 0) & ok).sum())
    x0, x1, y0, y1 = wrap(x0r, im.width, cu_), wrap(x0r + 1, im.width, cu_), wrap(y0r, im.height, cv_), wrap(y0r + 1, im.height, cv_)
    if stats is not None:
        stats.texels.update(zip(x0[ok & (wx == 0) & (wy == 0)].tolist(), y0[ok & (wx == 0) & (wy == 0)].tolist()))
    c00, c10, c01, c11 = (im.pixels[y, x].astype(np.int64) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    out = []
    for ch in range(4):
        a, b, c, d = ((t >> (8 * ch)) & 255 for t in (c00, c10, c01, c11))
        out.append((a * (256 - wx) * (256 - wy) + b * wx * (256 - wy) + c * (256 - wx) * wy + d * wx * wy + 32768) >> 16)
    return out


class Stats:
    """What check_conditions looks at. blends: per pixel how often it was blended; per_mesh: the same per mesh; texels: the (x, y) a
    sample took whole (nearest, or linear with both weights 0); raw: per image width the lowest and highest index before wrapping, per
    axis; fractional: linear samples with a weight other than 0; tie: covered samples of sampled meshes with an edge value of 0."""

    def __init__(self, tgt):
        self.blends = np.zeros((tgt.rows(), tgt.stride), dtype=np.int32)
        self.per_mesh = {}
        self.texels = set()
        self.raw = {}
        self.fractional = 0
        self.tie = 0
        self.stamped = np.zeros((tgt.rows(), tgt.stride), dtype=bool)

    def note_raw(self, ix, iy, im):
        if ix.size:
            r = self.raw.setdefault((im.width, im.height), [ix.min(), ix.max(), iy.min(), iy.max()])
            r[0], r[1], r[2], r[3] = min(r[0], ix.min()), max(r[1], ix.max()), min(r[2], iy.min()), max(r[3], iy.max())


def uv_double(fr, v):
    """The UVs of the vertices v (an index array) as float64 [.., 2]: binary32 widened, or int16 / 32767."""
    if fr.uv.dtype == np.int16:
        return fr.uv[v].astype(D) / 32767.0
    return fr.uv[v].astype(D)


def render(fr, tgt, image, mesh_begin=0, mesh_end=None, images=None, stats=None, only=None):
    """Draws into `image` ([rows, stride] uint32, changed in place) and returns it. images: instead of the frame's; only: the meshes
    that write colour (the conditions only: the others still stamp)."""
    images = fr.images if images is None else images
    sx0, sy0, sx1, sy1 = tgt.scissor
    if sx0 >= sx1 or sy0 >= sy1 or status(fr, mesh_begin, mesh_end, images) != capi.VGX_OK:
        return image
    if tgt.clear is not None:
        image[sy0:sy1, sx0:sx1] = np.uint32(tgt.clear)
    nm = fr.meshes.shape[0]
    end = nm if mesh_end is None else min(mesh_end, nm)
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    S = np.full(image.shape, -1, dtype=np.int64)  # -1 = NONE
    for m in range(mesh_begin, end):
        me = fr.meshes[m]
        d = int(me["draw"])
        ds = fr.dstate[d]
        key = int(fr.draws["state_key"][d])
        rx0, ry0, rx1, ry1 = M.draw_rect(tgt, ds["scissor"])
        is_clip = ((key >> 16) & 0xF) == CLIP
        is_sampled = sampled(fr, m)
        im = images[key & 0xFFFF] if is_sampled else None
        f, n, rule = int(ds["clip_first_draw"]), int(ds["clip_num_draws"]), int(ds["clip_rule"])
        tested = not is_clip and f != NONE and n != 0
        nt, nv, fv, fi = int(me["num_indices"]) // 3, int(me["num_vertices"]), int(me["first_vertex"]), int(me["first_index"])
        if nt == 0:
            continue
        ids = fr.idx[fi:fi + 3 * nt].astype(np.int64).reshape(-1, 3)
        valid = (ids < nv).all(axis=1)
        safe = np.where(valid[:, None], ids, 0) + (fv if nv else 0)
        P, C = pos[safe], fr.color[safe]
        with np.errstate(all="ignore"):
            lo, hi = P.min(axis=1).astype(D), P.max(axis=1).astype(D)
            ok = valid & ~np.isnan(lo).any(axis=1) & ~np.isnan(hi).any(axis=1)
            i0 = np.clip(np.floor(np.where(ok, lo[:, 0], 0) - tgt.x0) - 2, sx0, sx1).astype(np.int64)
            i1 = np.clip(np.ceil(np.where(ok, hi[:, 0], 0) - tgt.x0) + 2, sx0, sx1).astype(np.int64)
            j0 = np.clip(np.floor(np.where(ok, lo[:, 1], 0) - tgt.y0) - 2, sy0, sy1).astype(np.int64)
            j1 = np.clip(np.ceil(np.where(ok, hi[:, 1], 0) - tgt.y0) + 2, sy0, sy1).astype(np.int64)
        for t in np.nonzero(ok & (i0 < i1) & (j0 < j1))[0]:
            a, b, c = P[t, 0], P[t, 1], P[t, 2]
            win = (slice(j0[t], j1[t]), slice(i0[t], i1[t]))
            jj, ii = np.mgrid[j0[t]:j1[t], i0[t]:i1[t]]
            px, py = (ii + tgt.x0).astype(D) + 0.5, (jj + tgt.y0).astype(D) + 0.5
            got = R.cover(a, b, c, px, py)
            if got is None:
                continue
            cov, E0, E1, E2, Sum, zero = got
            cov = cov & (ii >= rx0) & (ii < rx1) & (jj >= ry0) & (jj < ry1)
            if not cov.any():
                continue
            if is_clip:
                S[win][cov] = d
                if stats is not None:
                    stats.stamped[win] |= cov
                continue
            if tested:
                s = S[win]
                cov = cov & (((s != -1) & (s >= f) & (s - f < n)) == (rule == 0))
                if not cov.any():
                    continue
            if only is not None and m not in only:
                continue
            with np.errstate(all="ignore"):
                q = []
                for ch in range(4):
                    ca, cb, cc = (D((int(C[t, k]) >> (8 * ch)) & 255) for k in range(3))
                    v = ((E1 * ca + E2 * cb) + E0 * cc) / Sum
                    q.append(np.minimum(np.where(cov, v + 0.5, 0).astype(np.int64), 255))
                if is_sampled:
                    uv = uv_double(fr, safe[t])
                    u = ((E1 * uv[0, 0] + E2 * uv[1, 0]) + E0 * uv[2, 0]) / Sum
                    v = ((E1 * uv[0, 1] + E2 * uv[1, 1]) + E0 * uv[2, 1]) / Sum
                    U, V = u * D(im.width), v * D(im.height)
                    cov = cov & (np.abs(U) < 2147483648.0) & (np.abs(V) < 2147483648.0)  # a NaN compares false
                    if stats is not None:
                        stats.tie += int((cov & zero).sum())
                    tc = sample(im, U, V, cov, stats)
                    q = [div255(q[ch] * tc[ch]) for ch in range(4)]
            view = image[win]
            hit = cov & (q[3] != 0)
            view[hit] = R.blend(view, q, q[3])[hit]
            if stats is not None:
                stats.blends[win] += hit
                stats.per_mesh.setdefault(m, np.zeros(stats.blends.shape, dtype=np.int32))[win] += hit
    return image


# ---- frames ---------------------------------------------------------------------------------------------------------
def finish(fr, mesh_draw, types, states, handles, uv, images):
    """Attaches draws (type and image handle per draw), the UV stream ([nv, 2] float32 or int16) and the images to a raster_model frame."""
    M.with_draws(fr, mesh_draw, types, states)
    fr.draws["state_key"] |= np.asarray(handles, dtype=np.uint32)
    fr.uv = np.ascontiguousarray(uv)
    assert fr.uv.shape == (fr.nv, 2) and fr.uv.dtype in (np.float32, np.int16)
    fr.images = list(images)
    return fr


def uv_bytes(fr):
    return 8 if fr.uv.dtype == np.float32 else 4


def texels(w, h, stride, seed, alphas):
    """An image of distinct texels: [h, stride], the padding holds a value no texel has."""
    rs = np.random.RandomState(seed)
    px = np.full((h, stride), 0x00DEAD00, dtype=np.uint32)
    k = 0
    for y in range(h):
        for x in range(w):
            px[y, x] = (int(alphas[k % len(alphas)]) << 24) | (int(rs.randint(0, 256)) << 16) | (int(rs.randint(0, 256)) << 8) | ((17 * k + 3) & 255)
            k += 1
    assert np.unique(px[:, :w]).size == w * h
    return px


def blit(nearest):
    """One opaque-white-vertex quad whose UVs map a 5 x 3 image 1:1 onto the pixels (3 .. 8) x (2 .. 5)."""
    b = R.Builder()
    b.mesh(M.quad(3.0, 2.0, 8.0, 5.0), 0xFFFFFFFF, M.QUAD, kind=R.TRILIST)
    fr = b.frame("blit_nearest" if nearest else "blit_linear", R.Target(12, 9, 14, 0, 0))
    im = Image(texels(5, 3, 7, 1, [255, 0, 128, 1, 254, 77]), 5, NEAREST if nearest else 0)
    return finish(fr, [0], [0], [M.state()], [0], np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=F), [im])


WRAP_VARIANTS = tuple("wrap_%s_%s_%d%d" % (t, fl, cu_, cv_) for t in ("f", "i") for fl in ("n", "l") for cu_ in (0, 1) for cv_ in (0, 1))


def wrap_frame(name):
    """Two diamonds (quads turned by 45 degrees, corners on pixel centres, so their edges pass through pixel centres) with UVs from -1.25
    to 2.5 (float) or -1 to 1 (int16: its whole range) over a 2 x 2 and a 1 x 1 image. The two edges of a diamond that take ties are
    the ones on which u and v are at their highest: there, and only there, the int16 case reaches index W."""
    _, t, fl, cl = name.split("_")
    flags = (NEAREST if fl == "n" else 0) | (CLAMP_U if cl[0] == "1" else 0) | (CLAMP_V if cl[1] == "1" else 0)
    b = R.Builder()
    lo, hi = (-1.25, 2.5) if t == "f" else (-1.0, 1.0)
    uvs = []
    for k, (cx, cy, r) in enumerate(((15.5, 15.5, 13), (43.5, 16.5, 12))):
        corners = [(cx, cy - r), (cx + r, cy), (cx, cy + r), (cx - r, cy)]
        cols = [0xFFFFFFFF, 0xC0FF8040, 0xFF40FF80, 0x80FFFFFF]
        b.mesh(corners, cols, M.QUAD, kind=R.TEXT if k else R.TRILIST)
        uvs += [(hi, lo), (hi, hi), (lo, hi), (lo, lo)]  # top -> right carries u = hi, right -> bottom v = hi: the two edges that take ties
    fr = b.frame(name, R.Target(58, 31, 61, 0, 0))
    uv = np.array(uvs, dtype=F) if t == "f" else np.round(np.array(uvs) * 32767).astype(np.int16)
    images = [Image(texels(2, 2, 3, 2, [255, 96, 200, 40]), 2, flags), Image(texels(1, 1, 1, 3, [180]), 1, flags)]
    return finish(fr, [0, 1], [0, 0], [M.state(), M.state()], [0, 1], uv, images)


def seam():
    """A text run of 4 glyph quads of 6 x 6 pixels whose corners are pixel centres: the diagonals and the shared edges pass through
    pixel centres. Vertex alpha 128 over opaque texels: a sample drawn twice would show."""
    b = R.Builder()
    verts, ind, uvs = [], [], []
    for k in range(4):
        x0, y0 = 4.5 + 6 * k, 5.5
        verts += [(x0, y0), (x0 + 6, y0), (x0 + 6, y0 + 6), (x0, y0 + 6)]
        ind += [4 * k + i for i in (0, 1, 2, 0, 2, 3)]
        s0, t0 = (k % 2) * 0.5, (k // 2) * 0.5
        uvs += [(s0, t0), (s0 + 0.5, t0), (s0 + 0.5, t0 + 0.5), (s0, t0 + 0.5)]
    b.mesh(verts, 0x80FFFFFF, ind, kind=R.TEXT)
    fr = b.frame("seam", R.Target(36, 18, 37, 0, 0))
    px = texels(8, 8, 8, 4, [255])
    uv = (np.array(uvs, dtype=F) * F(32767)).astype(np.int32).astype(np.int16)  # as vgx_text_quads writes them
    return finish(fr, [0], [0], [M.state()], [0], uv, [Image(px, 8, 0)])


def crowd():
    """300 small translucent meshes on one 16 x 16 tile (x, y in 16 .. 32): of every three, two are sampled quads -- from two images in
    turn -- and one is a path-kind triangle or quad. More than 256 meshes and more than 256 sampled triangles on the tile."""
    rs = np.random.RandomState(11)
    b = R.Builder()
    mesh_draw, uvs = [], []
    ns = 0
    for k in range(300):
        c = rs.uniform(6, 10, 2) + 16
        r = rs.uniform(1.5, 5.9)
        is_s = k % 3 != 2
        n = 4 if is_s else 3 + k % 2
        ang = rs.uniform(0, 6.28) + np.arange(n) * 6.28318 / n
        verts = [(c[0] + r * np.cos(t), c[1] + r * np.sin(t)) for t in ang]
        col = [int(rs.randint(40, 200)) << 24 | int(rs.randint(0, 1 << 24)) for _ in range(n)]
        if is_s:
            b.mesh(verts, col, M.QUAD, kind=R.TEXT if ns % 4 < 2 else R.TRILIST)
            mesh_draw.append(ns % 2)
            ns += 1
            u0, v0 = rs.uniform(-0.5, 1.0, 2)
            uvs += [(u0, v0), (u0 + 0.6, v0), (u0 + 0.6, v0 + 0.7), (u0, v0 + 0.7)]
        else:
            b.mesh(verts, col if k % 2 else col[0], [0, 1, 2] if n == 3 else M.QUAD, kind=k % 2)
            mesh_draw.append(2)
            uvs += [(7.0, 7.0)] * n
    fr = b.frame("crowd", R.Target(48, 48, 48, 0, 0))
    images = [Image(texels(4, 4, 5, 5, [255, 128, 200]), 4, 0), Image(texels(3, 5, 3, 6, [90, 255]), 3, NEAREST | CLAMP_U)]
    return finish(fr, mesh_draw, [0, 0, 0], [M.state()] * 3, [0, 1, 0], np.array(uvs, dtype=F), images)


STATE_VARIANTS = ("no_scissor", "no_in", "no_out", "no_stamp_mesh", "stamp_as_textured", "paint_as_textured")


def glyph_run(b, x, y, n, w, h, color, cells):
    """n glyph quads of w x h from (x, y) to the right as ONE mesh of kind TEXT; returns their UVs (quarter cells of the atlas)."""
    verts, ind, uvs = [], [], []
    for k in range(n):
        x0 = x + k * (w + 1.25)
        verts += [(x0, y), (x0 + w, y), (x0 + w, y + h), (x0, y + h)]
        ind += [4 * k + i for i in (0, 1, 2, 0, 2, 3)]
        s0, t0 = (cells[k] % 2) * 0.5, (cells[k] // 2) * 0.5
        uvs += [(s0, t0), (s0 + 0.5, t0), (s0 + 0.5, t0 + 0.5), (s0, t0 + 0.5)]
    b.mesh(verts, color, ind, kind=R.TEXT)
    return uvs


def state_frame(variant=None):
    """Text and a user mesh under the state of a frame; `variant` takes one piece of that state away (the conditions only)."""
    b = R.Builder()
    uv, mesh_draw, ty, st, hd = [], [], [], [], []

    def draw(typ, s, handle=0):
        ty.append(typ); st.append(s); hd.append(handle)
        return len(ty) - 1

    def mesh_of(d, n):
        mesh_draw.append(d)

    white = [(0.9, 0.9)]
    b.mesh(M.quad(-5.0, -5.0, 70.0, 60.0), 0xFF605040, M.QUAD)                                   # 0 an opaque backdrop
    mesh_of(draw(0, M.state()), 4); uv += white * 4
    clip_a = draw(0 if variant == "stamp_as_textured" else CLIP, M.state(), 1)                   # 1 region A: a quad of kind TEXT, stamped not drawn
    b.mesh(M.quad(6.25, 4.5, 30.5, 14.25), 0xFFFFFFFF, [] if variant == "no_stamp_mesh" else M.QUAD, kind=R.TEXT)
    mesh_of(clip_a, 4); uv += [(0, 0), (1, 0), (1, 1), (0, 1)]
    d = draw(0, M.state(region=None if variant == "no_in" else (clip_a, 1), rule=0), 0)          # 2 a run that straddles region A, In
    uv += glyph_run(b, 2.5, 6.25, 5, 6.5, 7.0, 0xE0FFFFFF, [0, 1, 2, 3, 0]); mesh_of(d, 20)
    clip_b = draw(CLIP, M.state())                                                               # 3 region B: a path-kind quad
    b.mesh(M.quad(40.5, 3.25, 52.25, 20.5), 0xFFFFFFFF, M.QUAD)
    mesh_of(clip_b, 4); uv += white * 4
    d = draw(0, M.state(region=None if variant == "no_out" else (clip_b, 1), rule=1), 1)         # 4 a user mesh that straddles region B, Out
    b.mesh([(34.5, 2.25), (60.25, 5.5), (57.5, 23.25), (36.25, 19.5)], [0xFFFFFFFF, 0xC0FF80FF, 0xFF80FFFF, 0xA0FFFFFF], M.QUAD, kind=R.TRILIST)
    mesh_of(d, 4); uv += [(-0.5, -0.5), (1.5, -0.5), (1.5, 1.5), (-0.5, 1.5)]
    d = draw(0, M.state(scissor=M.BIG if variant == "no_scissor" else (9, 24, 22, 6)), 0)        # 5 a run whose draw scissor cuts its glyphs
    uv += glyph_run(b, 3.25, 21.5, 5, 7.0, 10.5, 0xFFFFFFFF, [3, 2, 1, 0, 3]); mesh_of(d, 20)
    d = draw(0 if variant == "paint_as_textured" else 1, M.state(), 1)                           # 6 a user mesh of a gradient draw: vertex colours
    b.mesh(M.quad(36.5, 27.25, 58.25, 36.5), [0xFF2020E0, 0xFF20E020, 0xFFE02020, 0xFFE0E020], M.QUAD, kind=R.TRILIST)
    mesh_of(d, 4); uv += [(0, 0), (2, 0), (2, 2), (0, 2)]
    fr = b.frame("state", R.Target(64, 40, 67, 0, 0, scissor=(1, 1, 63, 39)))
    atlas = texels(8, 8, 9, 7, [255, 255, 0, 160, 255, 30])
    images = [Image(atlas, 8, NEAREST), Image(texels(4, 4, 4, 8, [255, 120]), 4, 0)]
    return finish(fr, mesh_draw, ty, st, hd, np.array(uv, dtype=F), images)


# ---- decoded: command-list bytes with shapes, Text and IndexedTriList -------------------------------------------------------
DECODED_CANVAS = (200, 120)
DECODED_STRINGS = b"Hello, frame!" + b"vgx 0123"


def tri_list_command(pos, colors, idx, uv, image):
    """clIndexedTriList's record (the layout vgx_cmdlist_decode reads): nv, pos, nuv, uv, nc, colours, ni, idx, image."""
    pos, colors, idx = np.asarray(pos, F).reshape(-1, 2), np.asarray(colors, np.uint32).reshape(-1), np.asarray(idx, np.uint16).reshape(-1)
    uv = np.ascontiguousarray(uv)
    p = struct.pack("<I", pos.shape[0]) + pos.tobytes() + struct.pack("<I", uv.shape[0]) + uv.tobytes() + struct.pack("<I", colors.shape[0]) + colors.tobytes()
    p += struct.pack("<I", idx.shape[0]) + idx.tobytes() + struct.pack("<H", image)
    r = cu.Recorder()
    r._cmd("IndexedTriList", p)
    return r.bytes()


def decoded_bytes():
    import text_frame as TF
    AA = cu.fill_flags(aa=True)
    r = M.Rec()
    r.begin_path(); r.rounded_rect(8, 8, 120, 50, 6.0); r.fill_path(0xFF804020, AA)
    r.begin_path(); r.circle(150, 70, 30); r.fill_path(0xC020A0E0, AA)
    data = r.bytes()
    data += TF.text_command(dict(kind=0, string=DECODED_STRINGS[:13], x=14.0, y=40.0, font_size=18.0, color=0xFFFFFFFF, alignment=TF.ALIGN_LEFT | TF.ALIGN_BASELINE,
                                 font=0, break_width=0.0, flags=0), 0)
    r = M.Rec()
    r.set_scissor(100, 60, 70, 40)
    data += r.bytes()
    gp = [(96.0, 66.0), (180.0, 62.0), (176.0, 110.0), (92.0, 104.0)]
    guv = (np.array([(0, 0), (0.999, 0), (0.999, 0.999), (0, 0.999)]) * 32767).astype(np.int16)
    data += tri_list_command(gp, [0xFFFFFFFF, 0xC0FFFFFF, 0xFF80FF80, 0x80FFFFFF], M.QUAD, guv, 1)
    r = M.Rec()
    r.reset_scissor()
    r.push_state(); r.transform_translate(20, 90); r.transform_rotate(-0.2)
    data += r.bytes()
    data += TF.text_command(dict(kind=0, string=DECODED_STRINGS[13:], x=0.0, y=0.0, font_size=22.0, color=0xD040FFFF, alignment=TF.ALIGN_LEFT | TF.ALIGN_BASELINE,
                                 font=0, break_width=0.0, flags=0), 13)
    r = M.Rec()
    r.pop_state()
    r.begin_path(); r.move_to(10, 100); r.line_to(190, 112); r.stroke_path(0xFF00FFFF, 3.0, cu.stroke_flags(1, 1, True))
    return data + r.bytes()


def atlas():
    """A 64 x 64 glyph atlas without a font: 16 x 16 cells of 4 x 4 texels, each with a pattern of its own in the alpha channel."""
    y, x = np.mgrid[0:64, 0:64]
    cell = (y // 4) * 16 + (x // 4)
    bit = (cell * 2654435761 >> ((y % 4) * 4 + (x % 4))) & 1
    a = np.where(bit == 1, 255, 40 + (cell % 5) * 20)
    return ((a.astype(np.uint32) << 24) | 0x00FFFFFF).astype(np.uint32)


def checker():
    y, x = np.mgrid[0:8, 0:8]
    return np.where((x + y) % 2 == 0, 0xFF3030FF, 0xC0FFE020).astype(np.uint32)


def merge(capi_, A, ext, uv_dtype):
    """The model's vgx_merge_uv_stream: both sequences interleaved by draw (a mesh of A before a mesh of ext of the same draw), streams
    packed, the UV stream holding ext's UVs at the vertices of ext's meshes and UV_GUARD bytes elsewhere."""
    seq = [(int(m["draw"]), 0, k) for k, m in enumerate(A.meshes)] + [(int(m["draw"]), 1, k) for k, m in enumerate(ext["meshes"])]
    seq.sort(key=lambda t: (t[0], t[1]))  # stable
    meshes = np.zeros(len(seq), dtype=capi_.mesh_dtype)
    pos, col, idx, uv = [], [], [], []
    v = i = 0
    for k, (d, src, j) in enumerate(seq):
        m = A.meshes[j] if src == 0 else ext["meshes"][j]
        sp, sc, si = (A.pos, A.color, A.idx) if src == 0 else (ext["pos"], ext["color"], ext["idx"])
        v0, nv, i0, ni = int(m["first_vertex"]), int(m["num_vertices"]), int(m["first_index"]), int(m["num_indices"])
        meshes[k] = (v, i, nv, ni, d, int(m["subpath_kind"]))
        pos.append(np.asarray(sp, F).reshape(-1, 2)[v0:v0 + nv]); col.append(sc[v0:v0 + nv]); idx.append(si[i0:i0 + ni])
        uv.append(ext["uv"][v0:v0 + nv] if src == 1 else np.full((nv, 2), UV_GUARD, dtype=np.uint8).repeat(np.dtype(uv_dtype).itemsize, axis=1).view(uv_dtype))
        v += nv
        i += ni
    return np.concatenate(pos), np.concatenate(col), np.concatenate(idx), meshes, np.concatenate(uv), [s[1] for s in seq]


def decoded_parts(rt, text_fn=None):
    """(oracle tessellation of the decoded list, the external sequence, draws, draw state): what the device test merges itself."""
    import text_frame as TF
    extra = {}
    w, h = DECODED_CANVAS
    rc, ps, draws, n = cu.decode(rt, decoded_bytes(), canvas=(float(w), float(h)), extra=extra, font_image=0, white_uv=(0, 0),
                                 text=dict(strings_size=len(DECODED_STRINGS)))
    assert rc == capi.VGX_OK and n["skipped"] == 0
    A = R.oracle.tessellate(ps, draws)
    ext, runs = TF.external_meshes(capi, draws, extra, DECODED_STRINGS, False, text_fn or TF.host_text_fn(capi))
    return A, ext, draws, extra["draw_state"], ps, runs


def decoded(rt):
    A, ext, draws, dstate, ps, _ = decoded_parts(rt)
    pos, col, idx, meshes, uv, _ = merge(capi, A, ext, np.int16)
    w, h = DECODED_CANVAS
    fr = R.make("decoded", pos, col, idx, meshes, R.Target(w, h, w + 3, 0, 0))
    fr.draws, fr.dstate, fr.pathset = draws, dstate, ps
    fr.uv = np.ascontiguousarray(uv)
    fr.images = [Image(atlas(), 64, 0), Image(checker(), 8, NEAREST)]
    return fr


NAMES = ("blit_nearest", "blit_linear") + WRAP_VARIANTS + ("seam", "crowd", "state")
_frames = {}


def frame(name, rt=None):
    if name not in _frames:
        if name == "decoded":
            _frames[name] = decoded(rt)
        elif name.startswith("blit"):
            _frames[name] = blit(name == "blit_nearest")
        elif name.startswith("wrap"):
            _frames[name] = wrap_frame(name)
        else:
            _frames[name] = {"seam": seam, "crowd": crowd, "state": state_frame}[name]()
    return _frames[name]


_images = {}


def expected(name, clear=False, rt=None):
    """The model's image of a frame over its target's background: computed once per session, never changed."""
    key = (name, bool(clear))
    if key not in _images:
        f = frame(name, rt)
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        img = render(f, tgt, tgt.background())
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def as_fill(fr):
    """The frame's streams with the kind of every TEXT / TRILIST mesh rewritten to VGX_MESH_FILL_AA: what vgx_raster_frame draws with
    vertex colours. The sampled meshes, and with them the meshes of those kinds under a clip or a paint draw: vgx_raster_frame would
    skip these too, where vgx_raster_textured stamps or draws them."""
    g = R.make(fr.name, fr.pos, fr.color, fr.idx, fr.meshes.copy(), fr.target)
    for m in range(fr.nm):
        if (int(fr.meshes["subpath_kind"][m]) >> 28) in (R.TEXT, R.TRILIST):
            g.meshes["subpath_kind"][m] = capi.MESH_FILL_AA << 28
    g.draws, g.dstate = fr.draws, fr.dstate
    return g


# ---- conditions: each frame does what it is for, decided on the model alone ------------------------------------------------
_checked = {}


def check_conditions(name, rt=None):
    if name in _checked:
        return True
    f = frame(name, rt)
    tgt = f.target
    st = Stats(tgt)
    img = render(f, tgt, tgt.background(), stats=st)
    assert np.array_equal(img, expected(name, rt=rt))
    assert R.guards_intact(tgt, img)
    assert status(f) == capi.VGX_OK
    changed = img != tgt.background()
    if name != "decoded":
        assert tgt.width <= 64 and tgt.height <= 64
    if name.startswith("blit"):
        im = f.images[0]
        assert (im.width, im.height, im.stride) == (5, 3, 7) and st.texels == {(x, y) for x in range(5) for y in range(3)}  # every texel appears
        assert st.fractional == 0
        a = im.pixels[:, :5] >> 24
        assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    elif name.startswith("wrap"):
        assert int(changed.sum()) > 200, int(changed.sum())
        for im in f.images:  # below 0 and at or above W, before wrapping, on both axes, for either image
            x_lo, x_hi, y_lo, y_hi = st.raw[(im.width, im.height)]
            assert x_lo < 0 and y_lo < 0 and x_hi >= im.width and y_hi >= im.height, (name, im.width, st.raw)
        if "_l_" in name:
            assert st.fractional > 100
        if "_i_" in name:
            assert f.uv.dtype == np.int16 and int(f.uv.min()) == -32767 and int(f.uv.max()) == 32767
        else:
            assert float(f.uv.min()) == -1.25 and float(f.uv.max()) == 2.5
    elif name == "seam":
        assert st.tie >= 20, st.tie                                                  # samples exactly on an edge that were taken ...
        j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
        x, y = i + 0.5, j + 0.5
        ins = R.inside_polygon([(4.5, 5.5), (28.5, 5.5), (28.5, 11.5), (4.5, 11.5)], x, y)
        assert st.blends.max() == 1 and np.all(st.blends[ins] == 1) and int(ins.sum()) == 23 * 5   # ... once, and no hole inside
        assert int((f.color >> 24).max()) == 128
    elif name == "crowd":
        ns = [m for m in range(f.nm) if sampled(f, m)]
        assert f.nm > 256 and 2 * len(ns) > 256 and f.pos.min() >= 16 and f.pos.max() <= 32       # one tile: entries and triangles > 256
        kinds = f.meshes["subpath_kind"] >> 28
        assert set(np.unique(kinds[[m for m in range(f.nm) if m not in ns]])) <= {0, 1}            # path kinds in between
        for h in (0, 1):
            mine = [m for m in ns if (int(f.draws["state_key"][int(f.meshes["draw"][m])]) & 0xFFFF) == h]
            assert len(mine) > 64
            others = [m for m in range(f.nm) if m not in mine]
            assert not np.array_equal(render(f, tgt, tgt.background(), only=others), img)          # both images contribute
        assert [int(f.meshes["draw"][m]) for m in ns[:4]] == [0, 1, 0, 1]                          # interleaved mesh by mesh
        assert st.blends.max() > 30
    elif name == "state":
        for v in STATE_VARIANTS:
            g = state_frame(v)
            other = render(g, tgt, tgt.background())
            assert int((other != img).sum()) >= 1, v
        assert 1 not in st.per_mesh and st.stamped.any()                                          # the TEXT mesh of the clip draw stamps, draws nothing
        assert 6 in st.per_mesh and st.per_mesh[6].sum() > 50
        g = as_fill(f)
        plain = M.render(g, tgt, tgt.background())
        assert np.array_equal(plain[27:37, 36:59], img[27:37, 36:59])                             # mesh 6: its vertex colours
        rx0, ry0, rx1, ry1 = M.draw_rect(tgt, f.dstate["scissor"][5])
        hit = st.per_mesh[5] > 0
        assert hit.any() and not hit[:, :rx0].any() and not hit[:, rx1:].any() and not hit[:ry0].any() and not hit[ry1:].any()
    elif name == "decoded":
        assert tgt.width <= 256 and tgt.height <= 256
        kinds = f.meshes["subpath_kind"] >> 28
        ns = [m for m in range(f.nm) if sampled(f, m)]
        assert (kinds == R.TEXT).sum() >= 2 and (kinds == R.TRILIST).sum() >= 1 and len(ns) >= 3 and len(ns) < f.nm
        for m in ns:
            assert m in st.per_mesh and st.per_mesh[m].sum() > 50, m
        assert {int(f.draws["state_key"][int(f.meshes["draw"][m])]) & 0xFFFF for m in ns} == {0, 1}
        assert len({tuple(int(v) for v in s) for s in f.dstate["scissor"]}) >= 2
    _checked[name] = True
    return True
