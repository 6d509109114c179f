"""vgx_raster_painted: a numpy statement of what include/vgx.h adds to vgx_raster_textured -- a mesh whose draw has type 1 or 2 takes
its colour from the gradient or the image pattern its draw names, evaluated at the pixel's sample -- the frames the CPU and GPU tests
share, and the conditions those frames must meet (tests/test_raster_painted_cpu.py: the lane code through libvgx_hosttest.so;
tests/test_gpu_raster_painted.py: the kernels).

Coverage and blend are raster_model's functions, the draw's rectangle raster_frame_model's, the texel rule and the status of sampled
meshes raster_textured_model's; this module adds the paint rule and the loop that applies it. It goes triangle by triangle in ascending
(mesh, triangle) order and knows nothing of mesh boxes, tiles or bins (the conditions of `crowd` and `classes` do: they are about the
kernels' tiles). numpy never fuses a multiply and an add, and its float64 square root is the IEEE one. Every comparison of images is
exact.
"""
import struct

import numpy as np

import cmdlist_util as cu
import raster_frame_model as M
import raster_model as R
import raster_textured_model as T

capi = R.capi
F = np.float32
D = np.float64
NONE = M.NONE
CLIP = M.CLIP
GRADIENT, PATTERN = 1, 2
UNUSED = 0xFFFFFFFF
NEAREST, CLAMP_U, CLAMP_V = T.NEAREST, T.CLAMP_U, T.CLAMP_V
CLEAR = T.CLEAR
Image = T.Image


# ---- paint records ----------------------------------------------------------------------------------------------------------
def unit(color):
    """0xAABBGGRR as the decoder's four floats c / 255.0f."""
    return [F((color >> (8 * k)) & 255) / F(255.0) for k in range(4)]


def inverse(fwd):
    """The inverse of the affine map (a, b, c, d, e, f): (x, y) -> (a x + c y + e, b x + d y + f), in float64, rounded to float32."""
    a, b, c, d, e, f = (float(v) for v in fwd)
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return [ia, ib, ic, id_, -(ia * e + ic * f), -(ib * e + id_ * f)]


def paint(typ, inv, params=(0, 0, 0, 0), inner=(0, 0, 0, 0), outer=(0, 0, 0, 0), image=0):
    """One vgx_paint (handle filled in by table()); inv = the six floats of m_Matrix's two rows; inner / outer: 0xAABBGGRR or four floats."""
    p = np.zeros(1, dtype=capi.paint_dtype)[0]
    p["type"] = typ
    with np.errstate(all="ignore"):
        p["matrix"] = np.array([inv[0], inv[1], 0, inv[2], inv[3], 0, inv[4], inv[5], 1], dtype=F)
        p["params"] = np.array(params, dtype=F)
        p["inner_color"] = np.array(unit(inner) if isinstance(inner, int) else inner, dtype=F)
        p["outer_color"] = np.array(unit(outer) if isinstance(outer, int) else outer, dtype=F)
    p["image"] = image
    return p


def linear_paint(fwd_xform, sx, sy, ex, ey, icol, ocol):
    """ctxCreateLinearGradient in float64 (the frames built by hand need not be the decoder's to the last bit)."""
    dx, dy = ex - sx, ey - sy
    dd = float(np.hypot(dx, dy))
    dx, dy = dx / dd, dy / dd
    large = 1e5
    g = (dy, -dx, dx, dy, sx - dx * large, sy - dy * large)
    return paint(GRADIENT, inverse(mul(fwd_xform, g)), (large, large + dd * 0.5, 0.0, max(1.0, dd)), icol, ocol)


def box_paint(fwd_xform, x, y, w, h, r, fe, icol, ocol, raw_feather=False):
    g = (1.0, 0.0, 0.0, 1.0, x + w * 0.5, y + h * 0.5)
    return paint(GRADIENT, inverse(mul(fwd_xform, g)), (w * 0.5, h * 0.5, r, fe if raw_feather else max(1.0, fe)), icol, ocol)


def radial_paint(fwd_xform, cx, cy, inr, outr, icol, ocol):
    r = (inr + outr) * 0.5
    return paint(GRADIENT, inverse(mul(fwd_xform, (1.0, 0.0, 0.0, 1.0, cx, cy))), (r, r, r, max(1.0, outr - inr)), icol, ocol)


def pattern_paint(fwd_xform, cx, cy, w, h, angle, image):
    cs, sn = np.cos(angle), np.sin(angle)
    inv = inverse(mul(fwd_xform, (cs, sn, -sn, cs, cx, cy)))
    return paint(PATTERN, [inv[0] / w, inv[1] / h, inv[2] / w, inv[3] / h, inv[4] / w, inv[5] / h], image=image)


def mul(a, b):
    """vgutil's multiplyMatrix3: the map b, then the map a."""
    return (a[0] * b[0] + a[2] * b[1], a[1] * b[0] + a[3] * b[1], a[0] * b[2] + a[2] * b[3], a[1] * b[2] + a[3] * b[3],
            a[0] * b[4] + a[2] * b[5] + a[4], a[1] * b[4] + a[3] * b[5] + a[5])


IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def table(records):
    """A paint table: entry k = records[k] with handle k, or an entry of type UNUSED for None."""
    t = np.zeros(len(records), dtype=capi.paint_dtype)
    for k, p in enumerate(records):
        if p is None:
            t[k]["type"] = UNUSED
        else:
            t[k] = p
            t[k]["handle"] = k
    return t


def scatter(paints):
    """The model's vgx_paint_tables with tables just large enough."""
    out = []
    for typ in (GRADIENT, PATTERN):
        mine = [p for p in paints if int(p["type"]) == typ]
        t = table([None] * (max(int(p["handle"]) for p in mine) + 1 if mine else 0))
        for p in mine:
            t[int(p["handle"])] = p
        out.append(t)
    return out


# ---- the specification ------------------------------------------------------------------------------------------------------
def q8(c):
    with np.errstate(all="ignore"):
        x = D(c) * 255.0 + 0.5
    if not x > 0:
        return 0
    if x >= 256:
        return 255
    return int(x)


def paint_coord(p, px, py):
    m = [D(v) for v in p["matrix"]]
    return (m[0] * px + m[3] * py) + m[6], (m[1] * px + m[4] * py) + m[7]


def gradient_t(p, qx, qy):
    """(t, t was a NaN before the clamps) of the gradient p at the paint coordinates."""
    ex, ey, rad, fe = (D(v) for v in p["params"])
    ax = np.abs(qx) - (ex - rad)
    ay = np.abs(qy) - (ey - rad)
    mx = np.where(ax > ay, ax, ay)
    inn = np.where(mx < 0.0, mx, 0.0)
    ox = np.where(ax > 0.0, ax, 0.0)
    oy = np.where(ay > 0.0, ay, 0.0)
    ln = np.sqrt(ox * ox + oy * oy)
    sd = (inn + ln) - rad
    t = (sd + fe * 0.5) / fe
    nan = np.isnan(t)
    t = np.where(t > 0.0, t, 0.0)
    t = np.where(t < 1.0, t, 1.0)
    return t, nan


def painted(fr, m):
    """GRADIENT / PATTERN when mesh m's draw (inside the table) has that type, else 0."""
    typ = (int(fr.draws["state_key"][int(fr.meshes["draw"][m])]) >> 16) & 0xF
    return typ if typ in (GRADIENT, PATTERN) else 0


def status(fr, mesh_begin=0, mesh_end=None, images=None, gradients=None, patterns=None):
    """What dev_status holds for a target whose scissor is not empty (VGX_E_GROWN aside)."""
    images = fr.images if images is None else images
    if T.status(fr, mesh_begin, mesh_end, images) != capi.VGX_OK:
        return capi.VGX_E_INVALID_ARG
    tabs = {GRADIENT: fr.gradients if gradients is None else gradients, PATTERN: fr.patterns if patterns is None else patterns}
    for m in range(mesh_begin, fr.nm if mesh_end is None else min(mesh_end, fr.nm)):
        typ = painted(fr, m)
        if typ:
            h = int(fr.draws["state_key"][int(fr.meshes["draw"][m])]) & 0xFFFF
            if h >= len(tabs[typ]) or int(tabs[typ][h]["type"]) != typ:
                return capi.VGX_E_INVALID_ARG
            if typ == PATTERN:
                im = int(tabs[typ][h]["image"]) & 0xFFFF
                if im >= len(images) or not T.image_valid(images[im]):
                    return capi.VGX_E_INVALID_ARG
    return capi.VGX_OK


class Stats(T.Stats):
    """T.Stats, and per painted mesh: samples blended with t == 0, t == 1, in between, with a t that was a NaN; samples blended under
    a vertex alpha strictly between 0 and 255; covered samples (blended or not); t per pixel of the last gradient sample there."""

    def __init__(self, tgt):
        T.Stats.__init__(self, tgt)
        self.t0, self.t1, self.tmid, self.tnan, self.fringe, self.covered = {}, {}, {}, {}, {}, {}
        self.t = np.full((tgt.rows(), tgt.stride), np.nan)

    def add(self, which, m, n):
        which[m] = which.get(m, 0) + int(n)


def render(fr, tgt, image, mesh_begin=0, mesh_end=None, images=None, gradients=None, patterns=None, stats=None, only=None):
    """Draws into `image` ([rows, stride] uint32, changed in place) and returns it. images / gradients / patterns: instead of the
    frame's; only: the meshes that write colour (the conditions only: the others still stamp)."""
    images = fr.images if images is None else images
    tabs = {GRADIENT: fr.gradients if gradients is None else gradients, PATTERN: fr.patterns if patterns is None else patterns}
    sx0, sy0, sx1, sy1 = tgt.scissor
    if sx0 >= sx1 or sy0 >= sy1 or status(fr, mesh_begin, mesh_end, images, tabs[GRADIENT], tabs[PATTERN]) != capi.VGX_OK:
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
        is_sampled = T.sampled(fr, m)
        typ = painted(fr, m)
        im = images[key & 0xFFFF] if is_sampled else None
        pt = tabs[typ][key & 0xFFFF] if typ else None
        if typ == PATTERN:
            im = images[int(pt["image"]) & 0xFFFF]
        if typ == GRADIENT:
            ends = [(q8(pt["inner_color"][ch]), q8(pt["outer_color"][ch])) for ch in range(4)]
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
                if stats is not None and typ:
                    stats.add(stats.covered, m, cov.sum())
                    stats.tie += int((cov & zero).sum())
                if is_sampled:
                    uv = T.uv_double(fr, safe[t])
                    u = ((E1 * uv[0, 0] + E2 * uv[1, 0]) + E0 * uv[2, 0]) / Sum
                    v = ((E1 * uv[0, 1] + E2 * uv[1, 1]) + E0 * uv[2, 1]) / Sum
                    U, V = u * D(im.width), v * D(im.height)
                    cov = cov & (np.abs(U) < 2147483648.0) & (np.abs(V) < 2147483648.0)  # a NaN compares false
                    tc = T.sample(im, U, V, cov, stats)
                    q = [T.div255(q[ch] * tc[ch]) for ch in range(4)]
                elif typ == PATTERN:
                    qx, qy = paint_coord(pt, px, py)
                    U, V = qx * D(im.width), qy * D(im.height)
                    cov = cov & (np.abs(U) < 2147483648.0) & (np.abs(V) < 2147483648.0)
                    tc = T.sample(im, U, V, cov, stats)
                    q = [T.div255(q[ch] * tc[ch]) for ch in range(4)]
                elif typ == GRADIENT:
                    qx, qy = paint_coord(pt, px, py)
                    tt, was_nan = gradient_t(pt, qx, qy)
                    g = [np.minimum(np.where(cov, D(I) * (1.0 - tt) + D(O) * tt + 0.5, 0).astype(np.int64), 255) for I, O in ends]
                    va = q[3]
                    q = [g[0], g[1], g[2], T.div255(g[3] * va)]
            view = image[win]
            hit = cov & (q[3] != 0)
            view[hit] = R.blend(view, q, q[3])[hit]
            if stats is not None:
                stats.blends[win] += hit
                stats.per_mesh.setdefault(m, np.zeros(stats.blends.shape, dtype=np.int32))[win] += hit
                if typ == GRADIENT:
                    stats.add(stats.t0, m, (hit & (tt == 0)).sum()); stats.add(stats.t1, m, (hit & (tt == 1)).sum())
                    stats.add(stats.tmid, m, (hit & (tt > 0) & (tt < 1)).sum()); stats.add(stats.tnan, m, (hit & was_nan).sum())
                    stats.add(stats.fringe, m, (hit & (va > 0) & (va < 255)).sum())
                    stats.t[win][hit] = tt[hit]
    return image


# ---- frames ---------------------------------------------------------------------------------------------------------
def finish(fr, mesh_draw, types, states, handles, uv, images, gradients, patterns):
    T.finish(fr, mesh_draw, types, states, handles, uv, images)
    fr.gradients, fr.patterns = table(gradients), table(patterns)
    return fr


class Rec(M.Rec):
    """The recorder with the paint commands (payloads as vgx_cmdlist_decode reads them)."""

    def linear_gradient(self, sx, sy, ex, ey, icol, ocol): self._cmd("CreateLinearGradient", struct.pack("<4fII", sx, sy, ex, ey, icol, ocol))
    def box_gradient(self, x, y, w, h, r, f, icol, ocol): self._cmd("CreateBoxGradient", struct.pack("<6fII", x, y, w, h, r, f, icol, ocol))
    def radial_gradient(self, cx, cy, inr, outr, icol, ocol): self._cmd("CreateRadialGradient", struct.pack("<4fII", cx, cy, inr, outr, icol, ocol))
    def image_pattern(self, cx, cy, w, h, angle, image): self._cmd("CreateImagePattern", struct.pack("<5fH", cx, cy, w, h, angle, image))
    def fill_gradient(self, flags, handle): self._cmd("FillPathGradient", struct.pack("<IHH", flags, handle, 0))
    def fill_pattern(self, flags, color, handle): self._cmd("FillPathImagePattern", struct.pack("<IIHH", flags, color, handle, 0))
    def stroke_gradient(self, width, flags, handle): self._cmd("StrokePathGradient", struct.pack("<fIHH", width, flags, handle, 0))
    def stroke_pattern(self, width, flags, color, handle): self._cmd("StrokePathImagePattern", struct.pack("<fIIHH", width, flags, color, handle, 0))


def from_bytes(rt, name, data, tgt, images, canvas=(256.0, 192.0)):
    """A command list decoded (vgx_cmdlist_decode runs on the host) and tessellated by the CPU oracle; the paint tables are the model's
    scatter of the decoder's records."""
    extra = {}
    rc, ps, draws, n = cu.decode(rt, data, canvas=canvas, extra=extra)
    assert rc == capi.VGX_OK and n["skipped"] == 0
    r = R.oracle.tessellate(ps, draws)
    fr = R.make(name, r.pos, r.color, r.idx, r.meshes, tgt)
    fr.draws, fr.dstate, fr.pathset, fr.paints = draws, extra["draw_state"], ps, extra["paints"].copy()
    fr.uv = np.full((max(fr.nv, 1), 2), np.nan, dtype=F)  # nobody reads it
    fr.images = list(images)
    fr.gradients, fr.patterns = scatter(fr.paints)
    return fr


AA = cu.fill_flags(aa=True)
NOAA = cu.fill_flags(aa=False)


def one_fill(rt, name):
    """linear / box / radial: one AA fill of a rounded rectangle under a rotated, non-uniformly scaled transform, on a target whose
    stride is above its width and whose origin is negative."""
    r = Rec()
    r.push_state(); r.transform_translate(6.0, -6.0); r.transform_rotate(0.35); r.transform_scale(1.6, 0.7)
    if name == "linear":
        r.linear_gradient(6.0, 8.0, 30.0, 34.0, 0xFF2040E0, 0xC0F0B020)
    elif name == "box":
        r.box_gradient(6.0, 6.0, 30.0, 36.0, 7.0, 9.0, 0xFFFFFFFF, 0x40201000)
    else:
        r.radial_gradient(20.0, 24.0, 4.0, 17.0, 0xFF30E0FF, 0x80FF2010)
    r.begin_path(); r.rounded_rect(1.0, 2.0, 40.0, 46.0, 5.0); r.fill_gradient(AA, 0)
    r.pop_state()
    return from_bytes(rt, name, r.bytes(), R.Target(80, 60, 83, -12, -9), [])


def clamps():
    """A box gradient with feather 1 and rad > ex (a negative inner extent): its ramp is one pixel wide, t == 0 and t == 1 are neighbours."""
    b = R.Builder()
    b.mesh(M.quad(2.0, 2.0, 44.0, 36.0), 0xFF000000, M.QUAD)
    fr = b.frame("clamps", R.Target(48, 40, 50, 0, 0))
    g = box_paint(IDENT, 20.0, 14.0, 6.0, 10.0, 8.0, 1.0, 0xFFFFE040, 0xFF2030A0)
    assert g["params"][2] > g["params"][0] and g["params"][3] == 1.0
    return finish(fr, [0], [GRADIENT], [M.state()], [0], np.full((fr.nv, 2), np.nan, dtype=F), [], [g], [])


def degenerate():
    """Eight quads, one draw each: (0) feather 0 with samples exactly on the rectangle's edge (0 / 0), (1) a NaN matrix entry, (2) an
    infinite one, (3) ends below 0 and above 1, (4) a NaN end, (5) a pattern whose coordinate is a NaN, (6) one whose texel coordinate
    reaches 2^31 half way, (7) a gradient whose params are all NaN."""
    b = R.Builder()
    cells = [(2 + 14 * (k % 4), 2 + 14 * (k // 4)) for k in range(8)]
    for x, y in cells:
        b.mesh(M.quad(x, y, x + 12.0, y + 12.0), 0xFF000000 if len(b.meshes) not in (5, 6) else 0xFFC0FF80, M.QUAD)
    fr = b.frame("degenerate", R.Target(60, 32, 61, 0, 0))
    x0, y0 = cells[0]
    g0 = box_paint(IDENT, x0 + 2.5, y0 + 2.5, 6.0, 6.0, 0.0, 0.0, 0xFF00FF00, 0xFF0000FF, raw_feather=True)
    g1 = box_paint(IDENT, cells[1][0] + 6.0, cells[1][1] + 6.0, 4.0, 4.0, 1.0, 3.0, 0xFFFF8000, 0xFF0080FF)
    g1["matrix"][0] = np.nan
    g2 = box_paint(IDENT, cells[2][0] + 6.0, cells[2][1] + 6.0, 4.0, 4.0, 1.0, 3.0, 0xFFFF8000, 0xFF0080FF)
    g2["matrix"][4] = np.inf
    g3 = radial_paint(IDENT, cells[3][0] + 6.0, cells[3][1] + 6.0, 1.0, 6.0, 0, 0)
    g3["inner_color"] = np.array([-0.5, 1.5, 0.25, 2.0], dtype=F)
    g3["outer_color"] = np.array([1.001, -1e-3, 1e30, 0.999], dtype=F)
    g4 = radial_paint(IDENT, cells[4][0] + 6.0, cells[4][1] + 6.0, 1.0, 6.0, 0xFF808080, 0xFFFFFFFF)
    g4["inner_color"][1] = np.nan
    g4["outer_color"][0] = -np.inf
    g7 = radial_paint(IDENT, cells[7][0] + 6.0, cells[7][1] + 6.0, 1.0, 6.0, 0xFF4080C0, 0xFF102030)
    g7["params"] = np.full(4, np.nan, dtype=F)
    p5 = pattern_paint(IDENT, 0.0, 0.0, 4.0, 4.0, 0.0, 0)
    p5["matrix"][6] = np.nan
    p6 = pattern_paint(IDENT, 0.0, 0.0, 4.0, 4.0, 0.0, 0)
    p6["matrix"][0] = F(2.0 ** 29 / 6.0)   # U = 4 * m0 * px + ...: 2^31 where px - x is 6 after the translation below
    p6["matrix"][6] = F(-(2.0 ** 29 / 6.0) * cells[6][0])
    im = Image(T.texels(4, 4, 4, 21, [255, 200]), 4, NEAREST)
    types = [GRADIENT] * 5 + [PATTERN, PATTERN, GRADIENT]
    handles = [0, 1, 2, 3, 4, 0, 1, 5]
    return finish(fr, list(range(8)), types, [M.state()] * 8, handles, np.full((fr.nv, 2), np.nan, dtype=F), [im], [g0, g1, g2, g3, g4, g7], [p5, p6])


PATTERN_VARIANTS = tuple("pattern_%s_%s" % (fl, w) for fl in ("nearest", "linear") for w in ("repeat", "clamp"))


def pattern_frame(name):
    """One AA-like quad (vertex alphas differ) under a rotated pattern whose image is far smaller than the quad, with a tint that is not
    white."""
    _, fl, w = name.split("_")
    flags = (NEAREST if fl == "nearest" else 0) | ((CLAMP_U | CLAMP_V) if w == "clamp" else 0)
    b = R.Builder()
    b.mesh([(3.25, 4.5), (58.5, 2.25), (60.75, 37.5), (5.5, 35.25)], [0xFF40C0FF, 0xC0FFFF80, 0xFF80FFFF, 0x80FFC0C0], M.QUAD, kind=R.TRILIST)
    fr = b.frame(name, R.Target(64, 40, 66, 0, 0))
    im = Image(T.texels(5, 3, 7, 22, [255, 90, 200, 0, 255]), 5, flags)
    p = pattern_paint((1.1, 0.2, -0.15, 0.9, 0.0, 0.0), 30.0, 18.0, 11.0, 7.5, 0.6, 0)
    return finish(fr, [0], [PATTERN], [M.state()], [0], np.full((fr.nv, 2), np.nan, dtype=F), [im], [], [p])


def seam():
    """Two triangles of one gradient draw that share an edge through pixel centres (corners on pixel centres), black vertices of
    alpha 255, gradient ends of alpha 128: a sample drawn twice would show."""
    b = R.Builder()
    b.mesh([(4.5, 5.5), (28.5, 5.5), (28.5, 17.5), (4.5, 17.5)], 0xFF000000, M.QUAD)
    fr = b.frame("seam", R.Target(36, 24, 37, 0, 0))
    g = linear_paint(IDENT, 4.0, 5.0, 29.0, 18.0, 0x80FF4020, 0x8020C0FF)
    return finish(fr, [0], [GRADIENT], [M.state()], [0], np.full((fr.nv, 2), np.nan, dtype=F), [], [g], [])


CROWD_SORTS = ("gradient0", "gradient1", "pattern", "text", "flat")


def crowd():
    """300 small translucent meshes on one 16 x 16 tile (x, y in 16 .. 32), in turn: gradient 0, gradient 1, the pattern, a sampled text
    quad, a flat mesh."""
    rs = np.random.RandomState(31)
    b = R.Builder()
    mesh_draw, uvs = [], []
    for k in range(300):
        c = rs.uniform(6, 10, 2) + 16
        r = rs.uniform(1.5, 5.9)
        sort = k % 5
        n = 4 if sort != 4 else 3 + (k // 5) % 2
        ang = rs.uniform(0, 6.28) + np.arange(n) * 6.28318 / n
        verts = [(c[0] + r * np.cos(t), c[1] + r * np.sin(t)) for t in ang]
        col = [int(rs.randint(40, 200)) << 24 | int(rs.randint(0, 1 << 24)) for _ in range(n)]
        b.mesh(verts, col, M.QUAD if n == 4 else [0, 1, 2], kind=R.TEXT if sort == 3 else (k % 2))
        mesh_draw.append(sort)
        if sort == 3:
            u0, v0 = rs.uniform(-0.5, 1.0, 2)
            uvs += [(u0, v0), (u0 + 0.6, v0), (u0 + 0.6, v0 + 0.7), (u0, v0 + 0.7)]
        else:
            uvs += [(np.nan, np.nan)] * n
    fr = b.frame("crowd", R.Target(48, 48, 48, 0, 0))
    images = [Image(T.texels(4, 4, 5, 5, [255, 128, 200]), 4, 0), Image(T.texels(3, 5, 3, 6, [90, 255]), 3, NEAREST | CLAMP_U)]
    g0 = radial_paint(IDENT, 24.0, 24.0, 1.0, 7.0, 0xE0FFFF00, 0x6000FFFF)
    g1 = linear_paint((0.8, 0.6, -0.6, 0.8, 0.0, 0.0), 20.0, 0.0, 34.0, 3.0, 0xFFFF00FF, 0x9000FF00)
    p = pattern_paint(IDENT, 17.0, 18.0, 6.0, 9.0, 0.4, 1)
    return finish(fr, mesh_draw, [GRADIENT, GRADIENT, PATTERN, 0, 0], [M.state()] * 5, [0, 1, 0, 0, 0], np.array(uvs, dtype=F), images, [g0, g1], [p])


def classes():
    """4 x 3 tiles; every mesh lies well inside one tile: flat meshes alone in some, a text quad in others, a painted quad in others, and
    text and paint together in others."""
    b = R.Builder()
    mesh_draw, uvs = [], []
    layout = {(0, 0): "f", (1, 0): "t", (2, 0): "g", (3, 0): "tg", (0, 1): "p", (1, 1): "fp", (2, 1): "ft", (3, 1): "f", (0, 2): "tp", (1, 2): "g", (2, 2): "", (3, 2): "t"}
    sorts = {"f": 0, "t": 1, "g": 2, "p": 3}
    for (tx, ty), what in sorted(layout.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        for k, ch in enumerate(what):
            x, y = 16 * tx + 2.25 + 3 * k, 16 * ty + 3.5 + 2 * k
            b.mesh(M.quad(x, y, x + 8.5, y + 7.25), [0xFF3060C0, 0xC0FFFFFF, 0xFFC06030, 0xE0FFFFFF], M.QUAD, kind=R.TEXT if ch == "t" else 1)
            mesh_draw.append(sorts[ch])
            uvs += [(0, 0), (1.5, 0), (1.5, 1.5), (0, 1.5)] if ch == "t" else [(np.nan, np.nan)] * 4
    fr = b.frame("classes", R.Target(64, 48, 64, 0, 0))
    fr.layout = layout
    images = [Image(T.texels(4, 4, 4, 23, [255, 160]), 4, 0)]
    g = linear_paint(IDENT, 0.0, 0.0, 64.0, 48.0, 0xFF00FFFF, 0xFFFF0040)
    p = pattern_paint(IDENT, 0.0, 0.0, 5.0, 5.0, 0.3, 0)
    return finish(fr, mesh_draw, [0, 0, GRADIENT, PATTERN], [M.state()] * 4, [0, 0, 0, 0], np.array(uvs, dtype=F), images, [g], [p])


STATE_VARIANTS = ("no_scissor", "no_in", "no_out", "no_stamp_mesh", "gradient_as_clip", "flat")


def state_frame(variant=None):
    """Painted draws under the state of a frame; `variant` takes one piece of that state away (the conditions only)."""
    b = R.Builder()
    mesh_draw, ty, st, hd = [], [], [], []

    def draw(typ, s, handle=0):
        ty.append(typ); st.append(s); hd.append(handle)
        return len(ty) - 1

    flat = variant == "flat"
    G, P = (0, 0) if flat else (GRADIENT, PATTERN)
    b.mesh(M.quad(-5.0, -5.0, 70.0, 60.0), 0xFF605040, M.QUAD)                                                 # 0 an opaque backdrop
    mesh_draw.append(draw(0, M.state()))
    clip_a = draw(CLIP, M.state(), 0xFFFF)                                                                       # 1 region A ...
    b.mesh(M.quad(6.25, 4.5, 30.5, 14.25), 0xFF000000, [] if variant == "no_stamp_mesh" else M.QUAD)
    mesh_draw.append(clip_a)
    inside = draw(CLIP if variant == "gradient_as_clip" else G, M.state(), 1)                                    # 2 ... a gradient draw recorded inside
    b.mesh(M.quad(26.5, 2.25, 38.25, 12.5), 0xFF000000, M.QUAD)                                               #   BeginClip .. EndClip: an ordinary draw
    mesh_draw.append(inside)
    clip_a2 = draw(CLIP, M.state(), 0xFFFF)                                                                      # 3 ... and the region's second clip draw
    b.mesh(M.quad(8.5, 12.25, 20.5, 20.75), 0xFF000000, M.QUAD)
    mesh_draw.append(clip_a2)
    d = draw(G, M.state(region=None if variant == "no_in" else (clip_a, 3), rule=0), 0)                        # 4 a gradient that straddles region A, In
    b.mesh(M.quad(2.5, 6.25, 34.5, 18.0), [0xFF000000, 0xC0000000, 0xFF000000, 0x80000000], M.QUAD)
    mesh_draw.append(d)
    clip_b = draw(CLIP, M.state(), 0xFFFF)                                                                       # 5 region B
    b.mesh(M.quad(40.5, 3.25, 52.25, 20.5), 0xFF000000, M.QUAD)
    mesh_draw.append(clip_b)
    d = draw(P, M.state(region=None if variant == "no_out" else (clip_b, 1), rule=1), 0)                       # 6 a pattern that straddles region B, Out
    b.mesh([(34.5, 2.25), (60.25, 5.5), (57.5, 23.25), (36.25, 19.5)], [0xFFFFFFFF, 0xC0FF80FF, 0xFF80FFFF, 0xA0FFFFFF], M.QUAD)
    mesh_draw.append(d)
    d = draw(G, M.state(scissor=M.BIG if variant == "no_scissor" else (9, 24, 22, 6)), 1)                      # 7 a gradient cut by its draw's scissor
    b.mesh(M.quad(3.25, 21.5, 40.0, 34.5), 0xE0000000, M.QUAD)
    mesh_draw.append(d)
    d = draw(P, M.state(scissor=M.BIG if variant == "no_scissor" else (40, 26, 14, 20)), 0)                    # 8 a pattern cut by its draw's scissor
    b.mesh(M.quad(36.5, 27.25, 60.25, 37.5), [0xFF2020E0, 0xFF20E020, 0xFFE02020, 0xFFE0E020], M.QUAD, kind=R.TRILIST)
    mesh_draw.append(d)
    fr = b.frame("state", R.Target(64, 40, 67, 0, 0, scissor=(1, 1, 63, 39)))
    images = [Image(T.texels(4, 4, 4, 8, [255, 120]), 4, 0)]
    g0 = linear_paint(IDENT, 2.0, 6.0, 35.0, 18.0, 0xFFFFFF00, 0xFF00FFFF)
    g1 = radial_paint(IDENT, 30.0, 10.0, 2.0, 26.0, 0xFFFF40FF, 0xFF40FF40)
    p = pattern_paint(IDENT, 34.0, 2.0, 9.0, 9.0, 0.25, 0)
    return finish(fr, mesh_draw, ty, st, hd, np.full((fr.nv, 2), np.nan, dtype=F), images, [g0, g1], [p])


# ---- decoded: command-list bytes with all four Create* commands and the four painted fills / strokes ----------------------------
DECODED_CANVAS = (96, 64)


def decoded_bytes():
    r = Rec()
    r.begin_path(); r.rect(0, 0, 96, 64); r.fill_path(0xFF403020, NOAA)
    r.push_state(); r.transform_translate(10.0, 6.0); r.transform_rotate(0.2); r.transform_scale(1.2, 0.8)
    r.linear_gradient(0.0, 0.0, 30.0, 20.0, 0xFF20C0FF, 0xFFFF4020)          # gradient 0
    r.image_pattern(4.0, 3.0, 12.0, 9.0, 0.5, 1)                               # pattern 0 on image 1
    r.begin_path(); r.rounded_rect(0.0, 0.0, 32.0, 22.0, 4.0); r.fill_gradient(AA, 0)
    r.begin_path(); r.move_to(2.0, 28.0); r.line_to(36.0, 30.0); r.line_to(20.0, 44.0); r.stroke_pattern(5.0, cu.stroke_flags(1, 1, True), 0xE0FFFFFF, 0)
    r.pop_state()
    r.push_state(); r.transform_translate(52.0, 8.0); r.transform_rotate(-0.15)
    r.box_gradient(2.0, 2.0, 30.0, 20.0, 5.0, 8.0, 0xC0000000, 0x00000000)     # gradient 1: a drop shadow
    r.radial_gradient(18.0, 38.0, 3.0, 13.0, 0xFFFFFFFF, 0x40FF00C0)           # gradient 2: a glow
    r.image_pattern(0.0, 0.0, 8.0, 8.0, 0.0, 0)                                # pattern 1 on image 0
    r.begin_path(); r.rect(-2.0, -2.0, 40.0, 30.0); r.fill_gradient(NOAA, 1)
    r.begin_path(); r.circle(18.0, 38.0, 12.0); r.stroke_gradient(4.0, cu.stroke_flags(0, 0, True), 2)
    r.begin_path(); r.circle(18.0, 38.0, 7.0); r.fill_pattern(AA, 0xFFC0FFFF, 1)
    r.pop_state()
    return r.bytes()


def decoded_images():
    return [Image(T.checker(), 8, NEAREST), Image(T.texels(6, 4, 6, 24, [255, 180]), 6, 0)]


def decoded(rt):
    w, h = DECODED_CANVAS
    return from_bytes(rt, "decoded", decoded_bytes(), R.Target(w, h, w + 3, 0, 0), decoded_images(), canvas=(float(w), float(h)))


NAMES = ("linear", "box", "radial", "clamps", "degenerate") + PATTERN_VARIANTS + ("seam", "crowd", "classes", "state", "decoded")
_frames = {}


def frame(name, rt=None):
    if name not in _frames:
        if name in ("linear", "box", "radial"):
            _frames[name] = one_fill(rt, name)
        elif name == "decoded":
            _frames[name] = decoded(rt)
        elif name.startswith("pattern"):
            _frames[name] = pattern_frame(name)
        else:
            _frames[name] = {"clamps": clamps, "degenerate": degenerate, "seam": seam, "crowd": crowd, "classes": classes, "state": state_frame}[name]()
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


def as_flat(fr):
    """The frame with the type of every painted draw set to 0: what vgx_raster_textured draws with vertex colours (a path-kind mesh of
    a type-0 draw is not sampled)."""
    g = R.make(fr.name, fr.pos, fr.color, fr.idx, fr.meshes.copy(), fr.target)
    g.draws, g.dstate, g.uv, g.images, g.gradients, g.patterns = fr.draws.copy(), fr.dstate, fr.uv, fr.images, fr.gradients, fr.patterns
    for d in range(g.draws.shape[0]):
        if ((int(g.draws["state_key"][d]) >> 16) & 0xF) in (GRADIENT, PATTERN):
            g.draws["state_key"][d] &= np.uint32(0xFFF0FFFF)
    return g


def tiles_of(fr, m):
    """The 16 x 16 tiles the box of mesh m reaches (the meshes of `crowd` and `classes` keep clear of tile borders)."""
    me = fr.meshes[m]
    p = fr.pos[int(me["first_vertex"]):int(me["first_vertex"]) + int(me["num_vertices"])]
    x0, y0, x1, y1 = p[:, 0].min() - fr.target.x0, p[:, 1].min() - fr.target.y0, p[:, 0].max() - fr.target.x0, p[:, 1].max() - fr.target.y0
    return {(tx, ty) for tx in range(int(x0) // 16, int(x1) // 16 + 1) for ty in range(int(y0) // 16, int(y1) // 16 + 1)}


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
    assert tgt.width <= 96 and tgt.height <= 64 and f.nm <= 400
    changed = img != tgt.background()
    pm = [m for m in range(f.nm) if painted(f, m)]
    assert pm
    if name in ("linear", "box", "radial"):
        assert tgt.stride > tgt.width and tgt.x0 < 0 and tgt.y0 < 0
        m = f.gradients[0]["matrix"]
        assert m[1] != 0 and m[3] != 0 and abs(abs(m[0]) - abs(m[4])) > 0.05            # rotated, and not a similarity
        for which in (st.t0, st.t1, st.tmid, st.fringe):
            assert sum(which.get(k, 0) for k in pm) >= 8, (name, which)
        assert (f.meshes["subpath_kind"][pm] >> 28 == capi.MESH_FILL_AA).all()
    elif name == "clamps":
        j0, i0 = np.nonzero(st.t == 0)
        j1, i1 = np.nonzero(st.t == 1)
        assert j0.size and j1.size and np.nanmax(np.where((st.t > 0) & (st.t < 1), 1, 0)) == 1
        dist = np.hypot(j0[:, None] - j1[None, :], i0[:, None] - i1[None, :])
        assert dist.min() <= 2.0, dist.min()
    elif name == "degenerate":
        assert st.t0.get(0, 0) > 0 and st.t1.get(0, 0) > 0 and st.tmid.get(0, 0) == 0 and st.tnan.get(0, 0) >= 4   # feather 0: a step, 0 / 0 on the edge
        for m in (1, 2, 7):
            assert st.per_mesh[m].sum() == st.covered[m] == 144, m                        # every sample is drawn, with whatever t the rule gives
        assert st.tnan.get(7, 0) == 144 and st.t0[7] == 144                              # NaN params: t is a NaN, taken as 0
        g3 = f.gradients[3]
        assert [q8(c) for c in g3["inner_color"]] == [0, 255, 64, 255] and [q8(c) for c in g3["outer_color"]] == [255, 0, 255, 255]
        assert [q8(c) for c in f.gradients[4]["inner_color"]][1] == 0 and q8(f.gradients[4]["outer_color"][0]) == 0   # NaN and -inf ends
        assert st.covered[5] == 144 and st.per_mesh[5].sum() == 0                             # a NaN coordinate: covered, left alone
        hit = st.per_mesh[6] > 0
        x = 2 + 14 * 2
        assert st.covered[6] == 144 and hit[16:28, x:x + 6].all() and not hit[:, x + 6:].any()   # 2^31 is reached half way
    elif name.startswith("pattern"):
        assert int(changed.sum()) > 1200
        im = f.images[0]
        x_lo, x_hi, y_lo, y_hi = st.raw[(im.width, im.height)]
        assert x_lo < 0 and y_lo < 0 and x_hi >= im.width and y_hi >= im.height          # wrapping is at work on both axes
        if "linear" in name:
            assert st.fractional > 500
        m = f.patterns[0]["matrix"]
        assert m[1] != 0 and m[3] != 0
        assert (f.color & 0xFFFFFF != 0xFFFFFF).all() and np.unique(f.color >> 24).size >= 3   # a tint, and alphas that differ
    elif name == "seam":
        assert st.tie >= 10, st.tie
        j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
        ins = R.inside_polygon([(4.5, 5.5), (28.5, 5.5), (28.5, 17.5), (4.5, 17.5)], i + 0.5, j + 0.5)
        assert st.blends.max() == 1 and np.all(st.blends[ins] == 1) and int(ins.sum()) == 23 * 11
        assert q8(f.gradients[0]["inner_color"][3]) == 128 and q8(f.gradients[0]["outer_color"][3]) == 128
    elif name == "crowd":
        assert f.nm > 256 and all(tiles_of(f, m) == {(1, 1)} for m in range(f.nm))       # more than 256 entries on one tile
        for s in range(5):
            mine = [m for m in range(f.nm) if int(f.meshes["draw"][m]) == s]
            assert len(mine) == 60 and min(mine) < 256 < max(mine)                         # on both sides of the reload
            others = [m for m in range(f.nm) if m not in mine]
            diff = render(f, tgt, tgt.background(), only=others) != img
            assert diff[16:32, 16:32].any(), CROWD_SORTS[s]
        assert T.sampled(f, 3) and not painted(f, 3) and painted(f, 0) == GRADIENT and painted(f, 2) == PATTERN
    elif name == "classes":
        cls = {}
        for m in range(f.nm):
            ts = tiles_of(f, m)
            assert len(ts) == 1
            c = cls.setdefault(next(iter(ts)), [False, False])
            c[0] |= T.sampled(f, m); c[1] |= bool(painted(f, m))
        assert tgt.width >= 48 and tgt.height >= 48
        for want in ((False, False), (True, False), (False, True), (True, True)):
            tiles = [t for t, c in cls.items() if tuple(c) == want]
            assert len(tiles) >= 2, want
            assert all(changed[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].any() for tx, ty in tiles), want
    elif name == "state":
        for v in STATE_VARIANTS:
            g = state_frame(v)
            other = render(g, tgt, tgt.background())
            assert int((other != img).sum()) >= 1, v
        assert st.stamped.any() and 1 not in st.per_mesh and 3 not in st.per_mesh
        assert st.per_mesh[2].sum() == st.covered[2] > 50                                 # the gradient draw inside BeginClip .. EndClip is drawn, untested
        for m in (4, 6):
            assert 0 < st.per_mesh[m].sum() and st.per_mesh[m].sum() <= st.covered[m]
        for m in (7, 8):
            rx0, ry0, rx1, ry1 = M.draw_rect(tgt, f.dstate["scissor"][int(f.meshes["draw"][m])])
            hit = st.per_mesh[m] > 0
            assert hit.any() and not hit[:, :rx0].any() and not hit[:, rx1:].any() and not hit[:ry0].any() and not hit[ry1:].any()
    elif name == "decoded":
        assert f.paints["type"].tolist() == [1, 2, 1, 1, 2] and f.paints["handle"].tolist() == [0, 0, 1, 2, 1]   # all four Create* commands
        types = (f.draws["state_key"] >> 16) & 0xF
        assert types.tolist() == [0, 1, 2, 1, 1, 2]                                       # fill / stroke x gradient / pattern
        for d in range(1, 6):
            ms = [m for m in range(f.nm) if int(f.meshes["draw"][m]) == d]
            assert ms and sum(st.per_mesh[m].sum() for m in ms if m in st.per_mesh) > 40, d
        assert {int(p["image"]) for p in f.patterns} == {0, 1}
    _checked[name] = True
    return True
