"""vgx_raster_frame: a numpy statement of what include/vgx.h adds to vgx_raster -- the scissor of every draw, the stamp S of every
pixel, clip draws that write it and the other draws that are tested against it -- the frames the CPU and GPU tests share, and the
conditions those frames must meet (tests/test_raster_frame_cpu.py: the lane code through libvgx_hosttest.so;
tests/test_gpu_raster_frame.py: the kernels).

Coverage, colour and blend are raster_model's own functions (raster_model.cover / blend), used as they are: this module adds the loop
that carries S and cuts by the draw's scissor. Like raster_model it goes triangle by triangle in ascending (mesh, triangle) order and
knows nothing of mesh boxes, tiles or bins. Every comparison of images is exact.
"""
import functools
import struct

import numpy as np

import cmdlist_util as cu
import raster_model as R

capi = R.capi
F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
CLIP = 3  # DrawCommand::Type::Clip in (state_key >> 16) & 0xF
BIG = (0, 0, 4000, 4000)  # a draw scissor that cuts nothing here


class Stats:
    """Per mesh, samples the coverage rule takes inside the target's scissor: `accept` took effect, `cut` fell outside the draw's
    scissor, `reject` failed the stamp test -- split into `reject_over` (a clip draw of the mesh's own region had stamped the pixel
    before and a later one overwrote it) and `reject_never`; `untouched` = accepted by an untested mesh where S was NONE. blends: as
    raster_model's, per pixel."""

    def __init__(self, tgt, nm):
        self.blends = np.zeros((tgt.rows(), tgt.stride), dtype=np.int32)
        self.per_mesh = {}
        for k in ("accept", "cut", "reject", "reject_over", "reject_never", "untouched"):
            setattr(self, k, np.zeros(nm, dtype=np.int64))


def draw_rect(tgt, sc):
    """The target's scissor cut by the draw scissor {x, y, w, h}, in image pixels, half open: integers throughout."""
    sx0, sy0, sx1, sy1 = tgt.scissor
    x, y, w, h = (int(v) for v in sc)
    return max(sx0, x - tgt.x0), max(sy0, y - tgt.y0), min(sx1, x + w - tgt.x0), min(sy1, y + h - tgt.y0)


def status(fr, mesh_begin=0, mesh_end=None):
    """What dev_status holds for a target whose scissor is not empty (VGX_E_GROWN aside)."""
    end = fr.nm if mesh_end is None else min(mesh_end, fr.nm)
    if mesh_begin < end and (fr.meshes["draw"][mesh_begin:end] >= fr.draws.shape[0]).any():
        return capi.VGX_E_INVALID_ARG
    return capi.VGX_OK


def render(fr, tgt, image, mesh_begin=0, mesh_end=None, order=None, stats=None, ignore_clips=False, order_free=False):
    """Draws into `image` ([rows, stride] uint32, changed in place) and returns it. The conditions only -- order: the meshes in
    another order; ignore_clips: clip draws do nothing and no draw is tested (scissors stay); order_free: the stamp rule replaced by
    "S ever equalled a draw of the region"."""
    sx0, sy0, sx1, sy1 = tgt.scissor
    if sx0 >= sx1 or sy0 >= sy1 or status(fr, mesh_begin, mesh_end) != capi.VGX_OK:
        return image
    if tgt.clear is not None:
        image[sy0:sy1, sx0:sx1] = np.uint32(tgt.clear)
    nm = fr.meshes.shape[0]
    end = nm if mesh_end is None else min(mesh_end, nm)
    pos = np.ascontiguousarray(fr.pos, dtype=F).reshape(-1, 2)
    S = np.full(image.shape, -1, dtype=np.int64)  # -1 = NONE
    ever = {}                                     # draw -> pixels it ever stamped
    for m in (range(mesh_begin, end) if order is None else order):
        me = fr.meshes[m]
        if (int(me["subpath_kind"]) >> 28) in (R.TEXT, R.TRILIST):
            continue
        d = int(me["draw"])
        ds = fr.dstate[d]
        rx0, ry0, rx1, ry1 = draw_rect(tgt, ds["scissor"])
        is_clip = ((int(fr.draws["state_key"][d]) >> 16) & 0xF) == CLIP
        f, n, rule = int(ds["clip_first_draw"]), int(ds["clip_num_draws"]), int(ds["clip_rule"])
        tested = not is_clip and not ignore_clips and f != NONE and n != 0
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
            cov, E0, E1, E2, Sum, _ = got
            in_draw = (ii >= rx0) & (ii < rx1) & (jj >= ry0) & (jj < ry1)
            if stats is not None:
                stats.cut[m] += int((cov & ~in_draw).sum())
            cov = cov & in_draw
            if not cov.any():
                continue
            if is_clip:
                if not ignore_clips:
                    S[win][cov] = d
                    ever.setdefault(d, np.zeros(image.shape, dtype=bool))[win] |= cov
                    if stats is not None:
                        stats.accept[m] += int(cov.sum())
                continue
            if tested:
                s = S[win]
                was = np.zeros(s.shape, dtype=bool)
                for k in range(f, f + n):
                    if k in ever:
                        was |= ever[k][win]
                member = was if order_free else ((s != -1) & (s >= f) & (s - f < n))
                passed = member == (rule == 0)
                if stats is not None:
                    stats.reject[m] += int((cov & ~passed).sum())
                    stats.reject_over[m] += int((cov & ~passed & was).sum())
                    stats.reject_never[m] += int((cov & ~passed & ~was).sum())
                cov = cov & passed
                if not cov.any():
                    continue
            elif stats is not None:
                stats.untouched[m] += int((cov & (S[win] == -1)).sum())
            if stats is not None:
                stats.accept[m] += int(cov.sum())
            with np.errstate(all="ignore"):
                q = []
                for ch in range(4):
                    ca, cb, cc = (D((int(C[t, k]) >> (8 * ch)) & 255) for k in range(3))
                    v = ((E1 * ca + E2 * cb) + E0 * cc) / Sum
                    q.append(np.minimum(np.where(cov, v + 0.5, 0).astype(np.int64), 255))
            view = image[win]
            hit = cov & (q[3] != 0)
            view[hit] = R.blend(view, q, q[3])[hit]
            if stats is not None:
                stats.blends[win] += hit
                stats.per_mesh.setdefault(m, np.zeros(stats.blends.shape, dtype=np.int32))[win] += hit
    return image


# ---- frames ---------------------------------------------------------------------------------------------------------
def state(scissor=BIG, region=None, rule=0):
    """One vgx_draw_state as a tuple; region = (first draw, draws) or None."""
    f, n = (NONE, 0) if region is None else region
    return (tuple(scissor), rule, f, n, 0)


def with_draws(fr, mesh_draw, types, states):
    """Attaches the draw table to a raster_model frame: mesh m belongs to draw mesh_draw[m]; draw d has type types[d] and the
    vgx_draw_state states[d]."""
    fr.meshes = fr.meshes.copy()
    fr.meshes["draw"] = np.asarray(mesh_draw, dtype=np.uint32)
    fr.draws = np.zeros(len(types), dtype=capi.draw_dtype)
    fr.draws["state_key"] = (np.asarray(types, dtype=np.uint32) << 16) | (np.arange(len(types), dtype=np.uint32) << 20)  # a generation per draw
    fr.dstate = np.array(states, dtype=capi.draw_state_dtype)
    assert fr.dstate.shape[0] == fr.draws.shape[0]
    return fr


def quad(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


QUAD = [0, 1, 2, 0, 2, 3]


def clips():
    """Frame pixels (-4 .. 82) x (-3 .. 71) are inside the target's scissor. Meshes = draws, one each."""
    b = R.Builder()
    st, ty = [], []

    def add(verts, colors, indices, kind, typ, s):
        b.mesh(verts, colors, indices, kind=kind)
        ty.append(typ)
        st.append(s)
        return len(ty) - 1

    add(quad(-20.0, -20.0, 120.0, 100.0), 0xFF605040, QUAD, 0, 0, state())                                   # 0 an opaque backdrop
    ring = [(25.5 + 15 * np.cos(k * np.pi / 4), 30.5 + 15 * np.sin(k * np.pi / 4)) for k in range(8)]
    fan = [i for k in range(8) for i in (0, 1 + k, 1 + (k + 1) % 8)]
    first = add([(25.5, 30.5)] + ring, 0xFF00FF00, fan, 0, CLIP, state())                                       # 1 region 1: a fan ...
    strip_v = [(30.25 + 5 * (k // 2), 20.5 if k % 2 == 0 else 40.75) for k in range(12)]                        # ... and a quad strip to x = 55.25
    strip_i = [i for k in range(0, 10, 2) for i in (k, k + 1, k + 2, k + 1, k + 3, k + 2)]
    add(strip_v, [0x80FF00FF + k for k in range(12)], strip_i, 1, CLIP, state(scissor=(28, 18, 22, 30)))        # 2 its own scissor ends at x = 50
    r1 = (first, 2)
    big = [(5.25, 5.5), (75.5, 4.25), (76.75, 64.5), (4.5, 66.25)]
    add(big, [0x60FF2020, 0xC020FF20, 0x202020FF, 0xA0FFFF20], QUAD, 1, 0, state(region=r1, rule=0))            # 3 translucent AA, larger than region 1, In
    second = add(quad(40.5, 25.25, 70.25, 55.5), 0xFFFFFFFF, QUAD, 0, CLIP, state())                            # 4 region 2 overlaps region 1
    add(quad(30.25, 15.5, 80.5, 65.25), [0x9040C0FF, 0x90FF40C0, 0x50C0FF40, 0x90404040], QUAD, 1, 0, state(region=(second, 1), rule=1))  # 5 straddles region 2, Out
    add(quad(0.5, 8.25, 82.0, 60.5), 0xB0E0E000, QUAD, 0, 0, state(region=r1, rule=0))                          # 6 names region 1 AFTER region 2's clip mesh
    add([(60.5, 2.5), (81.5, 6.25), (66.25, 24.5)], 0xA000A0FF, [0, 1, 2], 0, 0, state(region=(first, 0), rule=0))   # 7 n == 0: untested
    add([(2.5, 50.5), (30.25, 56.5), (8.5, 70.25)], 0xA0FF00A0, [0, 2, 1], 0, 0, (BIG, 0, NONE, 5, 0))          # 8 f == NONE: untested
    add(quad(-10.0, -10.0, 100.0, 90.0), [0x70102030, 0x70F0E0D0, 0x70805020, 0x7020F080], QUAD, 1, 0, state(scissor=(20, 10, 40, 45)))  # 9 cut on all four sides by its own scissor
    fr = b.frame("clips", R.Target(93, 80, 100, -7, -5, scissor=(3, 2, 90, 77)))
    return with_draws(fr, list(range(len(ty))), ty, st)


def lattice_clip():
    """raster_model.lattice()'s meshes 0 and 1 as the clip meshes of an In region under one opaque rectangle over the whole image."""
    src = R.lattice()
    nv, ni = int(src.meshes["first_vertex"][2]), int(src.meshes["first_index"][2])
    b = R.Builder()
    b.pos, b.color, b.idx = [tuple(p) for p in src.pos[:nv]], [int(c) for c in src.color[:nv]], [int(i) for i in src.idx[:ni]]
    b.meshes = [tuple(int(src.meshes[k][m]) for k in src.meshes.dtype.names) for m in range(2)]
    b.mesh(quad(-5.0, -5.0, 100.0, 80.0), 0xFF3060C0, QUAD)
    fr = b.frame("lattice_clip", src.target)
    return with_draws(fr, [0, 1, 2], [CLIP, CLIP, 0], [state(), state(), state(region=(0, 2), rule=0)])


def stack_clip():
    """raster_model.stack()'s 300 translucent meshes twice on one tile (x, y in 16 .. 32): under an In region that is the tile's left
    half, then under an Out region that is the left half again -- an Out region's draws land where its clip meshes are NOT, so the
    second 300 land on the right half, and S on the left half is overwritten between the two runs. More than 256 meshes and more
    than 256 triangles per run: S must survive both batch boundaries."""
    src = R.stack()
    b = R.Builder()
    left = quad(16.0, 16.0, 24.0, 32.0)
    mesh_draw, ty, st = [], [], []

    def run(rule):
        clip = len(ty)
        b.mesh(left, 0xFF0000FF, QUAD)
        mesh_draw.append(clip); ty.append(CLIP); st.append(state())
        ty.append(0); st.append(state(region=(clip, 1), rule=rule))
        for m in range(src.nm):
            me = src.meshes[m]
            fv, fi, nvv, nii = int(me["first_vertex"]), int(me["first_index"]), int(me["num_vertices"]), int(me["num_indices"])
            b.mesh([tuple(p) for p in src.pos[fv:fv + nvv]], [int(c) for c in src.color[fv:fv + nvv]], [int(i) for i in src.idx[fi:fi + nii]],
                   kind=int(me["subpath_kind"]) >> 28)
            mesh_draw.append(clip + 1)
    run(0)
    run(1)
    fr = b.frame("stack_clip", src.target)
    return with_draws(fr, mesh_draw, ty, st)


class Rec(cu.Recorder):
    """cmdlist_util.Recorder and the state commands this frame needs."""

    def reset_scissor(self): self._cmd("ResetScissor")
    def intersect_scissor(self, *a): self._f("IntersectScissor", *a)
    def begin_clip(self, rule): self._cmd("BeginClip", struct.pack("<I", rule))
    def end_clip(self): self._cmd("EndClip")
    def reset_clip(self): self._cmd("ResetClip")


DECODED_CANVAS = (256, 192)


def decoded_bytes():
    """The s_scissor_clip script of tests/test_cmdlist_ref.py at 0.3 x, in a 256 x 192 window, with the clipped draws moved so that
    they straddle their regions."""
    AA, NOAA = cu.fill_flags(aa=True), cu.fill_flags(aa=False)
    r = Rec()

    def rect(x, y, w, h, color, flags):
        r.begin_path(); r.rect(x, y, w, h); r.fill_path(color, flags)

    def circle(x, y, rad, color, flags):
        r.begin_path(); r.circle(x, y, rad); r.fill_path(color, flags)

    rect(3, 3, 30, 30, 0xFF0000FF, AA)
    rect(6, 6, 30, 30, 0xC000FF00, AA)
    r.set_scissor(0, 0, 90, 60)
    rect(9, 9, 90, 60, 0xC0FF0000, AA)                       # cut by the 90 x 60 scissor
    r.push_state(); r.intersect_scissor(15, 15, 30, 30)
    circle(30, 30, 22, 0xE0FFFFFF, AA)                       # cut by the 30 x 30 scissor
    r.pop_state()
    circle(30, 30, 6, 0xFF808080, AA)
    r.reset_scissor()
    r.begin_clip(0)
    rect(60, 60, 90, 90, 0xFF123456, AA)
    r.begin_path(); r.move_to(63, 63); r.line_to(180, 70); r.line_to(120, 150); r.stroke_path(0x00123456, 8.0, cu.stroke_flags(1, 1, True))
    r.end_clip()
    rect(40, 75, 160, 40, 0xD00000FF, AA)                    # straddles the In region
    rect(100, 40, 40, 140, 0xA000C0FF, NOAA)
    r.reset_clip()
    rect(10, 120, 40, 40, 0xFF0060FF, AA)
    r.begin_clip(1)
    circle(200, 100, 30, 0xFFFFFFFF, NOAA)
    r.end_clip()
    r.set_scissor(150, 60, 90, 100)
    r.begin_path(); r.circle(206, 106, 34); r.stroke_path(0xFFFFFFFF, 14.0, cu.stroke_flags(0, 0, True))   # straddles the Out region
    rect(140, 70, 110, 50, 0x9020D040, AA)                   # and so does this, cut by the scissor on three sides
    return r.bytes()


def decoded(rt):
    """The decoded list tessellated by the CPU oracle. rt: the runtime module (vgx_cmdlist_decode runs on the host)."""
    extra = {}
    rc, ps, draws, n = cu.decode(rt, decoded_bytes(), canvas=(float(DECODED_CANVAS[0]), float(DECODED_CANVAS[1])), extra=extra)
    assert rc == capi.VGX_OK
    r = R.oracle.tessellate(ps, draws)
    w, h = DECODED_CANVAS
    fr = R.make("decoded", r.pos, r.color, r.idx, r.meshes, R.Target(w, h, w + 3, 0, 0))
    fr.draws, fr.dstate, fr.pathset = draws, extra["draw_state"], ps
    return fr


NAMES = ("clips", "lattice_clip", "stack_clip")
_MAKERS = {"clips": clips, "lattice_clip": lattice_clip, "stack_clip": stack_clip}
_decoded = {}


def frame(name, rt=None):
    if name == "decoded":
        if "f" not in _decoded:
            _decoded["f"] = decoded(rt)
        return _decoded["f"]
    return _frame(name)


@functools.lru_cache(maxsize=None)
def _frame(name):
    return _MAKERS[name]()


_images = {}


def expected(name, clear=False, rt=None):
    """The model's image of a frame over its target's background: computed once per session, never changed."""
    key = (name, bool(clear))
    if key not in _images:
        f = frame(name, rt)
        tgt = f.target.with_clear(0xFF102030) if clear else f.target
        img = render(f, tgt, tgt.background())
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


# ---- conditions: each frame does what it is for, decided on the model alone ------------------------------------------------
_checked = {}


def check_conditions(name, rt=None):
    if name in _checked:
        return True
    f = frame(name, rt)
    tgt = f.target
    st = Stats(tgt, f.nm)
    img = render(f, tgt, tgt.background(), stats=st)
    assert np.array_equal(img, expected(name, rt=rt))
    assert R.guards_intact(tgt, img)
    plain = render(f, tgt, tgt.background(), ignore_clips=True)
    if name == "clips":
        sx0, sy0, sx1, sy1 = tgt.scissor
        assert tgt.width % 16 and all(v % 16 for v in tgt.scissor) and tgt.stride > tgt.width and tgt.x0 < 0 and tgt.y0 < 0
        for m in (3, 5):                                                            # In and Out decide both ways
            assert st.accept[m] >= 20 and st.reject[m] >= 20, (m, st.accept[m], st.reject[m])
        # last writer wins: accepted where only region 1 stamped, rejected where region 2 overwrote S, rejected where nothing stamped
        assert st.accept[6] >= 20 and st.reject_over[6] >= 20 and st.reject_never[6] >= 20, (st.accept[6], st.reject_over[6], st.reject_never[6])
        assert int(f.dstate["clip_num_draws"][7]) == 0 and int(f.dstate["clip_first_draw"][7]) != NONE and st.untouched[7] >= 20
        assert int(f.dstate["clip_first_draw"][8]) == NONE and int(f.dstate["clip_num_draws"][8]) != 0 and st.untouched[8] >= 20
        assert st.accept[2] >= 20 and st.cut[2] >= 20                               # the clip mesh's own scissor is smaller than its geometry
        rx0, ry0, rx1, ry1 = draw_rect(tgt, f.dstate["scissor"][9])
        assert sx0 < rx0 and sy0 < ry0 and rx1 < sx1 and ry1 < sy1 and st.cut[9] >= 20
        hit = st.per_mesh[9] > 0
        assert hit[ry0:ry1, rx0].any() and hit[ry0:ry1, rx1 - 1].any() and hit[ry0, rx0:rx1].any() and hit[ry1 - 1, rx0:rx1].any()  # cut on all four sides
        assert not hit[:, :rx0].any() and not hit[:, rx1:].any() and not hit[:ry0].any() and not hit[ry1:].any()
        assert not np.array_equal(img, plain)
        assert not np.array_equal(img, render(f, tgt, tgt.background(), order_free=True))
        clip = [m for m in range(f.nm) if ((int(f.draws["state_key"][m]) >> 16) & 0xF) == CLIP]
        assert len(clip) == 3 and all(m not in st.per_mesh for m in clip)           # no colour from a clip mesh ...
        g = clips()
        for m in clip:
            me = f.meshes[m]
            sl = slice(int(me["first_vertex"]), int(me["first_vertex"]) + int(me["num_vertices"]))
            assert (f.color[sl] >> 24).min() > 0                                    # ... of non-zero alpha ...
            g.color[sl] = f.color[sl] ^ np.uint32(0x00FFFFFF)
        assert np.array_equal(render(g, tgt, tgt.background()), img)                # ... whatever its colours
    elif name == "lattice_clip":
        src = R.lattice()
        R.check_conditions("lattice")
        rs = R.Stats(src.target, per_mesh=True)
        R.render(src, src.target, src.target.background(), mesh_end=2, stats=rs)
        union = (rs.per_mesh[0] == 1) | (rs.per_mesh[1] == 1)
        assert max(rs.per_mesh[0].max(), rs.per_mesh[1].max()) == 1 and int(union.sum()) > 1000
        assert np.array_equal(st.blends > 0, union)                                 # a seam that drops a sample would show as a hole
        assert np.array_equal(img != tgt.background(), union)
    elif name == "stack_clip":
        assert f.nm == 602 and st.blends[16:32, 16:24].max() > 30 and st.blends[16:32, 24:32].max() > 30
        assert not st.blends[:, :16].any() and not st.blends[:16].any()
        rev = render(f, tgt, tgt.background(), order=[0] + list(range(300, 0, -1)) + [301] + list(range(601, 301, -1)))
        assert not np.array_equal(rev, img)                                         # the order matters
        assert not np.array_equal(img, plain)
    elif name == "decoded":
        types = (f.draws["state_key"] >> 16) & 0xF
        user = types != CLIP
        regions = {(int(a), int(b)) for a, b in zip(f.dstate["clip_first_draw"][user], f.dstate["clip_num_draws"][user]) if a != NONE and b != 0}
        assert len(regions) >= 2, regions
        assert len({tuple(int(v) for v in s) for s in f.dstate["scissor"]}) >= 3
        assert {0, 1} <= {int(x) for x in f.dstate["clip_rule"][user & (f.dstate["clip_num_draws"] != 0)]}
        assert int((img != plain).sum()) >= 100
        assert tgt.width <= 256 and tgt.height <= 192
    _checked[name] = True
    return True
