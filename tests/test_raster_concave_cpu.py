"""CPU: the lane code of vgx_raster_concave (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_concave, the host loop of the
frame-level calls at the concave level) against the numpy statement (tests/raster_concave_model.py), and against things that do not
rest on that model: the winding predicate in exact rational arithmetic, a triangle drawn as three edges against the same triangle
through vgx_raster_painted's lane code, a convex polygon against its fan, and -- with the libtess2 linked into oracle/_ref/libvgref.so --
concave polygons against the image of libtess2's triangulation. Exact everywhere: np.array_equal on the uint32 images, the stride
padding and everything outside the scissor included. tests/test_gpu_raster_concave.py makes the same comparisons on the kernels, with
the `check_*` functions of this file run through the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import concave_frame as CF
import raster_concave_model as K
import raster_frame_model as M
import raster_model as R
import raster_painted_model as P
import test_gpu_concave as TC
import test_raster_cpu as base
import test_raster_frame_cpu as fcpu
import test_raster_painted_cpu as pcpu
import test_raster_textured_cpu as tcpu

capi = R.capi
CLEAR = K.CLEAR
F = np.float32
LEVEL_ARGS = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(capi.RasterDraws), C.POINTER(capi.RasterTextures),
              C.POINTER(capi.RasterPaints), C.POINTER(capi.RasterTarget), C.c_void_p]


def load_host():
    lib = pcpu.load_host()
    if not hasattr(lib, "vgxt_raster_concave"):  # a library from before this call: build again
        import __graft_entry__ as g
        g.build()
        lib = pcpu.load_host()
    lib.vgxt_raster_concave.restype = C.c_int
    lib.vgxt_raster_concave.argtypes = LEVEL_ARGS
    lib.vgxt_raster_winding.restype = C.c_int32
    lib.vgxt_raster_winding.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


def host_level(host, fn, f, tgt, image=None, with_bounds=False, begin=0, end=2**64 - 1, want=capi.VGX_OK):
    """One of the two widest host loops (vgxt_raster_painted, vgxt_raster_concave) over the target's background; returns the image."""
    img = tgt.background() if image is None else image
    rec = tcpu.image_records(f.images)
    g, p = np.ascontiguousarray(f.gradients), np.ascontiguousarray(f.patterns)
    mb = base.host_bounds(host, f) if with_bounds else None
    d, s, t = f.desc(), fcpu.draws_struct(f), tgt.struct(img.ctypes.data)
    x = capi.RasterTextures(f.uv.ctypes.data, rec.ctypes.data if len(f.images) else None, 8 if f.uv.dtype == np.float32 else 4, len(f.images))
    pt = pcpu.paints_struct(g, p)
    status = np.full(1, 77, dtype=np.uint32)
    assert getattr(host, fn)(C.byref(d), None if mb is None else mb.ctypes.data, begin, end, C.byref(s), C.byref(x), C.byref(pt), C.byref(t),
                             status.ctypes.data) == capi.VGX_OK
    assert status[0] == want
    return img


class HostRunner:
    """What the model-independent checks call: the new level and the painted level on the same kind of inputs."""

    def __init__(self, host):
        self.host = host

    def concave(self, f, tgt, **kw):
        return host_level(self.host, "vgxt_raster_concave", f, tgt, **kw)

    def painted(self, f, tgt, **kw):
        return host_level(self.host, "vgxt_raster_painted", f, tgt, **kw)


@pytest.fixture(scope="module")
def run(host):
    return HostRunner(host)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", K.NAMES)
def test_lane_code_equals_model(run, name, clear):
    K.check_conditions(name)
    f = K.frame(name)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = K.expected(name, clear)
    got = run.concave(f, tgt)
    assert np.array_equal(got, want), base.where(got, want)
    assert R.guards_intact(tgt, got)
    assert np.array_equal(run.concave(f, tgt, with_bounds=True), got)  # the boxes handed in: the same bytes


def test_mesh_range_and_status(run):
    f = K.frame("state")
    for begin, end in ((0, 3), (2, 5), (3, 99)):
        want = K.render(f, f.target, f.target.background(), begin, end)
        assert np.array_equal(run.concave(f, f.target, begin=begin, end=end), want)
    g = K.state_frame()
    g.meshes["draw"][4] = 99  # a contour mesh outside the draw table: nothing is written
    assert np.array_equal(run.concave(g, g.target.with_clear(CLEAR), want=capi.VGX_E_INVALID_ARG), g.target.background())


# ---- checks that do not rest on the model: shared with the GPU tests, which hand in a runner over the kernels --------------------
def exact_winding(u, v, px, py):
    """W of the header's rule in rational arithmetic: exact signs, no canonical form needed."""
    W = 0
    px, py = Fraction(px), Fraction(py)
    for a, b in zip(u, v):
        ax, ay, bx, by = (Fraction(float(c)) for c in (a[0], a[1], b[0], b[1]))
        E = (bx - ax) * (py - ay) - (by - ay) * (px - ax)  # the value of u -> v: positive on one side, whichever endpoint is `lo`
        if ay < py <= by and E < 0:
            W += 1
        elif by < py <= ay and E > 0:
            W -= 1
    return W


def test_winding_equals_exact_arithmetic(host):
    """Random edge soups on a half-pixel grid and off it; the samples include every vertex and points on edges."""
    rs = np.random.RandomState(5)
    seen = {"vertex": 0, "nonzero": 0, "on_edge": 0}
    for trial in range(20):
        n = int(rs.randint(3, 9))
        pts = (rs.randint(0, 24, (n, 2)) / 2.0 + (0 if trial % 2 else rs.uniform(-0.2, 0.2, (n, 2)))).astype(F)
        u, v = pts, np.roll(pts, -1, axis=0)
        if trial % 5 == 0:
            v = v[rs.permutation(n)]  # an open soup
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        samples = [(x / 2.0, y / 2.0) for x in range(0, 26, 1) for y in range(0, 26, 1)] + [(float(p[0]), float(p[1])) for p in pts]
        samples += [((float(a[0]) + float(b[0])) / 2, (float(a[1]) + float(b[1])) / 2) for a, b in zip(u, v)]
        for px, py in samples:
            want = exact_winding(u, v, px, py)
            assert host.vgxt_raster_winding(u.ctypes.data, v.ctypes.data, n, px, py) == want, (trial, px, py)
            seen["nonzero"] += want != 0
            seen["vertex"] += any(float(p[0]) == px and float(p[1]) == py for p in pts)
            seen["on_edge"] += any((Fraction(float(b[0])) - Fraction(float(a[0]))) * (Fraction(py) - Fraction(float(a[1])))
                                   == (Fraction(float(b[1])) - Fraction(float(a[1]))) * (Fraction(px) - Fraction(float(a[0]))) for a, b in zip(u, v))
    assert seen["vertex"] > 100 and seen["nonzero"] > 1000 and seen["on_edge"] > 1000, seen


def edges_frame(name, polys, tgt, colors, even_odd=False, as_triangles=None):
    """One mesh per polygon under one colour draw: contour rings, or (as_triangles: a function polygon -> index triples) triangles."""
    b = K.Builder()
    for poly, c in zip(polys, colors):
        if as_triangles is None:
            b.contours([poly], c, even_odd=even_odd)
        else:
            b.mesh([tuple(p) for p in poly], c, as_triangles(poly))
    return K.finish(b.frame(name, tgt))


def check_triangle_twin(run):
    """Random triangles on a half-pixel grid (ties are common), alpha 128: three edges through the new level equal the triangle through
    vgx_raster_painted at every pixel, under either rule."""
    rs = np.random.RandomState(9)
    tgt = R.Target(40, 40, 41, -3, -2)
    tris = [rs.randint(-8, 80, (3, 2)) / 2.0 for _ in range(60)]
    tris = [t.astype(F) for t in tris if R.orientation(*t.astype(F)) != 0]
    cols = [0x80000000 | int(rs.randint(0, 1 << 24)) for _ in tris]
    want = run.painted(edges_frame("twin", tris, tgt, cols, as_triangles=lambda p: [0, 1, 2]), tgt)
    assert int((want != tgt.background()).sum()) > 800
    for eo in (False, True):
        got = run.concave(edges_frame("twin", tris, tgt, cols, even_odd=eo), tgt)
        assert np.array_equal(got, want), base.where(got, want)


def check_convex_fan(run):
    """A convex polygon equals the fan strokerConvexFill makes of it (0, i, i + 1)."""
    tgt = R.Target(48, 40, 48, 0, 0)
    polys = [TC._ring(14.3, 12.7, 11.2, 9), TC._ring(33.5, 26.5, 12.5, 14, cw=True), np.array(M.quad(2.5, 28.5, 20.5, 37.5), dtype=F)]
    cols = [0xC02060F0, 0x8030F060, 0xA0F0F020]
    fan = lambda p: [k for i in range(1, len(p) - 1) for k in (0, i, i + 1)]
    want = run.painted(edges_frame("fan", polys, tgt, cols, as_triangles=fan), tgt)
    got = run.concave(edges_frame("fan", polys, tgt, cols), tgt)
    assert np.array_equal(got, want), base.where(got, want)


SIMPLE = {
    "L": [[(3, 2), (30, 2), (30, 12), (14, 12), (14, 33), (3, 33)]],
    "comb": [[(2, 2), (38, 2), (38, 30), (32, 30), (32, 9), (26, 9), (26, 30), (20, 30), (20, 9), (14, 9), (14, 30), (8, 30), (8, 9), (2, 9)]],
    "ring": [[(4, 4), (36, 4), (36, 34), (4, 34)], [(12, 10), (12, 26), (28, 26), (28, 10)]],   # the hole: the opposite orientation
}


def tess_frame(ref, name, contours, tgt, color, even_odd):
    verts, idx = CF._polygons(ref, [np.array(c, dtype=F) for c in contours], 1 if even_odd else 0)
    b = K.Builder()
    b.mesh([tuple(p) for p in verts], color, [int(i) for i in idx])
    return K.finish(b.frame(name, tgt)), verts


def check_simple_concave(run, ref):
    """Simple concave polygons on an integer grid: the edge mesh equals the image of libtess2's TESS_POLYGONS triangulation."""
    tgt = R.Target(42, 38, 43, -1, -1)
    for name, contours in SIMPLE.items():
        for eo in (False, True):
            tf, _ = tess_frame(ref, name, contours, tgt, 0x90E04080, eo)
            want = run.painted(tf, tgt)
            b = K.Builder()
            b.contours([np.array(c, dtype=F) for c in contours], 0x90E04080, even_odd=eo)
            got = run.concave(K.finish(b.frame(name, tgt)), tgt)
            assert int((want != tgt.background()).sum()) > 300
            assert np.array_equal(got, want), (name, eo, base.where(got, want))


PENT = [(58.0 + 56.0 * np.cos(1.2566370614 * k - 1.5707963), 58.0 + 56.0 * np.sin(1.2566370614 * k - 1.5707963)) for k in (0, 2, 4, 1, 3)]   # large: its five crossings are not representable
CROSSING = {
    "squares_same": [[(4, 4), (24, 4), (24, 24), (4, 24)], [(14, 12), (36, 12), (36, 34), (14, 34)]],
    "squares_opposite": [[(4, 4), (24, 4), (24, 24), (4, 24)], [(14, 12), (14, 34), (36, 34), (36, 12)]],
    "pentagram": [PENT],
    "bowtie": [[(4, 6), (34, 30), (34, 6), (4, 30)]],   # crosses at (19, 18)
}
EXCLUDED = {}  # (fixture, even_odd) -> (excluded, covered), recorded by check_crossing


def exact_intersections(contours):
    """Every proper crossing of two edges of the contours, as exact rationals."""
    segs = []
    for c in contours:
        c = [(Fraction(float(F(x))), Fraction(float(F(y)))) for x, y in c]
        segs += [(c[k], c[(k + 1) % len(c)]) for k in range(len(c))]
    out = []
    for i in range(len(segs)):
        for j in range(i + 1, len(segs)):
            (p, q), (r, s) = segs[i], segs[j]
            d = (q[0] - p[0]) * (s[1] - r[1]) - (q[1] - p[1]) * (s[0] - r[0])
            if d == 0:
                continue
            t = ((r[0] - p[0]) * (s[1] - r[1]) - (r[1] - p[1]) * (s[0] - r[0])) / d
            w = ((r[0] - p[0]) * (q[1] - p[1]) - (r[1] - p[1]) * (q[0] - p[0])) / d
            if 0 < t < 1 and 0 < w < 1:
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def check_crossing(run, ref):
    """Overlapping and self-intersecting fixtures under both rules. libtess2 rounds the intersection vertices it creates, so samples
    within one pixel of an intersection vertex that is not bit-equal to the exact intersection are left out; they may be at most 1 %
    of the covered ones."""
    tgt = R.Target(118, 116, 118, 0, 0)
    j, i = np.mgrid[0:tgt.rows(), 0:tgt.stride]
    for name, contours in CROSSING.items():
        for eo in (False, True):
            tf, verts = tess_frame(ref, name, contours, tgt, 0xFF40A0E0, eo)
            want = run.painted(tf, tgt)
            b = K.Builder()
            b.contours([np.array(c, dtype=F) for c in contours], 0xFF40A0E0, even_odd=eo)
            got = run.concave(K.finish(b.frame(name, tgt)), tgt)
            mask = np.zeros(want.shape, dtype=bool)
            for x, y in exact_intersections(contours):
                near = [v for v in verts if abs(float(v[0]) - float(x)) < 0.01 and abs(float(v[1]) - float(y)) < 0.01]
                if not any(Fraction(float(v[0])) == x and Fraction(float(v[1])) == y for v in near):
                    mask |= (np.abs(i + 0.5 - float(x)) <= 1.0) & (np.abs(j + 0.5 - float(y)) <= 1.0)
            cov = int((got != tgt.background()).sum())
            EXCLUDED[(name, eo)] = (int(mask.sum()), cov)
            assert cov > 150 and mask.sum() * 100 <= cov, (name, eo, int(mask.sum()), cov)
            assert np.array_equal(got[~mask], want[~mask]), (name, eo, base.where(np.where(mask, 0, got), np.where(mask, 0, want)))


def check_levels(run):
    """A frame without contour meshes gives vgx_raster_painted's bytes; the painted level draws a frame WITH them as the frame with
    those meshes removed."""
    for name in ("state", "crowd"):
        f = P.frame(name)
        assert np.array_equal(run.concave(f, f.target), P.expected(name))
    for name in ("state", "classes", "odd"):
        f = K.frame(name)
        want = P.render(K.without_contours(f), f.target, f.target.background())
        got = run.painted(f, f.target)
        assert np.array_equal(got, want), (name, base.where(got, want))
        assert not np.array_equal(got, K.expected(name))


def test_triangle_twin(run):
    check_triangle_twin(run)


def test_convex_polygon_equals_fan(run):
    check_convex_fan(run)


def test_simple_concave_polygons_equal_libtess2(run, ref):
    check_simple_concave(run, ref)


def test_crossing_fixtures_equal_libtess2_away_from_rounded_vertices(run, ref):
    """Excluded / covered samples per fixture, recorded in EXCLUDED and printed. With these coordinates: the two overlapping squares (equal
    and opposite orientation) and the bow-tie cross at integer points libtess2 represents exactly, 0 excluded under both rules; the
    pentagram's five crossings are not representable, 20 of 3496 covered samples excluded under NonZero and 20 of 2420 under EvenOdd
    (0.57 % and 0.83 %), which is why it is drawn this large."""
    check_crossing(run, ref)
    print(EXCLUDED)


def test_levels(run):
    check_levels(run)


def test_older_host_loops_skip_contour_meshes(host):
    """vgxt_raster, vgxt_raster_frame and vgxt_raster_textured too; vgxt_pick never reports a contour mesh."""
    f = K.frame("state")
    g = K.without_contours(f)
    assert np.array_equal(base.host_render(host, f, f.target), base.host_render(host, g, g.target))
    assert np.array_equal(fcpu.host_frame(host, f, f.target), fcpu.host_frame(host, g, g.target))
    assert np.array_equal(tcpu.host_textured(host, f, f.target), tcpu.host_textured(host, g, g.target))
    import test_pick_cpu as pick
    lib = pick.load_host() if hasattr(pick, "load_host") else host
    h = K.frame("centres")  # contour meshes only
    q = np.zeros(3, dtype=capi.pick_query_dtype)
    q["x"], q["y"], q["mesh_end"] = [8.0, 6.0, 28.0], [8.0, 18.0, 22.0], 0xFFFFFFFF
    hits = np.zeros(3, dtype=capi.pick_hit_dtype)
    d = h.desc()
    lib.vgxt_pick.restype = C.c_int
    lib.vgxt_pick.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.vgxt_pick(C.byref(d), None, q.ctypes.data, 3, hits.ctypes.data) == capi.VGX_OK
    assert (hits["mesh"] == 0xFFFFFFFF).all()
