"""CPU: the lane code of vgx_raster_concave (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_concave, the host loop of the
frame-level calls at the concave level) against the numpy statement (tests/raster_concave_model.py), and against things that do not
rest on that model: the winding predicate in exact rational arithmetic, a triangle drawn as three edges against the same triangle
through vgx_raster_painted's lane code, a convex polygon against its fan, and -- with the libtess2 linked into oracle/_ref/libvgref.so --
concave polygons against the image of libtess2's triangulation. Exact everywhere: np.array_equal on the uint32 images, the stride
padding and everything outside the scissor included. tests/test_gpu_raster_concave.py makes the same comparisons on the kernels, with
the same `check_*` functions of tests/raster_harness.py run through the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import raster_concave_model as K
import raster_harness as H
import raster_model as R
import test_gpu_concave as TC
from raster_harness import host  # noqa: F401 (fixture)

capi = R.capi
CLEAR = K.CLEAR
F = np.float32


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


@pytest.fixture(scope="module")
def run(host):
    return H.HostRunner(host)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", K.NAMES)
def test_lane_code_equals_model(run, name, clear):
    K.check_conditions(name)
    f = K.frame(name)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = K.expected(name, clear)
    got = run.concave(f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
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
            want = H.exact_winding(u, v, px, py)
            assert host.vgxt_raster_winding(u.ctypes.data, v.ctypes.data, n, px, py) == want, (trial, px, py)
            seen["nonzero"] += want != 0
            seen["vertex"] += any(float(p[0]) == px and float(p[1]) == py for p in pts)
            seen["on_edge"] += any((Fraction(float(b[0])) - Fraction(float(a[0]))) * (Fraction(py) - Fraction(float(a[1])))
                                   == (Fraction(float(b[1])) - Fraction(float(a[1]))) * (Fraction(px) - Fraction(float(a[0]))) for a, b in zip(u, v))
    assert seen["vertex"] > 100 and seen["nonzero"] > 1000 and seen["on_edge"] > 1000, seen


# ---- checks that do not rest on the model (tests/raster_harness.py): the GPU tests hand in a runner over the kernels ----------------
def test_triangle_twin(run):
    H.check_triangle_twin(run)


def test_convex_polygon_equals_fan(run):
    H.check_convex_fan(run)


def test_simple_concave_polygons_equal_libtess2(run, ref):
    H.check_simple_concave(run, ref)


def test_crossing_fixtures_equal_libtess2_away_from_rounded_vertices(run, ref):
    """Excluded / covered samples per fixture, recorded in EXCLUDED and printed. With these coordinates: the two overlapping squares (equal
    and opposite orientation) and the bow-tie cross at integer points libtess2 represents exactly, 0 excluded under both rules; the
    pentagram's five crossings are not representable, 20 of 3496 covered samples excluded under NonZero and 20 of 2420 under EvenOdd
    (0.57 % and 0.83 %), which is why it is drawn this large."""
    H.check_crossing(run, ref)
    print(H.EXCLUDED)


def test_levels(run):
    H.check_levels(run)


def test_older_host_loops_skip_contour_meshes(host):
    """vgxt_raster, vgxt_raster_frame and vgxt_raster_textured too; vgxt_pick never reports a contour mesh."""
    f = K.frame("state")
    g = K.without_contours(f)
    assert np.array_equal(H.host_level(host, "raster", f, f.target), H.host_level(host, "raster", g, g.target))
    assert np.array_equal(H.host_level(host, "frame", f, f.target), H.host_level(host, "frame", g, g.target))
    assert np.array_equal(H.host_level(host, "textured", f, f.target), H.host_level(host, "textured", g, g.target))
    h = K.frame("centres")  # contour meshes only
    q = np.zeros(3, dtype=capi.pick_query_dtype)
    q["x"], q["y"], q["mesh_end"] = [8.0, 6.0, 28.0], [8.0, 18.0, 22.0], 0xFFFFFFFF
    hits = np.zeros(3, dtype=capi.pick_hit_dtype)
    d = h.desc()
    assert host.vgxt_pick(C.byref(d), None, q.ctypes.data, 3, hits.ctypes.data) == capi.VGX_OK
    assert (hits["mesh"] == 0xFFFFFFFF).all()
