"""CPU: the lane code of vgx_raster_painted (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_painted, the host loop of the
frame-level calls at the painted level) against the numpy statement (tests/raster_painted_model.py), and against six things that do not rest on that
model: two closed forms of a gradient, a gradient of one colour against vgxt_raster_textured, a 1:1 pattern blit computed from div255
alone, a pattern against a sampled quad with the same map, and the frames without a painted draw. vgx_paint_tables is checked here too
(host only). Exact everywhere: np.array_equal on the uint32 images, the stride padding and everything outside the scissor included.
tests/test_gpu_raster_painted.py makes the same comparisons on the kernels, with the same `check_*` functions of tests/raster_harness.py run through the device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import raster_harness as H
import raster_model as R
import raster_painted_model as P
import raster_textured_model as T
from raster_harness import draws_struct, host, image_records, rt  # noqa: F401 (host, rt: fixtures)

capi = R.capi
CLEAR = P.CLEAR
F = np.float32
BAD = capi.VGX_E_INVALID_ARG


@pytest.fixture(scope="module")
def run(host):
    return H.HostRunner(host)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", P.NAMES)
def test_lane_code_equals_model(host, rt, name, clear):
    P.check_conditions(name, rt)
    f = P.frame(name, rt)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = P.expected(name, clear, rt)
    got = H.host_level(host, "painted", f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
    assert R.guards_intact(tgt, got)
    assert np.array_equal(H.host_level(host, "painted", f, tgt, with_bounds=True), got)  # the boxes handed in: the same bytes


def test_the_paint_shows(host, rt):
    """What the call is for: vgxt_raster_textured draws these frames black or in their flat tint."""
    for name in ("linear", "pattern_linear_repeat", "decoded"):
        f = P.frame(name, rt)
        assert not np.array_equal(H.host_level(host, "textured", f, f.target), P.expected(name, rt=rt))


# ---- checks that do not rest on the model (tests/raster_harness.py): the GPU test hands in a runner over the kernels ------------------
def test_linear_ramp_closed_form(run, rt):
    H.check_linear_ramp(run, rt)


def test_radial_distances_closed_form(run, rt):
    H.check_radial_distances(run, rt)


def test_one_colour_gradient_equals_textured(run, rt):
    H.check_one_colour_gradient(run, rt)


def test_pattern_blit_from_div255(run):
    H.check_pattern_blit(run)


def test_pattern_equals_sampled_quad(run):
    H.check_pattern_equals_sampled_quad(run)


@pytest.mark.parametrize("name", T.NAMES)
def test_no_painted_draw_equals_textured(run, name):
    H.check_no_painted_draw(run, name)


# ---- the pieces ---------------------------------------------------------------------------------------------------------
def test_q8_and_gradient_t_pieces(host):
    for c in (0.0, 1.0, -0.5, 1.5, 0.5, 0.25, 1e30, -1e30, np.nan, np.inf, -np.inf, 0.999, 1.001, -1e-3, 1e-3):
        assert host.vgxt_raster_q8(C.c_float(c)) == P.q8(F(c)), c
    for k in range(256):
        assert host.vgxt_raster_q8(C.c_float(float(F(k) / F(255.0)))) == k   # the decoder's c / 255.0f gives c back
    rs = np.random.RandomState(5)
    for _ in range(400):
        params = rs.uniform(-3, 40, 4).astype(F)
        if rs.rand() < 0.2:
            params[rs.randint(4)] = rs.choice([0.0, np.nan, np.inf, -np.inf])
        qx, qy = rs.uniform(-60, 60, 2)
        if rs.rand() < 0.1:
            qx = rs.choice([np.nan, np.inf, -np.inf])
        p = np.zeros(1, dtype=capi.paint_dtype)[0]
        p["params"] = params
        with np.errstate(all="ignore"):
            want, _ = P.gradient_t(p, np.float64(qx), np.float64(qy))
        got = host.vgxt_raster_gradient_t(params.ctypes.data, qx, qy)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (params, qx, qy)


def test_host_sqrt_is_correctly_rounded(host):
    """x86-64's sqrtsd against integer arithmetic: r = sqrt(x) is correctly rounded iff (r - u/2)^2 < x < (r + u/2)^2 (ties cannot occur)."""
    rs = np.random.RandomState(6)
    xs = list(rs.uniform(0, 1e6, 200)) + [float(a * a + b * b) for a, b in rs.uniform(0, 300, (200, 2)).astype(F).astype(float)] + [4.0, 2.0, 1e-300, 1e300]
    for x in xs:
        r = host.vgxt_raster_sqrt(x)
        X, Rr = Fraction(x), Fraction(r)
        lo, hi = Fraction(np.nextafter(r, 0.0)), Fraction(np.nextafter(r, np.inf))
        assert ((Rr + lo) / 2) ** 2 <= X <= ((Rr + hi) / 2) ** 2, x


# ---- protocol ---------------------------------------------------------------------------------------------------------------
def test_invalid_paint_writes_nothing(host):
    f = P.frame("state")
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for what, kw in H.invalid_cases(f):
            got = H.host_level(host, "painted", f, tgt, want=BAD, **kw)
            assert np.array_equal(got, tgt.background()), what
    assert P.status(f, gradients=f.gradients[:1]) == BAD and P.status(f, patterns=f.patterns[:0]) == BAD
    # entries no painted mesh of the range names may be garbage: meshes 0 .. 3 name gradient 1 alone
    junk_g = f.gradients.copy()
    junk_g[0] = np.frombuffer(bytes(range(96)), dtype=capi.paint_dtype)[0]
    junk_p = np.frombuffer(bytes(range(7, 103)), dtype=capi.paint_dtype).copy()
    got = H.host_level(host, "painted", f, f.target, gradients=junk_g, patterns=junk_p, end=4)
    assert np.array_equal(got, P.render(f, f.target, f.target.background(), mesh_end=4))
    assert not np.array_equal(got, f.target.background())
    # a path-kind mesh of a type-0 draw with a handle outside every table is no painted mesh
    g = P.state_frame()
    g.draws["state_key"][0] |= 0xFFFF
    assert np.array_equal(H.host_level(host, "painted", g, g.target), P.expected("state"))


def test_mesh_range_and_split_calls(host):
    f = P.frame("crowd")
    img = H.host_level(host, "painted", f, f.target, end=150)
    assert np.array_equal(img, P.render(f, f.target, f.target.background(), mesh_end=150))
    img = H.host_level(host, "painted", f, f.target, image=img, begin=150)
    assert np.array_equal(img, P.expected("crowd"))


def test_host_argument_checks(host):
    f = P.frame("state")
    img = f.target.background()
    d, s = f.desc(), draws_struct(f)
    rec = image_records(f.images)
    x = capi.RasterTextures(f.uv.ctypes.data, rec.ctypes.data, 8, 1)
    gp, pp = f.gradients.ctypes.data, f.patterns.ctypes.data

    def call(paints):
        t = f.target.struct(img.ctypes.data)
        return host.vgxt_raster_painted(C.byref(d), None, 0, f.nm, C.byref(s), C.byref(x), None if paints is None else C.byref(paints), C.byref(t), None)

    assert call(None) == BAD
    assert call(capi.RasterPaints(None, pp, 2, 1)) == BAD and call(capi.RasterPaints(gp, None, 2, 1)) == BAD
    assert call(capi.RasterPaints(gp + 2, pp, 2, 1)) == BAD and call(capi.RasterPaints(gp, pp + 1, 2, 1)) == BAD
    assert np.array_equal(img, f.target.background())  # none of them wrote
    assert call(capi.RasterPaints(gp, pp, 2, 1)) == capi.VGX_OK
    assert np.array_equal(img, P.expected("state"))


# ---- vgx_paint_tables (host only) -----------------------------------------------------------------------------------------------
def test_paint_tables_scatter(rt):
    f = P.frame("decoded", rt)
    g, p = rt.paint_tables(f.paints)
    assert g.tobytes() == f.gradients.tobytes() and p.tobytes() == f.patterns.tobytes()   # the model's scatter
    assert g["handle"].tolist() == [0, 1, 2] and p["handle"].tolist() == [0, 1]
    # holes marked, capacity beyond the records, a later record with the same handle wins
    recs = np.zeros(4, dtype=capi.paint_dtype)
    recs["type"] = [1, 2, 1, 1]
    recs["handle"] = [3, 1, 0, 3]
    recs["image"] = [10, 11, 12, 13]
    g, p = rt.paint_tables(recs, num_gradients=6, num_patterns=2)
    assert g["type"].tolist() == [1, P.UNUSED, P.UNUSED, 1, P.UNUSED, P.UNUSED] and p["type"].tolist() == [P.UNUSED, 2]
    assert int(g["image"][3]) == 13 and int(g["image"][0]) == 12 and int(p["image"][1]) == 11
    assert g[1].tobytes() == P.table([None])[0].tobytes()                                  # a hole is zeros behind its type
    g, p = rt.paint_tables(recs[:0])
    assert g.shape[0] == 0 and p.shape[0] == 0


def test_paint_tables_refusals(rt):
    lib = rt.lib()
    recs = np.zeros(2, dtype=capi.paint_dtype)
    recs["type"] = [1, 2]
    recs["handle"] = [2, 0]
    g, p = np.zeros(4, dtype=capi.paint_dtype), np.zeros(4, dtype=capi.paint_dtype)

    def call(n, cg, cp, r=recs, gg=g, pp=p):
        return lib.vgx_paint_tables(r.ctypes.data if r is not None else None, n, gg.ctypes.data if gg is not None else None, cg,
                                    pp.ctypes.data if pp is not None else None, cp)

    assert call(2, 3, 1) == capi.VGX_OK
    assert call(2, 2, 1) == capi.VGX_E_NOSPACE and call(2, 3, 0) == capi.VGX_E_NOSPACE
    for t in (0, 3, P.UNUSED):
        bad = recs.copy()
        bad["type"][1] = t
        assert call(2, 3, 1, r=bad) == BAD
    assert call(2, 3, 1, r=None) == BAD and call(2, 3, 1, gg=None) == BAD and call(2, 3, 1, pp=None) == BAD
    assert call(0, 0, 0, r=None, gg=None, pp=None) == capi.VGX_OK


def test_struct_sizes():
    assert C.sizeof(capi.RasterPaints) == 24 and capi.paint_dtype.itemsize == 96
    assert capi.paint_dtype.fields["matrix"][1] == 8 and capi.paint_dtype.fields["params"][1] == 44 and capi.paint_dtype.fields["image"][1] == 92
