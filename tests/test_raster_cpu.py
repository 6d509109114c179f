"""CPU: the lane code of vgx_raster (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster, a plain loop over meshes, triangles
and the pixels of each triangle's box) against the numpy statement of the specification (tests/raster_model.py), and the coverage
predicate against exact rational arithmetic. Exact everywhere: np.array_equal on the uint32 images, the stride padding and everything
outside the scissor included. The GPU suite (tests/test_gpu_raster.py) makes the same comparison on the kernels."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import raster_harness as H
import raster_model as R
from raster_harness import host  # noqa: F401 (fixture)

capi = R.capi
F = np.float32
D = np.float64


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", R.NAMES)
def test_lane_code_equals_model(host, name, clear):
    R.check_conditions(name)
    f = R.frame(name)
    tgt = f.target.with_clear(0xFF102030) if clear else f.target
    want = R.expected(name, clear)
    got = H.host_level(host, "raster", f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
    assert R.guards_intact(tgt, got)
    assert not np.array_equal(got, tgt.background())
    # with the boxes handed in instead of computed by the call: the same bytes
    assert np.array_equal(H.host_level(host, "raster", f, tgt, with_bounds=True), got)


@pytest.mark.parametrize("name", R.NAMES)
def test_split_mesh_ranges(host, name):
    """[0, k) then [k, n) without CLEAR equals [0, n); so does mesh by mesh."""
    f = R.frame(name)
    want = R.expected(name)
    for k in sorted({0, 1, f.nm // 2, f.nm - 1, f.nm}):
        img = H.host_level(host, "raster", f, f.target, end=k)
        H.host_level(host, "raster", f, f.target, image=img, begin=k)
        assert np.array_equal(img, want), k
    if f.nm <= 300:
        img = f.target.background()
        for m in range(f.nm):
            H.host_level(host, "raster", f, f.target, image=img, begin=m, end=m + 1, with_bounds=bool(m % 2))
        assert np.array_equal(img, want)
    # an empty range writes nothing, or only the clear
    img = H.host_level(host, "raster", f, f.target, begin=f.nm)
    assert np.array_equal(img, f.target.background())
    tc = f.target.with_clear(0x01020304)
    img = H.host_level(host, "raster", f, tc, begin=3, end=3)
    sx0, sy0, sx1, sy1 = tc.scissor
    assert np.all(img[sy0:sy1, sx0:sx1] == 0x01020304) and R.guards_intact(tc, img)


def fr(v):
    return Fraction(float(v))


def exact_cover(a, b, c, px, py):
    """The rule of include/vgx.h over the rationals: every binary32 value and every sample is a rational number, nothing rounds.
    The canonical edge value is, as a real number, s * ((v - u) x (p - u)) whichever endpoint is lo."""
    (ax, ay), (bx, by), (cx, cy) = [(fr(p[0]), fr(p[1])) for p in (a, b, c)]
    px, py = Fraction(px), Fraction(py)
    if not (min(ax, bx, cx) <= px <= max(ax, bx, cx) and min(ay, by, cy) <= py <= max(ay, by, cy)):
        return False
    A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    if A == 0:
        return False
    s = 1 if A > 0 else -1
    total = 0
    for (ux, uy), (vx, vy) in (((ax, ay), (bx, by)), ((bx, by), (cx, cy)), ((cx, cy), (ax, ay))):
        E = s * ((vx - ux) * (py - uy) - (vy - uy) * (px - ux))
        dx, dy = s * (vx - ux), s * (vy - uy)
        if not (E > 0 or (E == 0 and (dy > 0 or (dy == 0 and dx < 0)))):
            return False
        total += E
    return total > 0


def products_exact(a, b, c, px, py):
    """The regime of the header: every difference the rule takes is exact in binary64 and so is every product of two of them."""
    def ok(p, q, r, s):  # (p - q) * (r - s)
        d1, d2 = D(p) - D(q), D(r) - D(s)
        return Fraction(float(d1)) == Fraction(float(p)) - Fraction(float(q)) and Fraction(float(d2)) == Fraction(float(r)) - Fraction(float(s)) \
            and Fraction(float(d1 * d2)) == Fraction(float(d1)) * Fraction(float(d2))
    good = ok(b[0], a[0], c[1], a[1]) and ok(b[1], a[1], c[0], a[0])
    for u, v in ((a, b), (b, c), (c, a)):
        lo, hi = (u, v) if (u[0] < v[0] or (u[0] == v[0] and u[1] <= v[1])) else (v, u)
        good = good and ok(hi[0], lo[0], py, lo[1]) and ok(hi[1], lo[1], px, lo[0])
    return good


def test_predicate_has_the_exact_sign(host):
    """The claim of include/vgx.h, checked and not assumed: on the Tiger frame's own triangles and the pixel centres of their boxes,
    wherever every difference and product is exact, model and lane code give the answer exact rational arithmetic gives; and that is
    the regime nearly all of these pairs are in (a condition on the inputs: the frame's scale was chosen for it)."""
    f = R.frame("tiger")
    tgt = f.target
    T = R.PM.triangles(f.pos, f.color, f.idx, f.meshes)
    rs = np.random.RandomState(4)
    pairs = []
    for g in rs.permutation(np.nonzero(T.valid)[0]):
        a, b, c = T.a[g], T.b[g], T.c[g]
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        xs = np.arange(np.ceil(lo[0] - 0.5), np.floor(hi[0] - 0.5) + 1) + 0.5
        ys = np.arange(np.ceil(lo[1] - 0.5), np.floor(hi[1] - 0.5) + 1) + 0.5
        cen = [(x, y) for y in ys for x in xs]
        for k in rs.permutation(len(cen))[:8]:
            pairs.append((g, cen[k][0], cen[k][1]))
        if len(pairs) >= 3000:
            break
    assert len(pairs) >= 3000
    regime, wrong, covered = 0, [], 0
    for g, x, y in pairs:
        a, b, c = T.a[g], T.b[g], T.c[g]
        got = R.cover(a, b, c, np.array([x]), np.array([y]))
        model = bool(got[0][0]) if got is not None else False
        lane = bool(host.vgxt_raster_cover(a.ctypes.data, b.ctypes.data, c.ctypes.data, x, y))
        assert lane == model, (int(g), x, y)
        if products_exact(a, b, c, x, y):
            regime += 1
            exact = exact_cover(a, b, c, x, y)
            covered += exact
            if exact != model:
                wrong.append((int(g), x, y, model, exact))
    assert not wrong, (len(wrong), wrong[:5])
    assert regime >= 0.95 * len(pairs), (regime, len(pairs))
    assert 200 < covered < regime - 200  # both outcomes


def rand_f32(rs, n, far):
    m = rs.uniform(-1, 1, n)
    e = rs.randint(-40, 41, n) if far else rs.randint(0, 10, n)
    return (m * np.power(2.0, e)).astype(F)


def test_seam_property(host):
    """A shared edge, arbitrary binary32 endpoints (far-off exponents included), taken in its two directions by two triangles of either
    orientation: the two canonical edge values are exact negatives of each other, and exactly one direction takes a tie."""
    rs = np.random.RandomState(6)
    n = 4000
    ux, uy, vx, vy = (rand_f32(rs, n, k % 2 == 0) for k in range(4))
    ux[::7], uy[::11] = vx[::7], vy[::11]  # vertical and horizontal edges
    px = np.where(rs.rand(n) < 0.5, np.floor(rs.uniform(-600, 600, n)) + 0.5, rs.uniform(-1, 1, n) * np.power(2.0, rs.randint(-30, 31, n)))
    py = np.where(rs.rand(n) < 0.5, np.floor(rs.uniform(-600, 600, n)) + 0.5, rs.uniform(-1, 1, n) * np.power(2.0, rs.randint(-30, 31, n)))
    zeros = 0
    for k in range(n):
        u, v = np.array([ux[k], uy[k]], dtype=F), np.array([vx[k], vy[k]], dtype=F)
        if k % 13 == 0:  # a sample on the edge: the midpoint, where binary64 holds it exactly
            px[k], py[k] = (D(u[0]) + D(v[0])) / 2, (D(u[1]) + D(v[1])) / 2
        if u.tobytes() == v.tobytes():
            continue
        for s1, s2 in ((1, 1), (0, 0), (1, 0)):
            t1, t2 = C.c_int(), C.c_int()
            # same orientation: the neighbour walks the edge the other way; opposite orientations: it walks it the same way
            e1 = host.vgxt_raster_edge(u.ctypes.data, v.ctypes.data, s1, px[k], py[k], C.byref(t1))
            e2 = host.vgxt_raster_edge(*((v.ctypes.data, u.ctypes.data) if s1 == s2 else (u.ctypes.data, v.ctypes.data)), s2, px[k], py[k], C.byref(t2))
            assert e1 == -e2 and not np.isnan(e1), (k, e1, e2)
            assert t1.value + t2.value == 1, k
            zeros += e1 == 0
            m1, _ = R.edge(u, v, 1.0 if s1 else -1.0, np.array([px[k]]), np.array([py[k]]))
            assert m1[0] == e1
    assert zeros > 100  # ties were there to be taken
    # u == v bit for bit: the value is 0 whatever the sample
    u = np.array([3.25, -7.5], dtype=F)
    t = C.c_int()
    assert host.vgxt_raster_edge(u.ctypes.data, u.ctypes.data, 1, 1e300, -1e300, C.byref(t)) == 0.0


def test_host_argument_checks(host):
    f = R.frame("lattice")
    img = f.target.background()
    d = f.desc()

    def call(tgt=None, desc=d, ptr=img.ctypes.data, bounds=None, status=None, **kw):
        t = (tgt or f.target).struct(ptr)
        for k, v in kw.items():
            setattr(t, k, v)
        return host.vgxt_raster(C.byref(desc) if desc is not None else None, bounds, 0, f.nm, C.byref(t), status)

    bad = capi.VGX_E_INVALID_ARG
    assert call(desc=None) == bad
    assert host.vgxt_raster(C.byref(d), None, 0, f.nm, None, None) == bad
    assert call(ptr=None) == bad and call(ptr=img.ctypes.data + 2) == bad
    assert call(stride=f.target.width - 1) == bad
    assert call(width=16385, stride=16385) == bad and call(height=16385) == bad
    assert call(x0=(1 << 23) + 1) == bad and call(y0=-(1 << 23) - 1) == bad
    assert call(scissor=(C.c_uint32 * 4)(5, 0, 4, 10)) == bad and call(scissor=(C.c_uint32 * 4)(0, 0, f.target.width + 1, 10)) == bad
    assert call(scissor=(C.c_uint32 * 4)(0, 9, 4, 8)) == bad and call(scissor=(C.c_uint32 * 4)(0, 0, 4, f.target.height + 1)) == bad
    assert call(bounds=img.ctypes.data + 4) == bad and call(status=img.ctypes.data + 1) == bad
    assert call(desc=capi.CacheDesc(None, d.color, d.idx, d.meshes, f.nm, f.nv, f.ni)) == bad
    assert call(desc=capi.CacheDesc(d.pos, d.color, d.idx, d.meshes, 0xFFFFFFFF, f.nv, f.ni)) == capi.VGX_E_RANGE
    assert np.array_equal(img, f.target.background())  # none of them wrote
    # valid and writing nothing: an empty scissor (no pixels needed), an image without pixels, no meshes
    assert call(ptr=None, scissor=(C.c_uint32 * 4)(7, 7, 7, 20), flags=capi.RASTER_CLEAR) == capi.VGX_OK
    assert call(ptr=None, width=0, stride=0, scissor=(C.c_uint32 * 4)(0, 0, 0, 0)) == capi.VGX_OK
    assert call(desc=capi.CacheDesc(None, None, None, None, 0, 0, 0)) == capi.VGX_OK
    assert call(x0=1 << 23, y0=-(1 << 23)) == capi.VGX_OK
    assert np.array_equal(img, f.target.background())
