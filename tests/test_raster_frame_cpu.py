"""CPU: the lane code of vgx_raster_frame (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_frame, vgxt_raster's plain loop
with the draw's scissor and a stamp image of its own) against the numpy statement (tests/raster_frame_model.py), and against
vgxt_raster where the new state must change nothing or amounts to a scissor. Exact everywhere: np.array_equal on the uint32 images,
the stride padding and everything outside the scissor included. tests/test_gpu_raster_frame.py makes the same comparisons on the
kernels."""
import ctypes as C
import importlib

import numpy as np
import pytest

import raster_frame_model as M
import raster_model as R
import test_raster_cpu as base

capi = R.capi
NONE = M.NONE
CLEAR = 0xFF102030


def load_host():
    lib = base.load_host()
    if not hasattr(lib, "vgxt_raster_frame"):  # a library from before this call: build again
        import __graft_entry__ as g
        g.build()
        lib = base.load_host()
    lib.vgxt_raster_frame.restype = C.c_int
    lib.vgxt_raster_frame.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(capi.RasterDraws), C.POINTER(capi.RasterTarget),
                                      C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def draws_struct(f):
    nd = f.draws.shape[0]
    return capi.RasterDraws(f.draws.ctypes.data if nd else None, f.dstate.ctypes.data if nd else None, nd, 0)


def host_frame(host, f, tgt, image=None, with_bounds=False, begin=0, end=2**64 - 1, want=capi.VGX_OK):
    """vgxt_raster_frame over the target's background (or `image`, changed in place); returns the image."""
    img = tgt.background() if image is None else image
    mb = base.host_bounds(host, f) if with_bounds else None
    d, s, t = f.desc(), draws_struct(f), tgt.struct(img.ctypes.data)
    status = np.full(1, 77, dtype=np.uint32)
    assert host.vgxt_raster_frame(C.byref(d), None if mb is None else mb.ctypes.data, begin, end, C.byref(s), C.byref(t), status.ctypes.data) == capi.VGX_OK
    assert status[0] == want
    return img


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", M.NAMES + ("decoded",))
def test_lane_code_equals_model(host, rt, name, clear):
    M.check_conditions(name, rt)
    f = M.frame(name, rt)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = M.expected(name, clear, rt)
    got = host_frame(host, f, tgt)
    assert np.array_equal(got, want), base.where(got, want)
    assert R.guards_intact(tgt, got)
    assert np.array_equal(host_frame(host, f, tgt, with_bounds=True), got)  # the boxes handed in: the same bytes


def whole(f, scissors=None):
    """The frame with a state that changes nothing: one draw per mesh, no regions, `scissors` (or the whole canvas) per draw."""
    g = R.make(f.name, f.pos, f.color, f.idx, f.meshes, f.target)
    return M.with_draws(g, list(range(g.nm)), [0] * g.nm, [M.state(scissor=M.BIG if scissors is None else scissors[m]) for m in range(g.nm)])


def tiger_window():
    """The Tiger frame's own target starts at frame pixel (-40, -30), and a draw scissor is unsigned: no scissor holds those pixels.
    The same window from frame pixel (0, 0) still lies inside the drawing; there "the whole canvas" cuts nothing."""
    t = R.frame("tiger").target
    return R.Target(t.width, t.height, t.stride, 0, 0, scissor=t.scissor)


def test_unused_state_equals_vgxt_raster(host):
    """(a) every draw's scissor the whole canvas, no regions: vgxt_raster's bytes."""
    f = R.frame("tiger")
    for tgt in (tiger_window(), tiger_window().with_clear(CLEAR)):
        got = host_frame(host, whole(f), tgt)
        assert np.array_equal(got, base.host_render(host, f, tgt)), base.where(got, base.host_render(host, f, tgt))
        assert R.guards_intact(tgt, got) and int((got != tgt.background()).sum()) > 10000


def frame_scissor(tgt, sc):
    """A draw scissor {x, y, w, h} in frame pixels as a target scissor, cut by the target's own."""
    return M.draw_rect(tgt, sc)


def test_three_scissors_equal_three_calls(host):
    """(b) three per-draw scissors on three runs of meshes: three vgxt_raster calls, each under the target's scissor cut by the draw's."""
    f = R.frame("tiger")
    tgt = f.target  # frame pixels (-40 .. 160) x (-30 .. 130); a uint16 scissor starts at 0 or later
    cuts = [(0, 0, 70, 130), (37, 21, 100, 50), (90, 3, 200, 200)]
    a, b = f.nm // 3, 2 * f.nm // 3
    g = whole(f, [cuts[0] if m < a else (cuts[1] if m < b else cuts[2]) for m in range(f.nm)])
    got = host_frame(host, g, tgt)
    want = tgt.background()
    for (lo, hi), c in zip(((0, a), (a, b), (b, f.nm)), cuts):
        sc = frame_scissor(tgt, c)
        assert sc[0] < sc[2] and sc[1] < sc[3] and sc != tgt.scissor
        base.host_render(host, f, R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, sc), image=want, begin=lo, end=hi)
    assert np.array_equal(got, want), base.where(got, want)
    assert not np.array_equal(got, R.expected("tiger"))


def clipped_tiger(rule, rect=(20, 10, 110, 90)):
    """The Tiger frame behind one clip quad with integer corners {x, y, w, h}: mesh 0 is the quad, the Tiger's meshes follow."""
    f = R.frame("tiger")
    x, y, w, h = rect
    b = R.Builder()
    b.mesh(M.quad(float(x), float(y), float(x + w), float(y + h)), 0xFFFFFFFF, M.QUAD)
    nv, ni = 4, 6
    meshes = f.meshes.copy()
    meshes["first_vertex"] += nv
    meshes["first_index"] += ni
    first = np.array(b.meshes, dtype=capi.mesh_dtype)
    g = R.make("tiger_clip", np.concatenate([np.array(b.pos, dtype=np.float32), f.pos]), np.concatenate([np.array(b.color, dtype=np.uint32), f.color]),
               np.concatenate([np.array(b.idx, dtype=np.uint16), f.idx]), np.concatenate([first, meshes]), tiger_window())
    return M.with_draws(g, [0] + [1] * f.nm, [M.CLIP, 0], [M.state(), M.state(region=(0, 1), rule=rule)])


def test_in_region_of_a_rectangle_is_a_scissor(host):
    """(c) an In region made of one axis-aligned quad with integer corners: vgxt_raster under the scissor of that rectangle. A pixel
    centre is never on the quad's outline, so the tie rule has nothing to decide."""
    f = R.frame("tiger")
    tgt = tiger_window()
    rect = (20, 10, 110, 90)
    got = host_frame(host, clipped_tiger(0, rect), tgt)
    sc = frame_scissor(tgt, rect)
    want = base.host_render(host, f, R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, sc))
    assert np.array_equal(got, want), base.where(got, want)
    assert not np.array_equal(got, tgt.background()) and not np.array_equal(got, base.host_render(host, f, tgt))


def test_out_region_of_a_rectangle_is_its_complement(host):
    """(d) an Out region made of the same quad: the unclipped render outside the rectangle, the background inside."""
    f = R.frame("tiger")
    tgt = tiger_window()
    rect = (20, 10, 110, 90)
    got = host_frame(host, clipped_tiger(1, rect), tgt)
    x0, y0, x1, y1 = frame_scissor(tgt, rect)
    plain = base.host_render(host, f, tgt)
    want = plain.copy()
    want[y0:y1, x0:x1] = tgt.background()[y0:y1, x0:x1]
    assert np.array_equal(got, want), base.where(got, want)
    assert not np.array_equal(got, plain)


def test_mesh_range_that_does_not_start_at_0(host):
    """The range [2, 7) of `clips` holds region 1's second clip mesh, region 2 and their users: the model of that range. And a range
    that leaves its clip meshes out sees S = NONE everywhere: In draws nothing, Out everything."""
    f = M.frame("clips")
    want = M.render(f, f.target, f.target.background(), mesh_begin=2, mesh_end=7)
    got = host_frame(host, f, f.target, begin=2, end=7)
    assert np.array_equal(got, want), base.where(got, want)
    assert not np.array_equal(got, M.expected("clips")) and not np.array_equal(got, f.target.background())
    assert np.array_equal(host_frame(host, f, f.target, begin=3, end=4), f.target.background())
    g = R.make("x", f.pos, f.color, f.idx, f.meshes, f.target)
    assert np.array_equal(host_frame(host, f, f.target, begin=5, end=6), base.host_render(host, g, f.target, begin=5, end=6))


def test_invalid_draw_index_writes_nothing(host):
    f = M.clips()
    f.meshes["draw"][8] = f.draws.shape[0]
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        assert M.status(f) == capi.VGX_E_INVALID_ARG
        got = host_frame(host, f, tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
        assert np.array_equal(M.render(f, tgt, tgt.background()), tgt.background())
    # a range without the mesh is drawn
    got = host_frame(host, f, f.target, end=8)
    assert np.array_equal(got, M.render(M.frame("clips"), f.target, f.target.background(), mesh_end=8))
    # a TEXT mesh is skipped, its draw index is looked at all the same
    f = M.lattice_clip()
    f.meshes["subpath_kind"][1] = R.TEXT << 28
    f.meshes["draw"][1] = 3
    assert np.array_equal(host_frame(host, f, f.target, want=capi.VGX_E_INVALID_ARG), f.target.background())


def test_empty_range_and_empty_draw_scissor(host):
    f = M.frame("clips")
    assert np.array_equal(host_frame(host, f, f.target, begin=f.nm), f.target.background())
    tc = f.target.with_clear(0x01020304)
    img = host_frame(host, f, tc, begin=3, end=3)
    sx0, sy0, sx1, sy1 = tc.scissor
    assert np.all(img[sy0:sy1, sx0:sx1] == 0x01020304) and R.guards_intact(tc, img)
    # w == 0 or h == 0, or a scissor that misses the image: the mesh does nothing (the backdrop of `clips` here)
    for sc in ((10, 10, 0, 50), (10, 10, 50, 0), (3000, 10, 50, 50), (65535, 65535, 65535, 65535)):
        g = M.clips()
        g.dstate["scissor"][0] = sc
        want = M.render(g, g.target, g.target.background())
        assert np.array_equal(host_frame(host, g, g.target), want)
        assert not np.array_equal(want, M.expected("clips"))
    assert np.array_equal(host_frame(host, g, g.target, end=1), g.target.background())


def test_host_argument_checks(host):
    f = M.frame("lattice_clip")
    img = f.target.background()
    d = f.desc()
    bad = capi.VGX_E_INVALID_ARG

    def call(state=None, no_state=False, desc=d, ptr=img.ctypes.data, bounds=None, status=None, **kw):
        t = f.target.struct(ptr)
        for k, v in kw.items():
            setattr(t, k, v)
        s = draws_struct(f) if state is None else state
        return host.vgxt_raster_frame(C.byref(desc) if desc is not None else None, bounds, 0, f.nm, None if no_state else C.byref(s), C.byref(t), status)

    dr, ds, nd = f.draws.ctypes.data, f.dstate.ctypes.data, f.draws.shape[0]
    assert call(no_state=True) == bad
    assert call(state=capi.RasterDraws(None, ds, nd, 0)) == bad and call(state=capi.RasterDraws(dr, None, nd, 0)) == bad
    assert call(state=capi.RasterDraws(dr + 2, ds, nd, 0)) == bad and call(state=capi.RasterDraws(dr, ds + 1, nd, 0)) == bad
    assert call(state=capi.RasterDraws(dr, ds, nd, 1)) == bad
    # as vgxt_raster
    assert call(desc=None) == bad and call(ptr=None) == bad and call(ptr=img.ctypes.data + 2) == bad
    assert call(stride=f.target.width - 1) == bad and call(width=16385, stride=16385) == bad and call(x0=(1 << 23) + 1) == bad
    assert call(scissor=(C.c_uint32 * 4)(5, 0, 4, 10)) == bad and call(scissor=(C.c_uint32 * 4)(0, 0, 4, f.target.height + 1)) == bad
    assert call(bounds=img.ctypes.data + 4) == bad and call(status=img.ctypes.data + 1) == bad
    assert call(desc=capi.CacheDesc(d.pos, d.color, d.idx, d.meshes, 0xFFFFFFFF, f.nv, f.ni)) == capi.VGX_E_RANGE
    assert np.array_equal(img, f.target.background())  # none of them wrote
    # valid: no draws and no meshes; null arrays with num_draws == 0 (every mesh is then out of the table: the device status says so)
    assert call(state=capi.RasterDraws(None, None, 0, 0), desc=capi.CacheDesc(None, None, None, None, 0, 0, 0)) == capi.VGX_OK
    status = np.full(1, 77, dtype=np.uint32)
    assert call(state=capi.RasterDraws(None, None, 0, 0), status=status.ctypes.data) == capi.VGX_OK and status[0] == bad
    assert call(ptr=None, scissor=(C.c_uint32 * 4)(7, 7, 7, 20), flags=capi.RASTER_CLEAR) == capi.VGX_OK
    assert np.array_equal(img, f.target.background())


def test_struct_sizes():
    assert C.sizeof(capi.RasterDraws) == 24 and capi.draw_state_dtype.itemsize == 24
