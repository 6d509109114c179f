"""CPU: the lane code of vgx_raster_frame (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_frame, vgxt_raster's plain loop
with the draw's scissor and a stamp image of its own) against the numpy statement (tests/raster_frame_model.py), and against
vgxt_raster where the new state must change nothing or amounts to a scissor. Exact everywhere: np.array_equal on the uint32 images,
the stride padding and everything outside the scissor included. tests/test_gpu_raster_frame.py makes the same comparisons on the
kernels."""
import ctypes as C

import numpy as np
import pytest

import raster_frame_model as M
import raster_harness as H
import raster_model as R
from raster_harness import clipped_tiger, draws_struct, host, rt, tiger_window, whole  # noqa: F401 (host, rt: fixtures)

capi = R.capi
NONE = M.NONE
CLEAR = 0xFF102030


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", M.NAMES + ("decoded",))
def test_lane_code_equals_model(host, rt, name, clear):
    M.check_conditions(name, rt)
    f = M.frame(name, rt)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = M.expected(name, clear, rt)
    got = H.host_level(host, "frame", f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
    assert R.guards_intact(tgt, got)
    assert np.array_equal(H.host_level(host, "frame", f, tgt, with_bounds=True), got)  # the boxes handed in: the same bytes


def test_unused_state_equals_vgxt_raster(host):
    """(a) every draw's scissor the whole canvas, no regions: vgxt_raster's bytes."""
    f = R.frame("tiger")
    for tgt in (tiger_window(), tiger_window().with_clear(CLEAR)):
        got = H.host_level(host, "frame", whole(f), tgt)
        assert np.array_equal(got, H.host_level(host, "raster", f, tgt)), H.where(got, H.host_level(host, "raster", f, tgt))
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
    got = H.host_level(host, "frame", g, tgt)
    want = tgt.background()
    for (lo, hi), c in zip(((0, a), (a, b), (b, f.nm)), cuts):
        sc = frame_scissor(tgt, c)
        assert sc[0] < sc[2] and sc[1] < sc[3] and sc != tgt.scissor
        H.host_level(host, "raster", f, R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, sc), image=want, begin=lo, end=hi)
    assert np.array_equal(got, want), H.where(got, want)
    assert not np.array_equal(got, R.expected("tiger"))


def test_in_region_of_a_rectangle_is_a_scissor(host):
    """(c) an In region made of one axis-aligned quad with integer corners: vgxt_raster under the scissor of that rectangle. A pixel
    centre is never on the quad's outline, so the tie rule has nothing to decide."""
    f = R.frame("tiger")
    tgt = tiger_window()
    rect = (20, 10, 110, 90)
    got = H.host_level(host, "frame", clipped_tiger(0, rect), tgt)
    sc = frame_scissor(tgt, rect)
    want = H.host_level(host, "raster", f, R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, sc))
    assert np.array_equal(got, want), H.where(got, want)
    assert not np.array_equal(got, tgt.background()) and not np.array_equal(got, H.host_level(host, "raster", f, tgt))


def test_out_region_of_a_rectangle_is_its_complement(host):
    """(d) an Out region made of the same quad: the unclipped render outside the rectangle, the background inside."""
    f = R.frame("tiger")
    tgt = tiger_window()
    rect = (20, 10, 110, 90)
    got = H.host_level(host, "frame", clipped_tiger(1, rect), tgt)
    x0, y0, x1, y1 = frame_scissor(tgt, rect)
    plain = H.host_level(host, "raster", f, tgt)
    want = plain.copy()
    want[y0:y1, x0:x1] = tgt.background()[y0:y1, x0:x1]
    assert np.array_equal(got, want), H.where(got, want)
    assert not np.array_equal(got, plain)


def test_mesh_range_that_does_not_start_at_0(host):
    """The range [2, 7) of `clips` holds region 1's second clip mesh, region 2 and their users: the model of that range. And a range
    that leaves its clip meshes out sees S = NONE everywhere: In draws nothing, Out everything."""
    f = M.frame("clips")
    want = M.render(f, f.target, f.target.background(), mesh_begin=2, mesh_end=7)
    got = H.host_level(host, "frame", f, f.target, begin=2, end=7)
    assert np.array_equal(got, want), H.where(got, want)
    assert not np.array_equal(got, M.expected("clips")) and not np.array_equal(got, f.target.background())
    assert np.array_equal(H.host_level(host, "frame", f, f.target, begin=3, end=4), f.target.background())
    g = R.make("x", f.pos, f.color, f.idx, f.meshes, f.target)
    assert np.array_equal(H.host_level(host, "frame", f, f.target, begin=5, end=6), H.host_level(host, "raster", g, f.target, begin=5, end=6))


def test_invalid_draw_index_writes_nothing(host):
    f = M.clips()
    f.meshes["draw"][8] = f.draws.shape[0]
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        assert M.status(f) == capi.VGX_E_INVALID_ARG
        got = H.host_level(host, "frame", f, tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
        assert np.array_equal(M.render(f, tgt, tgt.background()), tgt.background())
    # a range without the mesh is drawn
    got = H.host_level(host, "frame", f, f.target, end=8)
    assert np.array_equal(got, M.render(M.frame("clips"), f.target, f.target.background(), mesh_end=8))
    # a TEXT mesh is skipped, its draw index is looked at all the same
    f = M.lattice_clip()
    f.meshes["subpath_kind"][1] = R.TEXT << 28
    f.meshes["draw"][1] = 3
    assert np.array_equal(H.host_level(host, "frame", f, f.target, want=capi.VGX_E_INVALID_ARG), f.target.background())


def test_empty_range_and_empty_draw_scissor(host):
    f = M.frame("clips")
    assert np.array_equal(H.host_level(host, "frame", f, f.target, begin=f.nm), f.target.background())
    tc = f.target.with_clear(0x01020304)
    img = H.host_level(host, "frame", f, tc, begin=3, end=3)
    sx0, sy0, sx1, sy1 = tc.scissor
    assert np.all(img[sy0:sy1, sx0:sx1] == 0x01020304) and R.guards_intact(tc, img)
    # w == 0 or h == 0, or a scissor that misses the image: the mesh does nothing (the backdrop of `clips` here)
    for sc in ((10, 10, 0, 50), (10, 10, 50, 0), (3000, 10, 50, 50), (65535, 65535, 65535, 65535)):
        g = M.clips()
        g.dstate["scissor"][0] = sc
        want = M.render(g, g.target, g.target.background())
        assert np.array_equal(H.host_level(host, "frame", g, g.target), want)
        assert not np.array_equal(want, M.expected("clips"))
    assert np.array_equal(H.host_level(host, "frame", g, g.target, end=1), g.target.background())


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
