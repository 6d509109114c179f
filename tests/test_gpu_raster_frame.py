"""GPU: vgx_raster_frame (csrc/vgx_raster.hip: the frame family k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<false, false> at
the frame level) against the numpy statement
(tests/raster_frame_model.py) on its four frames -- `decoded` after GPU tessellation of the decoded batch -- and against vgx_raster
where the new state must change nothing or amounts to a scissor. Every comparison is np.array_equal on the whole uint32 buffer: the
stride padding and everything outside the scissor included."""
import ctypes as C

import numpy as np
import pytest

import raster_frame_model as M
import raster_harness as H
import raster_model as R
from raster_harness import DevFrame, DevState, dev_frame, gpu_bounds, rt, warm_ctx, where  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = 0xFF102030


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", M.NAMES)
def test_kernels_equal_model(rt, warm_ctx, name, clear):
    M.check_conditions(name)
    f = M.frame(name)
    df, ds = DevFrame(f), DevState(f)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = M.expected(name, clear)
    _, own = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt)
    assert np.array_equal(own, want), where(own, want)
    assert R.guards_intact(tgt, own)
    _, given = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt, bounds=gpu_bounds(rt, warm_ctx, df))
    assert np.array_equal(given, want), where(given, want)
    _, again = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt)
    assert np.array_equal(again, own)  # two runs, the same bytes
    assert df.unchanged()


def test_decoded_frame_after_gpu_tessellation(rt, warm_ctx):
    """Command-list bytes -> vgx_cmdlist_decode -> path set -> the tessellator on the device -> vgx_raster_frame: the model's image of
    the same decode tessellated by the CPU oracle."""
    import torch
    M.check_conditions("decoded", rt)
    f = M.frame("decoded", rt)
    pset = rt.PathSet(warm_ctx, f.pathset)
    dd = rt.upload_draws(f.draws)
    sizes = rt.tessellate_count(warm_ctx, pset, dd, f.draws.shape[0])
    assert (sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]) == (f.nv, f.ni, f.nm)
    bufs = rt.MeshBuffers(dd.device, f.nv, f.ni, f.nm)
    rt.tessellate_emit(warm_ctx, pset, dd, f.draws.shape[0], bufs)
    torch.cuda.synchronize()
    pset.close()

    class Dev:
        desc = capi.CacheDesc(bufs.pos.data_ptr(), bufs.color.data_ptr(), bufs.idx.data_ptr(), bufs.meshes.data_ptr(), f.nm, f.nv, f.ni)
    ds = DevState(f)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = M.expected("decoded", clear, rt)
        _, got = H.gpu_level(rt, warm_ctx, "frame", Dev, ds, tgt=tgt)
        assert np.array_equal(got, want), where(got, want)
        assert R.guards_intact(tgt, got)
    # the runtime wrapper, on an image of its own
    img, status = rt.raster_frame(warm_ctx, Dev.desc, ds.t[0], ds.t[1], f.draws.shape[0], f.target.width, f.target.height, clear_color=CLEAR)
    torch.cuda.synchronize()
    t = f.target
    want = M.render(f, R.Target(t.width, t.height, t.width, 0, 0, clear=CLEAR), np.zeros((t.height, t.width), dtype=np.uint32))
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), want)


def test_unused_state_equals_vgx_raster(rt, warm_ctx):
    """(a) every draw's scissor the whole canvas, no regions: vgx_raster's bytes."""
    f = R.frame("tiger")
    g = H.whole(f)
    df, ds = dev_frame(f), DevState(g)
    dg = DevFrame(g)  # the same streams, every mesh a draw of its own
    for tgt in (H.tiger_window(), H.tiger_window().with_clear(CLEAR)):
        _, got = H.gpu_level(rt, warm_ctx, "frame", dg, ds, tgt=tgt)
        _, want = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt)
        assert np.array_equal(got, want), where(got, want)
        assert R.guards_intact(tgt, got) and int((got != tgt.background()).sum()) > 10000


def test_three_scissors_equal_three_calls(rt, warm_ctx):
    """(b) three per-draw scissors on three runs of meshes: three vgx_raster calls, each under the target's scissor cut by the draw's."""
    f = R.frame("tiger")
    tgt = f.target
    cuts = [(0, 0, 70, 130), (37, 21, 100, 50), (90, 3, 200, 200)]
    a, b = f.nm // 3, 2 * f.nm // 3
    g = H.whole(f, [cuts[0] if m < a else (cuts[1] if m < b else cuts[2]) for m in range(f.nm)])
    df = dev_frame(f)
    _, got = H.gpu_level(rt, warm_ctx, "frame", DevFrame(g), DevState(g), tgt=tgt)
    img, want = None, None
    for (lo, hi), c in zip(((0, a), (a, b), (b, f.nm)), cuts):
        sc = M.draw_rect(tgt, c)
        img, want = H.gpu_level(rt, warm_ctx, "raster", df, tgt=R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, sc), image=img, begin=lo, end=hi)
    assert np.array_equal(got, want), where(got, want)
    assert not np.array_equal(got, R.expected("tiger")) and not np.array_equal(got, tgt.background())


@pytest.mark.parametrize("rule", [0, 1])
def test_region_of_a_rectangle(rt, warm_ctx, rule):
    """(c) an In region made of one axis-aligned quad with integer corners is vgx_raster under the scissor of that rectangle; (d) as an
    Out region it leaves the unclipped render outside the rectangle and the background inside."""
    f = R.frame("tiger")
    tgt = H.tiger_window()
    rect = (20, 10, 110, 90)
    g = H.clipped_tiger(rule, rect)
    _, got = H.gpu_level(rt, warm_ctx, "frame", DevFrame(g), DevState(g), tgt=tgt)
    x0, y0, x1, y1 = M.draw_rect(tgt, rect)
    _, plain = H.gpu_level(rt, warm_ctx, "raster", dev_frame(f), tgt=tgt)
    if rule == 0:
        _, want = H.gpu_level(rt, warm_ctx, "raster", dev_frame(f), tgt=R.Target(tgt.width, tgt.height, tgt.stride, tgt.x0, tgt.y0, (x0, y0, x1, y1)))
    else:
        want = plain.copy()
        want[y0:y1, x0:x1] = tgt.background()[y0:y1, x0:x1]
    assert np.array_equal(got, want), where(got, want)
    assert not np.array_equal(got, plain) and not np.array_equal(got, tgt.background())


def test_mesh_range_that_does_not_start_at_0(rt, warm_ctx):
    f = M.frame("clips")
    df, ds = DevFrame(f), DevState(f)
    want = M.render(f, f.target, f.target.background(), mesh_begin=2, mesh_end=7)
    _, got = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=f.target, begin=2, end=7)
    assert np.array_equal(got, want), where(got, want)
    tc = f.target.with_clear(0x01020304)
    _, got = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tc, begin=3, end=3)  # an empty range: only the clear
    sx0, sy0, sx1, sy1 = tc.scissor
    assert np.all(got[sy0:sy1, sx0:sx1] == 0x01020304) and R.guards_intact(tc, got)


def test_fresh_context_grows_then_succeeds(rt):
    """A fresh context holds one bin entry per mesh: the first call ends with VGX_E_GROWN and has written NOTHING, the clear included;
    the repeat succeeds. After vgx_raster_reserve one call is enough. vgx_scratch_bytes counts the per-mesh state of this call."""
    t = R.frame("tiger")  # moved so that its own window starts at frame pixel (0, 0): no draw scissor cuts it, its meshes reach several tiles each
    f = R.make("tiger_moved", t.pos + np.array([-t.target.x0, -t.target.y0], dtype=np.float32), t.color, t.idx, t.meshes, H.tiger_window())
    g = H.whole(f)
    df, dg, ds = DevFrame(f), DevFrame(g), DevState(g)
    tgt = f.target.with_clear(CLEAR)
    entries = R.bin_entries(f, tgt)
    ctx = rt.Context(0)
    try:
        _, want = H.gpu_level(rt, ctx, "raster", df, tgt=tgt, want=capi.VGX_E_GROWN)
        assert np.array_equal(want, tgt.background())
        _, want = H.gpu_level(rt, ctx, "raster", df, tgt=tgt)
    finally:
        ctx.close()
    H.check_fresh_context_grows_then_succeeds(rt, lambda ctx, tgt, **kw: H.gpu_level(rt, ctx, "frame", dg, ds, tgt=tgt, **kw), f, lambda tgt: want, entries,
                                              min_growth=32 * f.nm)  # the buffer only this call allocates


def test_invalid_draw_index_writes_nothing(rt, warm_ctx):
    f = M.clips()
    f.meshes["draw"][8] = f.draws.shape[0]
    df, ds = DevFrame(f), DevState(f)
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        _, got = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
    _, got = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=f.target, end=8)  # a range without the mesh is drawn
    assert np.array_equal(got, M.render(M.frame("clips"), f.target, f.target.background(), mesh_end=8))
    # it ranks above VGX_E_GROWN: a fresh context, more entries than it holds, and the bad index
    t = R.frame("tiger")
    g = H.whole(t)
    g.meshes["draw"][t.nm // 2] = t.nm
    ctx = rt.Context(0)
    try:
        tgt = H.tiger_window().with_clear(CLEAR)
        _, got = H.gpu_level(rt, ctx, "frame", DevFrame(g), DevState(g), tgt=tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
    finally:
        ctx.close()


def test_refused_calls(rt, warm_ctx):
    import torch
    f = M.frame("lattice_clip")
    df, ds = DevFrame(f), DevState(f)
    t = f.target
    image = torch.from_numpy(t.background().view(np.int32)).to("cuda:0")
    lib = rt.lib()
    dr, dst, nd = ds.t[0].data_ptr(), ds.t[1].data_ptr(), f.draws.shape[0]

    def call(state=None, no_state=False, **kw):
        s = t.struct(image.data_ptr())
        for k, v in kw.items():
            setattr(s, k, v)
        st = ds.struct if state is None else state
        return lib.vgx_raster_frame(warm_ctx.handle, C.byref(df.desc), None, 0, f.nm, None if no_state else C.byref(st), C.byref(s), None, rt._stream_ptr())

    bad = capi.VGX_E_INVALID_ARG
    assert call(no_state=True) == bad
    assert call(state=capi.RasterDraws(None, dst, nd, 0)) == bad and call(state=capi.RasterDraws(dr, None, nd, 0)) == bad
    assert call(state=capi.RasterDraws(dr + 2, dst, nd, 0)) == bad and call(state=capi.RasterDraws(dr, dst + 1, nd, 0)) == bad
    assert call(state=capi.RasterDraws(dr, dst, nd, 1)) == bad
    assert call(stride=t.width - 1) == bad and call(scissor=(C.c_uint32 * 4)(5, 0, 4, 10)) == bad
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().view(np.uint32), t.background())


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_raster_frame of another stream -> vgx_tessellate_emit gives the meshes it gives without the call."""
    f = M.frame("stack_clip")
    df, ds = DevFrame(f), DevState(f)
    call = lambda: rt.raster_frame(gpu_ctx, df.desc, ds.t[0], ds.t[1], f.draws.shape[0], f.target.width, f.target.height, clear_color=CLEAR)
    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, call, M.expected("stack_clip", True))


def test_vgx_raster_after_vgx_raster_frame(rt):
    """The two calls share their tables: vgx_raster on raster_model's frames gives the model's bytes after a vgx_raster_frame call on the
    same context."""
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, 8192, 1 << 17)
        c = M.frame("clips")
        dc, sc = DevFrame(c), DevState(c)
        for name in ("lattice", "stack", "tiger"):
            _, got = H.gpu_level(rt, ctx, "frame", dc, sc, tgt=c.target)
            assert np.array_equal(got, M.expected("clips"))
            f = R.frame(name)
            _, got = H.gpu_level(rt, ctx, "raster", dev_frame(f), tgt=f.target)
            assert np.array_equal(got, R.expected(name)), (name, where(got, R.expected(name)))
    finally:
        ctx.close()
