"""GPU: vgx_raster (csrc/vgx_raster.hip) against the numpy statement of the specification (tests/raster_model.py) on the frames of
tests/test_raster_cpu.py, and against the lane code (vgxt_raster) on a 65-instance Tiger frame the model would be slow on. Every
comparison is np.array_equal on the whole uint32 buffer: the stride padding and everything outside the scissor included."""
import ctypes as C

import numpy as np
import pytest

import raster_harness as H
import raster_model as R
from raster_harness import DevFrame, dev_frame, gpu_bounds, rt, warm_ctx, where  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
F = np.float32
CLEAR = 0xFF102030


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", R.NAMES)
def test_kernels_equal_model(rt, warm_ctx, name, clear):
    R.check_conditions(name)
    f = R.frame(name)
    df = dev_frame(f)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = R.expected(name, clear)
    _, own = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt)
    assert np.array_equal(own, want), where(own, want)
    assert R.guards_intact(tgt, own)
    mb = gpu_bounds(rt, warm_ctx, df)
    _, given = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt, bounds=mb)
    assert np.array_equal(given, want), where(given, want)
    _, again = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt)
    assert np.array_equal(again, own)  # two runs, the same bytes
    assert df.unchanged()


@pytest.mark.parametrize("name", R.NAMES)
def test_split_mesh_ranges(rt, warm_ctx, name):
    f = R.frame(name)
    df = dev_frame(f)
    want = R.expected(name)
    mb = gpu_bounds(rt, warm_ctx, df)
    for n, k in enumerate(sorted({1, f.nm // 3, f.nm - 1})):
        img, _ = H.gpu_level(rt, warm_ctx, "raster", df, tgt=f.target, end=k, bounds=mb if n % 2 else None)
        _, got = H.gpu_level(rt, warm_ctx, "raster", df, tgt=f.target, image=img, begin=k, bounds=None if n % 2 else mb)
        assert np.array_equal(got, want), (k, where(got, want))
    # an empty range writes nothing, or only the clear
    _, got = H.gpu_level(rt, warm_ctx, "raster", df, tgt=f.target, begin=f.nm)
    assert np.array_equal(got, f.target.background())
    tc = f.target.with_clear(0x01020304)
    _, got = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tc, begin=1, end=1)
    sx0, sy0, sx1, sy1 = tc.scissor
    assert np.all(got[sy0:sy1, sx0:sx1] == 0x01020304) and R.guards_intact(tc, got)


@pytest.fixture(scope="module")
def tiger65():
    """pick_model's 65-instance Tiger frame through a 1000 x 700 window that cuts instances on every side."""
    p = R.PM.frame("tiger", 65)
    return R.make("tiger65", p.pos, p.color, p.idx, p.meshes, R.Target(1000, 700, 1003, 2000, 1500, scissor=(2, 1, 999, 690)))


def test_kernels_equal_lane_code_on_65_tigers(rt, warm_ctx, tiger65):
    f = tiger65
    host = H.load_host()
    df = DevFrame(f)
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        want = H.host_level(host, "raster", f, tgt)
        assert int((want != tgt.background()).sum()) > 100000
        _, got = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt)
        assert np.array_equal(got, want), where(got, want)
        assert R.guards_intact(tgt, got)
        _, given = H.gpu_level(rt, warm_ctx, "raster", df, tgt=tgt, bounds=gpu_bounds(rt, warm_ctx, df))
        assert np.array_equal(given, want)
    k = f.nm // 2 + 7
    img, _ = H.gpu_level(rt, warm_ctx, "raster", df, tgt=f.target, end=k)
    _, got = H.gpu_level(rt, warm_ctx, "raster", df, tgt=f.target, image=img, begin=k)
    assert np.array_equal(got, H.host_level(host, "raster", f, f.target))
    assert df.unchanged()


def test_fresh_context_grows_then_succeeds(rt):
    """A fresh context holds one bin entry per mesh (plus the head room of a scratch table): the Tiger's meshes reach several tiles
    each, so the first call ends with VGX_E_GROWN and has written NOTHING, the clear included; the repeat succeeds. After
    vgx_raster_reserve one call is enough. vgx_scratch_bytes counts the scratch."""
    f = R.frame("tiger")
    df = dev_frame(f)
    tgt = f.target.with_clear(CLEAR)
    entries = R.bin_entries(f, tgt)
    assert entries > 2 * f.nm + 64, (entries, f.nm)  # condition on the input: the first guess cannot hold them
    ctx = rt.Context(0)
    try:
        before = int(rt.lib().vgx_scratch_bytes(ctx.handle))
        img, got = H.gpu_level(rt, ctx, "raster", df, tgt=tgt, want=capi.VGX_E_GROWN)
        assert np.array_equal(got, tgt.background())
        first = int(rt.lib().vgx_scratch_bytes(ctx.handle))
        assert first - before >= 16 * f.nm
        _, got = H.gpu_level(rt, ctx, "raster", df, tgt=tgt, image=img)
        assert np.array_equal(got, R.expected("tiger", True)), where(got, R.expected("tiger", True))
        grown = int(rt.lib().vgx_scratch_bytes(ctx.handle))
        assert grown - first >= 16 * (entries // 2 - f.nm) > 0
        _, got = H.gpu_level(rt, ctx, "raster", df, tgt=tgt)
        assert np.array_equal(got, R.expected("tiger", True))
        assert int(rt.lib().vgx_scratch_bytes(ctx.handle)) == grown  # and stays
    finally:
        ctx.close()
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, f.nm, entries)
        reserved = int(rt.lib().vgx_scratch_bytes(ctx.handle))
        assert reserved >= 16 * entries + 12 * f.nm
        _, got = H.gpu_level(rt, ctx, "raster", df, tgt=tgt)
        assert np.array_equal(got, R.expected("tiger", True))
    finally:
        ctx.close()


def test_runtime_wrapper_and_refused_calls(rt, warm_ctx):
    import torch
    f = R.frame("lattice")
    df = dev_frame(f)
    t = f.target
    img, status = rt.raster(warm_ctx, df.desc, t.width, t.height, t.x0, t.y0, clear_color=CLEAR)
    torch.cuda.synchronize()
    want = R.render(f, R.Target(t.width, t.height, t.width, t.x0, t.y0, clear=CLEAR), np.zeros((t.height, t.width), dtype=np.uint32))
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), want)
    # refused on the host: nothing enqueued, nothing written
    image = torch.from_numpy(t.background().view(np.int32)).to("cuda:0")
    lib = rt.lib()

    def call(ptr=image.data_ptr(), desc=df.desc, bounds=None, status=None, **kw):
        s = t.struct(ptr)
        for k, v in kw.items():
            setattr(s, k, v)
        return lib.vgx_raster(warm_ctx.handle, C.byref(desc) if desc is not None else None, bounds, 0, f.nm, C.byref(s), status, rt._stream_ptr())

    bad = capi.VGX_E_INVALID_ARG
    assert call(desc=None) == bad and call(ptr=None) == bad and call(ptr=image.data_ptr() + 2) == bad
    assert call(stride=t.width - 1) == bad and call(width=16385, stride=16385) == bad and call(x0=(1 << 23) + 1) == bad
    assert call(scissor=(C.c_uint32 * 4)(5, 0, 4, 10)) == bad and call(scissor=(C.c_uint32 * 4)(0, 0, 4, t.height + 1)) == bad
    assert call(bounds=image.data_ptr() + 4) == bad and call(status=image.data_ptr() + 1) == bad
    assert lib.vgx_raster(warm_ctx.handle, C.byref(df.desc), None, 0, f.nm, None, None, rt._stream_ptr()) == bad
    d = df.desc
    assert call(desc=capi.CacheDesc(d.pos, d.color, d.idx, d.meshes, 0xFFFFFFFF, f.nv, f.ni)) == capi.VGX_E_RANGE
    # valid, writing nothing: an empty scissor, no meshes, no status word
    assert call(ptr=None, scissor=(C.c_uint32 * 4)(7, 7, 7, 20), flags=capi.RASTER_CLEAR) == capi.VGX_OK
    assert call(desc=capi.CacheDesc(None, None, None, None, 0, 0, 0)) == capi.VGX_OK
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().view(np.uint32), t.background())


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_raster of another stream -> vgx_tessellate_emit gives the meshes it gives without the raster call."""
    f = R.frame("stack")
    df = dev_frame(f)
    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, lambda: rt.raster(gpu_ctx, df.desc, f.target.width, f.target.height, clear_color=CLEAR),
                                   R.expected("stack", True))
