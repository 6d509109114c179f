"""GPU: vgx_raster_painted (csrc/vgx_raster.hip: the frame family k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, PAINT> at
the painted level) against the numpy statement
(tests/raster_painted_model.py) on its frames, against the six checks of tests/raster_harness.py that do not rest on that
model (run here through the kernels, with the GPU's own vgx_raster_textured where they compare against it), the statuses and the
VGX_E_GROWN protocol, and end to end from command-list bytes: vgx_cmdlist_decode -> vgx_paint_tables -> the tessellator on the device
-> vgx_raster_painted. Every comparison is np.array_equal on the whole uint32 buffer: the stride padding and everything outside the
scissor included."""
import ctypes as C

import numpy as np
import pytest

import raster_harness as H
import raster_model as R
import raster_painted_model as P
import raster_textured_model as T
from raster_harness import DevFrame, DevPaints, DevRunner, DevState, DevTex, gpu_bounds, rt, warm_ctx, where  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = P.CLEAR
BAD = capi.VGX_E_INVALID_ARG


@pytest.fixture(scope="module")
def run(rt, warm_ctx):
    return DevRunner(rt, warm_ctx)


@pytest.mark.parametrize("name", [n for n in P.NAMES if n != "decoded"])
def test_kernels_equal_model(rt, warm_ctx, name):
    """Clear and no clear, with and without mesh_bounds, twice with the same bytes, inputs unchanged."""
    P.check_conditions(name, rt)
    f = P.frame(name, rt)
    df, ds, dx, dp = DevFrame(f), DevState(f), DevTex(f), DevPaints(f.gradients, f.patterns)
    mb = gpu_bounds(rt, warm_ctx, df)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = P.expected(name, clear, rt)
        _, own = H.gpu_level(rt, warm_ctx, "painted", df, ds, dx, dp, tgt)
        assert np.array_equal(own, want), where(own, want)
        assert R.guards_intact(tgt, own)
        _, given = H.gpu_level(rt, warm_ctx, "painted", df, ds, dx, dp, tgt, bounds=mb)
        assert np.array_equal(given, want), where(given, want)
        _, again = H.gpu_level(rt, warm_ctx, "painted", df, ds, dx, dp, tgt)
        assert np.array_equal(again, own)  # two runs, the same bytes
    assert df.unchanged() and dp.unchanged()


def test_decoded_end_to_end_on_the_device(rt, warm_ctx):
    """Command-list bytes -> vgx_cmdlist_decode -> vgx_paint_tables -> the tessellator on the device -> vgx_raster_painted: the model's
    image of the same decode tessellated by the CPU oracle, also through the runtime wrapper."""
    import torch
    P.check_conditions("decoded", rt)
    f = P.frame("decoded", rt)
    g, p = rt.paint_tables(f.paints)
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
    ds, dx, dp = DevState(f), DevTex(f), DevPaints(g, p)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = P.expected("decoded", clear, rt)
        _, got = H.gpu_level(rt, warm_ctx, "painted", Dev, ds, dx, dp, tgt)
        assert np.array_equal(got, want), where(got, want)
        assert R.guards_intact(tgt, got)
    img, status = rt.raster_painted(warm_ctx, Dev.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], 8, dx.t[1], len(f.images), dp.t[0], len(g), dp.t[1], len(p),
                                    f.target.width, f.target.height, clear_color=CLEAR)
    torch.cuda.synchronize()
    t = f.target
    want = P.render(f, R.Target(t.width, t.height, t.width, 0, 0, clear=CLEAR), np.zeros((t.height, t.width), dtype=np.uint32))
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), want)


# ---- the checks that do not rest on the model -------------------------------------------------------------------------------
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


# ---- protocol ---------------------------------------------------------------------------------------------------------------
def big_frame():
    return H.big_frame(P.frame("crowd"))


def test_fresh_context_grows_then_succeeds(rt):
    """The VGX_E_GROWN protocol: a fresh context's first call writes NOTHING, the clear included, the repeat succeeds; after
    vgx_raster_reserve one call is enough, and vgx_scratch_bytes counts the tile bits only this call allocates."""
    f = big_frame()
    tgt = f.target.with_clear(CLEAR)
    want = P.render(f, tgt, tgt.background())
    assert not np.array_equal(want, T.render(P.as_flat(f), tgt, tgt.background()))
    df, ds, dx, dp = DevFrame(f), DevState(f), DevTex(f), DevPaints(f.gradients, f.patterns)
    flat = P.as_flat(f)
    textured = lambda ctx, tgt: H.gpu_level(rt, ctx, "textured", DevFrame(flat), DevState(flat), dx, tgt=tgt)  # everything vgx_raster_textured allocates
    H.check_fresh_context_grows_then_succeeds(rt, lambda ctx, tgt, **kw: H.gpu_level(rt, ctx, "painted", df, ds, dx, dp, tgt, **kw), f, lambda tgt: want,
                                              R.bin_entries(T.as_fill(f), tgt), prepare=textured, min_growth=4)  # one word of tile bits for 4 x 4 tiles


def test_invalid_paint_writes_nothing(rt, warm_ctx, run):
    """Each invalid case ends with VGX_E_INVALID_ARG and not one pixel or guard word changed, the clear included; entries no painted
    mesh of the range names may be garbage; the status ranks above VGX_E_GROWN."""
    f = P.frame("state")
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for what, kw in H.invalid_cases(f):
            got = run.painted(f, tgt, want=BAD, **kw)
            assert np.array_equal(got, tgt.background()), what
    junk_g = f.gradients.copy()
    junk_g[0] = np.frombuffer(bytes(range(96)), dtype=capi.paint_dtype)[0]
    junk_p = np.frombuffer(bytes(range(7, 103)), dtype=capi.paint_dtype).copy()
    got = run.painted(f, f.target, gradients=junk_g, patterns=junk_p, end=4)
    assert np.array_equal(got, P.render(f, f.target, f.target.background(), mesh_end=4))
    g = big_frame()
    ctx = rt.Context(0)
    try:
        tgt = g.target.with_clear(CLEAR)
        got = DevRunner(rt, ctx).painted(g, tgt, gradients=g.gradients[:1], want=BAD)
        assert np.array_equal(got, tgt.background())
    finally:
        ctx.close()


def test_mesh_range_and_split_calls(rt, warm_ctx):
    f = P.frame("crowd")
    df, ds, dx, dp = DevFrame(f), DevState(f), DevTex(f), DevPaints(f.gradients, f.patterns)
    img, got = H.gpu_level(rt, warm_ctx, "painted", df, ds, dx, dp, f.target, end=150)
    assert np.array_equal(got, P.render(f, f.target, f.target.background(), mesh_end=150))
    _, got = H.gpu_level(rt, warm_ctx, "painted", df, ds, dx, dp, f.target, image=img, begin=150)
    assert np.array_equal(got, P.expected("crowd"))


def test_refused_calls(rt, warm_ctx):
    import torch
    f = P.frame("state")
    df, ds, dx, dp = DevFrame(f), DevState(f), DevTex(f), DevPaints(f.gradients, f.patterns)
    t = f.target
    image = torch.from_numpy(t.background().view(np.int32)).to("cuda:0")
    lib = rt.lib()
    gp, pp = dp.t[0].data_ptr(), dp.t[1].data_ptr()

    def call(paints, tex=True):
        s = t.struct(image.data_ptr())
        return lib.vgx_raster_painted(warm_ctx.handle, C.byref(df.desc), None, 0, f.nm, C.byref(ds.struct), C.byref(dx.struct) if tex else None,
                                      None if paints is None else C.byref(paints), C.byref(s), None, rt._stream_ptr())

    assert call(None) == BAD and call(dp.struct, tex=False) == BAD
    assert call(capi.RasterPaints(None, pp, 2, 1)) == BAD and call(capi.RasterPaints(gp, None, 2, 1)) == BAD
    assert call(capi.RasterPaints(gp + 2, pp, 2, 1)) == BAD and call(capi.RasterPaints(gp, pp + 1, 2, 1)) == BAD
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().view(np.uint32), t.background())
    assert call(capi.RasterPaints(gp, pp, 2, 1)) == capi.VGX_OK
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().view(np.uint32), P.expected("state"))


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_raster_painted of another stream -> vgx_tessellate_emit gives the meshes it gives without the call."""
    f = P.frame("crowd")
    df, ds, dx, dp = DevFrame(f), DevState(f), DevTex(f), DevPaints(f.gradients, f.patterns)
    call = lambda: rt.raster_painted(gpu_ctx, df.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], T.uv_bytes(f), dx.t[1], len(f.images),
                                     dp.t[0], len(f.gradients), dp.t[1], len(f.patterns), f.target.width, f.target.height, clear_color=CLEAR)
    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, call, P.expected("crowd", True))
