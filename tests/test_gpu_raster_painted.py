"""GPU: vgx_raster_painted (csrc/vgx_raster.hip: the frame family k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, PAINT> at
the painted level) against the numpy statement
(tests/raster_painted_model.py) on its frames, against the six checks of tests/test_raster_painted_cpu.py that do not rest on that
model (run here through the kernels, with the GPU's own vgx_raster_textured where they compare against it), the statuses and the
VGX_E_GROWN protocol, and end to end from command-list bytes: vgx_cmdlist_decode -> vgx_paint_tables -> the tessellator on the device
-> vgx_raster_painted. Every comparison is np.array_equal on the whole uint32 buffer: the stride padding and everything outside the
scissor included."""
import ctypes as C
import importlib

import numpy as np
import pytest

import raster_model as R
import raster_painted_model as P
import raster_textured_model as T
import test_gpu_raster as G
import test_gpu_raster_frame as GF
import test_gpu_raster_textured as GT
import test_raster_painted_cpu as cpu
import test_raster_textured_cpu as tcpu

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = P.CLEAR
BAD = capi.VGX_E_INVALID_ARG


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def warm_ctx(rt):
    ctx = rt.Context(0)
    rt.raster_reserve(ctx, 8192, 1 << 17)
    yield ctx
    ctx.close()


class DevPaints:
    """The two paint tables in device memory."""

    def __init__(self, gradients, patterns):
        self.host = [np.ascontiguousarray(gradients), np.ascontiguousarray(patterns)]
        self.t = [G.to_dev(a) for a in self.host]
        ng, npat = len(gradients), len(patterns)
        self.struct = capi.RasterPaints(self.t[0].data_ptr() if ng else None, self.t[1].data_ptr() if npat else None, ng, npat)

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy()[:h.nbytes], h.view(np.uint8).reshape(-1)) for t, h in zip(self.t, self.host))


def gpu_painted(rt, ctx, df, ds, dx, dp, tgt, image=None, bounds=None, begin=0, end=2**64 - 1, want=capi.VGX_OK):
    """One vgx_raster_painted call over the target's background (or `image`, a device tensor, changed in place), synchronised; returns
    (image tensor, image as uint32 [rows, stride])."""
    import torch
    if image is None:
        image = torch.from_numpy(tgt.background().view(np.int32)).to("cuda:0")
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
    t = tgt.struct(image.data_ptr())
    st = rt.lib().vgx_raster_painted(ctx.handle, C.byref(df.desc), None if bounds is None else bounds.data_ptr(), begin, end, C.byref(ds.struct),
                                     C.byref(dx.struct), C.byref(dp.struct), C.byref(t), status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == capi.VGX_OK
    assert status.cpu().tolist() == [want, 77, 77]
    return image, image.cpu().numpy().view(np.uint32)


class DevRunner:
    """The runner of the model-independent checks over the kernels (tests/test_raster_painted_cpu.py: HostRunner)."""

    def __init__(self, rt, ctx):
        self.rt, self.ctx = rt, ctx

    def painted(self, f, tgt, images=None, gradients=None, patterns=None, records=None, begin=0, end=2**64 - 1, want=capi.VGX_OK):
        dx = GT.DevTex(f, images=images, records=records)
        dp = DevPaints(f.gradients if gradients is None else gradients, f.patterns if patterns is None else patterns)
        return gpu_painted(self.rt, self.ctx, G.DevFrame(f), GF.DevState(f), dx, dp, tgt, begin=begin, end=end, want=want)[1]

    def textured(self, f, tgt, end=2**64 - 1, want=capi.VGX_OK):
        return GT.gpu_textured(self.rt, self.ctx, G.DevFrame(f), GF.DevState(f), GT.DevTex(f), tgt, end=end, want=want)[1]


@pytest.fixture(scope="module")
def run(rt, warm_ctx):
    return DevRunner(rt, warm_ctx)


@pytest.mark.parametrize("name", [n for n in P.NAMES if n != "decoded"])
def test_kernels_equal_model(rt, warm_ctx, name):
    """Clear and no clear, with and without mesh_bounds, twice with the same bytes, inputs unchanged."""
    P.check_conditions(name, rt)
    f = P.frame(name, rt)
    df, ds, dx, dp = G.DevFrame(f), GF.DevState(f), GT.DevTex(f), DevPaints(f.gradients, f.patterns)
    mb = G.gpu_bounds(rt, warm_ctx, df)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = P.expected(name, clear, rt)
        _, own = gpu_painted(rt, warm_ctx, df, ds, dx, dp, tgt)
        assert np.array_equal(own, want), G.where(own, want)
        assert R.guards_intact(tgt, own)
        _, given = gpu_painted(rt, warm_ctx, df, ds, dx, dp, tgt, bounds=mb)
        assert np.array_equal(given, want), G.where(given, want)
        _, again = gpu_painted(rt, warm_ctx, df, ds, dx, dp, tgt)
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
    ds, dx, dp = GF.DevState(f), GT.DevTex(f), DevPaints(g, p)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = P.expected("decoded", clear, rt)
        _, got = gpu_painted(rt, warm_ctx, Dev, ds, dx, dp, tgt)
        assert np.array_equal(got, want), G.where(got, want)
        assert R.guards_intact(tgt, got)
    img, status = rt.raster_painted(warm_ctx, Dev.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], 8, dx.t[1], len(f.images), dp.t[0], len(g), dp.t[1], len(p),
                                    f.target.width, f.target.height, clear_color=CLEAR)
    torch.cuda.synchronize()
    t = f.target
    want = P.render(f, R.Target(t.width, t.height, t.width, 0, 0, clear=CLEAR), np.zeros((t.height, t.width), dtype=np.uint32))
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), want)


# ---- the checks that do not rest on the model -------------------------------------------------------------------------------
def test_linear_ramp_closed_form(run, rt):
    cpu.check_linear_ramp(run, rt)


def test_radial_distances_closed_form(run, rt):
    cpu.check_radial_distances(run, rt)


def test_one_colour_gradient_equals_textured(run, rt):
    cpu.check_one_colour_gradient(run, rt)


def test_pattern_blit_from_div255(run):
    cpu.check_pattern_blit(run)


def test_pattern_equals_sampled_quad(run):
    cpu.check_pattern_equals_sampled_quad(run)


@pytest.mark.parametrize("name", T.NAMES)
def test_no_painted_draw_equals_textured(run, name):
    cpu.check_no_painted_draw(run, name)


# ---- protocol ---------------------------------------------------------------------------------------------------------------
def big_frame():
    """`crowd` magnified four times, its one tile now the 4 x 4 tiles of a 64 x 64 image: every mesh reaches several tiles, more bin
    entries than a fresh context's first guess of one entry per mesh holds. The paints stay where they are: any valid paint will do."""
    f = P.frame("crowd")
    g = R.make("crowd_x4", (f.pos - np.float32(16.0)) * np.float32(4.0), f.color, f.idx, f.meshes, R.Target(64, 64, 64, 0, 0))
    g.draws, g.dstate, g.uv, g.images, g.gradients, g.patterns = f.draws, f.dstate, f.uv, f.images, f.gradients, f.patterns
    return g


def test_fresh_context_grows_then_succeeds(rt):
    """The VGX_E_GROWN protocol: a fresh context's first call writes NOTHING, the clear included, the repeat succeeds; after
    vgx_raster_reserve one call is enough, and vgx_scratch_bytes counts the tile bits only this call allocates."""
    f = big_frame()
    tgt = f.target.with_clear(CLEAR)
    want = P.render(f, tgt, tgt.background())
    assert not np.array_equal(want, T.render(P.as_flat(f), tgt, tgt.background()))
    df, ds, dx, dp = G.DevFrame(f), GF.DevState(f), GT.DevTex(f), DevPaints(f.gradients, f.patterns)
    entries = R.bin_entries(T.as_fill(f), tgt)
    assert entries > 2 * f.nm + 64, (entries, f.nm)  # condition on the input: the first guess cannot hold them
    ctx = rt.Context(0)
    try:
        img, got = gpu_painted(rt, ctx, df, ds, dx, dp, tgt, want=capi.VGX_E_GROWN)
        assert np.array_equal(got, tgt.background())
        _, got = gpu_painted(rt, ctx, df, ds, dx, dp, tgt, image=img)
        assert np.array_equal(got, want), G.where(got, want)
    finally:
        ctx.close()
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, f.nm, entries)
        flat = P.as_flat(f)
        GT.gpu_textured(rt, ctx, G.DevFrame(flat), GF.DevState(flat), dx, tgt)           # everything vgx_raster_textured allocates
        before = int(rt.lib().vgx_scratch_bytes(ctx.handle))
        _, got = gpu_painted(rt, ctx, df, ds, dx, dp, tgt)
        assert np.array_equal(got, want)
        assert int(rt.lib().vgx_scratch_bytes(ctx.handle)) - before >= 4                   # one word of tile bits for 4 x 4 tiles
    finally:
        ctx.close()


def test_invalid_paint_writes_nothing(rt, warm_ctx, run):
    """Each invalid case ends with VGX_E_INVALID_ARG and not one pixel or guard word changed, the clear included; entries no painted
    mesh of the range names may be garbage; the status ranks above VGX_E_GROWN."""
    f = P.frame("state")
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for what, kw in cpu.invalid_cases(f):
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
    df, ds, dx, dp = G.DevFrame(f), GF.DevState(f), GT.DevTex(f), DevPaints(f.gradients, f.patterns)
    img, got = gpu_painted(rt, warm_ctx, df, ds, dx, dp, f.target, end=150)
    assert np.array_equal(got, P.render(f, f.target, f.target.background(), mesh_end=150))
    _, got = gpu_painted(rt, warm_ctx, df, ds, dx, dp, f.target, image=img, begin=150)
    assert np.array_equal(got, P.expected("crowd"))


def test_refused_calls(rt, warm_ctx):
    import torch
    f = P.frame("state")
    df, ds, dx, dp = G.DevFrame(f), GF.DevState(f), GT.DevTex(f), DevPaints(f.gradients, f.patterns)
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
    import torch
    f = P.frame("crowd")
    df, ds, dx, dp = G.DevFrame(f), GF.DevState(f), GT.DevTex(f), DevPaints(f.gradients, f.patterns)
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    for _ in range(2):  # the first call of this context may end with VGX_E_GROWN; either way the counted state must survive
        img, status = rt.raster_painted(gpu_ctx, df.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], T.uv_bytes(f), dx.t[1], len(f.images),
                                        dp.t[0], len(f.gradients), dp.t[1], len(f.patterns), f.target.width, f.target.height, clear_color=CLEAR)
        torch.cuda.synchronize()
    assert int(status.item()) == capi.VGX_OK
    bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(gpu_ctx, pset, dd, d.shape[0], bufs)
    torch.cuda.synchronize()
    pset.close()
    nv, ni, nm = ref.sizes["num_vertices"], ref.sizes["num_indices"], ref.sizes["num_meshes"]
    assert (sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]) == (nv, ni, nm)
    assert np.array_equal(bufs.pos[:nv].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
    assert np.array_equal(bufs.color[:nv].cpu().numpy().view(np.uint32), ref.color)
    assert np.array_equal(bufs.idx[:ni].cpu().numpy().view(np.uint16), ref.idx)
    gm = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    for name in ref.meshes.dtype.names:
        assert np.array_equal(gm[name], ref.meshes[name]), name
    assert np.array_equal(img.cpu().numpy().view(np.uint32), P.expected("crowd", True))
