"""GPU: vgx_raster_textured (csrc/vgx_raster.hip: the frame family k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, false> at
the textured level) against the numpy statement
(tests/raster_textured_model.py) on its frames, against the GPU's own vgx_raster_frame where the images are white or no mesh is
sampled, and end to end from command-list bytes: vgx_text_quads -> vgx_merge_uv_stream -> vgx_raster_textured. Every comparison is
np.array_equal on the whole uint32 buffer: the stride padding and everything outside the scissor included."""
import ctypes as C
import importlib

import numpy as np
import pytest

import raster_frame_model as M
import raster_model as R
import raster_textured_model as T
import test_gpu_raster as G
import test_gpu_raster_frame as GF
import test_raster_textured_cpu as cpu

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = T.CLEAR


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def warm_ctx(rt):
    ctx = rt.Context(0)
    rt.raster_reserve(ctx, 8192, 1 << 17)
    yield ctx
    ctx.close()


class DevTex:
    """The UV stream and the images of a frame in device memory. images / records: instead of the frame's."""

    def __init__(self, f, images=None, records=None, uv=None):
        images = f.images if images is None else images
        uv = f.uv if uv is None else uv
        self.px = [G.to_dev(im.pixels) for im in images]
        rec = cpu.image_records(images) if records is None else records.copy()
        for k in range(len(images)):
            rec["pixels"][k] = self.px[k].data_ptr() + (int(rec["pixels"][k]) - images[k].pixels.ctypes.data if records is not None else 0)
        self.uv_host = uv
        self.t = [G.to_dev(uv), G.to_dev(rec)]
        self.struct = capi.RasterTextures(self.t[0].data_ptr(), self.t[1].data_ptr() if len(images) else None, 8 if uv.dtype == np.float32 else 4, len(images))

    def unchanged(self):
        return np.array_equal(self.t[0].cpu().numpy()[:self.uv_host.nbytes], self.uv_host.view(np.uint8).reshape(-1))


def gpu_textured(rt, ctx, df, ds, dx, tgt, image=None, bounds=None, begin=0, end=2**64 - 1, want=capi.VGX_OK):
    """One vgx_raster_textured call over the target's background (or `image`, a device tensor, changed in place), synchronised; returns
    (image tensor, image as uint32 [rows, stride])."""
    import torch
    if image is None:
        image = torch.from_numpy(tgt.background().view(np.int32)).to("cuda:0")
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
    t = tgt.struct(image.data_ptr())
    st = rt.lib().vgx_raster_textured(ctx.handle, C.byref(df.desc), None if bounds is None else bounds.data_ptr(), begin, end, C.byref(ds.struct),
                                      C.byref(dx.struct), C.byref(t), status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == capi.VGX_OK
    assert status.cpu().tolist() == [want, 77, 77]
    return image, image.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", T.NAMES + ("decoded",))
def test_kernels_equal_model(rt, warm_ctx, name):
    """Clear and no clear, with and without mesh_bounds, twice with the same bytes, inputs unchanged."""
    T.check_conditions(name, rt)
    f = T.frame(name, rt)
    df, ds, dx = G.DevFrame(f), GF.DevState(f), DevTex(f)
    mb = G.gpu_bounds(rt, warm_ctx, df)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = T.expected(name, clear, rt)
        _, own = gpu_textured(rt, warm_ctx, df, ds, dx, tgt)
        assert np.array_equal(own, want), G.where(own, want)
        assert R.guards_intact(tgt, own)
        _, given = gpu_textured(rt, warm_ctx, df, ds, dx, tgt, bounds=mb)
        assert np.array_equal(given, want), G.where(given, want)
        _, again = gpu_textured(rt, warm_ctx, df, ds, dx, tgt)
        assert np.array_equal(again, own)  # two runs, the same bytes
    assert df.unchanged() and dx.unchanged()


@pytest.mark.parametrize("name", ["blit_nearest", "blit_linear"])
def test_blit_is_the_clear_blended_with_the_texels(rt, warm_ctx, name):
    """(i) as tests/test_raster_textured_cpu.py computes it, from div255 alone."""
    f = T.frame(name)
    tgt = f.target.with_clear(CLEAR)
    want = tgt.background()
    want[:, :tgt.width] = CLEAR
    for y in range(3):
        for x in range(5):
            s = int(f.images[0].pixels[y, x])
            a = s >> 24
            if a:
                ch = [cpu.div255(((s >> (8 * k)) & 255) * a + ((CLEAR >> (8 * k)) & 255) * (255 - a)) for k in range(3)]
                want[2 + y, 3 + x] = ch[0] | (ch[1] << 8) | (ch[2] << 16) | (cpu.div255(255 * a + (CLEAR >> 24) * (255 - a)) << 24)
    _, got = gpu_textured(rt, warm_ctx, G.DevFrame(f), GF.DevState(f), DevTex(f), tgt)
    assert np.array_equal(got, want), G.where(got, want)


@pytest.mark.parametrize("name", ("blit_linear", "wrap_f_l_00", "wrap_i_n_11", "seam", "crowd", "state", "decoded"))
def test_white_images_give_vgx_raster_frame(rt, warm_ctx, name):
    """(ii) every image all 0xFFFFFFFF: the GPU's vgx_raster_frame of the same streams with the kinds TEXT / TRILIST rewritten to FILL_AA."""
    f = T.frame(name, rt)
    g = T.as_fill(f)
    ds = GF.DevState(f)
    dx = DevTex(f, images=[im.white() for im in f.images])
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        _, got = gpu_textured(rt, warm_ctx, G.DevFrame(f), ds, dx, tgt)
        _, want = GF.gpu_frame(rt, warm_ctx, G.DevFrame(g), ds, tgt)
        assert np.array_equal(got, want), G.where(got, want)
        assert not np.array_equal(got, T.expected(name, tgt.clear is not None, rt))


@pytest.mark.parametrize("name", M.NAMES)
def test_no_sampled_mesh_equals_vgx_raster_frame(rt, warm_ctx, name):
    """(iii) raster_frame_model's frames through the new call, with no image at all and a UV stream of NaNs nobody reads."""
    f = M.frame(name)
    df, ds = G.DevFrame(f), GF.DevState(f)
    dx = DevTex(f, images=[], uv=np.full((max(f.nv, 1), 2), np.nan, dtype=np.float32))
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        _, got = gpu_textured(rt, warm_ctx, df, ds, dx, tgt)
        _, want = GF.gpu_frame(rt, warm_ctx, df, ds, tgt)
        assert np.array_equal(got, want), G.where(got, want)
        assert np.array_equal(got, M.expected(name, tgt.clear is not None))


def big_frame():
    """`crowd` magnified four times, its one tile now the 4 x 4 tiles of a 64 x 64 image: every mesh reaches several tiles, more bin
    entries than a fresh context's first guess of one entry per mesh holds."""
    f = T.frame("crowd")
    scale = np.float32(4.0)
    g = R.make("crowd_x4", (f.pos - np.float32(16.0)) * scale, f.color, f.idx, f.meshes, R.Target(64, 64, 64, 0, 0))
    g.draws, g.dstate, g.uv, g.images = f.draws, f.dstate, f.uv, f.images
    return g


def test_fresh_context_grows_then_succeeds(rt):
    """The VGX_E_GROWN protocol: a fresh context's first call writes NOTHING, the clear included, the repeat succeeds; after
    vgx_raster_reserve one call is enough."""
    f = big_frame()
    tgt = f.target.with_clear(CLEAR)
    want = T.render(f, tgt, tgt.background())
    df, ds, dx = G.DevFrame(f), GF.DevState(f), DevTex(f)
    entries = R.bin_entries(T.as_fill(f), tgt)
    assert entries > 2 * f.nm + 64, (entries, f.nm)  # condition on the input: the first guess cannot hold them
    ctx = rt.Context(0)
    try:
        img, got = gpu_textured(rt, ctx, df, ds, dx, tgt, want=capi.VGX_E_GROWN)
        assert np.array_equal(got, tgt.background())
        _, got = gpu_textured(rt, ctx, df, ds, dx, tgt, image=img)
        assert np.array_equal(got, want), G.where(got, want)
    finally:
        ctx.close()
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, f.nm, entries)
        _, got = gpu_textured(rt, ctx, df, ds, dx, tgt)
        assert np.array_equal(got, want)
    finally:
        ctx.close()


def test_invalid_image_writes_nothing(rt, warm_ctx):
    """VGX_E_INVALID_ARG writes nothing, the clear included; a bad image nobody samples is not looked at; the status ranks above
    VGX_E_GROWN."""
    f = T.frame("state")
    df, ds = G.DevFrame(f), GF.DevState(f)
    rec = cpu.image_records(f.images)
    rec["stride"][1] = rec["width"][1] - 1
    bad = DevTex(f, records=rec)
    one = DevTex(f, images=f.images[:1])
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for dx in (bad, one):
            _, got = gpu_textured(rt, warm_ctx, df, ds, dx, tgt, want=capi.VGX_E_INVALID_ARG)
            assert np.array_equal(got, tgt.background())
    _, got = gpu_textured(rt, warm_ctx, df, ds, bad, f.target, begin=5)  # only the paint draw's mesh names image 1 there
    assert np.array_equal(got, T.render(f, f.target, f.target.background(), mesh_begin=5))
    g = big_frame()
    ctx = rt.Context(0)
    try:
        tgt = g.target.with_clear(CLEAR)
        _, got = gpu_textured(rt, ctx, G.DevFrame(g), GF.DevState(g), DevTex(g, images=g.images[:1]), tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
    finally:
        ctx.close()


def test_refused_calls(rt, warm_ctx):
    import torch
    f = T.frame("state")
    df, ds, dx = G.DevFrame(f), GF.DevState(f), DevTex(f)
    t = f.target
    image = torch.from_numpy(t.background().view(np.int32)).to("cuda:0")
    lib = rt.lib()
    uvp, recp = dx.t[0].data_ptr(), dx.t[1].data_ptr()

    def call(tex=None, no_tex=False, begin=0):
        s = t.struct(image.data_ptr())
        return lib.vgx_raster_textured(warm_ctx.handle, C.byref(df.desc), None, begin, f.nm, C.byref(ds.struct), None if no_tex else C.byref(dx.struct if tex is None else tex),
                                       C.byref(s), None, rt._stream_ptr())

    bad = capi.VGX_E_INVALID_ARG
    assert call(no_tex=True) == bad
    assert call(capi.RasterTextures(uvp, recp, 0, 2)) == bad and call(capi.RasterTextures(uvp, recp, 6, 2)) == bad
    assert call(capi.RasterTextures(None, recp, 8, 2)) == bad and call(capi.RasterTextures(uvp + 4, recp, 8, 2)) == bad
    assert call(capi.RasterTextures(uvp, None, 8, 2)) == bad and call(capi.RasterTextures(uvp, recp + 4, 8, 2)) == bad
    assert call(capi.RasterTextures(None, recp, 8, 2), begin=f.nm) == capi.VGX_OK  # an empty range needs no UV stream
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().view(np.uint32), t.background())


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_raster_textured of another stream -> vgx_tessellate_emit gives the meshes it gives without the call."""
    import torch
    f = T.frame("crowd")
    df, ds, dx = G.DevFrame(f), GF.DevState(f), DevTex(f)
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    for _ in range(2):  # the first call of this context may end with VGX_E_GROWN; either way the counted state must survive
        img, status = rt.raster_textured(gpu_ctx, df.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], T.uv_bytes(f), dx.t[1], len(f.images),
                                         f.target.width, f.target.height, clear_color=CLEAR)
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
    assert np.array_equal(img.cpu().numpy().view(np.uint32), T.expected("crowd", True))


def test_decoded_end_to_end_on_the_device(rt, warm_ctx):
    """Command-list bytes -> vgx_cmdlist_decode_text -> the tessellator on the device; the text runs by vgx_text_quads at their places
    in the external sequence beside the user mesh; vgx_merge_uv_stream; vgx_raster_textured: the model's image. The merged UV stream
    holds the external sequence's UVs at the vertices of its meshes and the fill pattern everywhere else."""
    import torch
    import text_frame as TF
    T.check_conditions("decoded", rt)
    f = T.frame("decoded", rt)
    A, ext, draws, dstate, ps, runs = T.decoded_parts(rt, TF.gpu_text_fn(rt, warm_ctx))
    host_ext = T.decoded_parts(rt)[1]
    for k in ("pos", "color", "uv", "idx"):
        assert np.array_equal(np.asarray(ext[k]).view(np.uint8), np.asarray(host_ext[k]).view(np.uint8)), k  # vgx_text_quads == its lane code
    assert runs.shape[0] >= 2
    dev = torch.device("cuda", 0)
    pset = rt.PathSet(warm_ctx, ps)
    dd = rt.upload_draws(draws)
    sizes = rt.tessellate_count(warm_ctx, pset, dd, draws.shape[0])
    a = rt.MeshBuffers(dev, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(warm_ctx, pset, dd, draws.shape[0], a)
    torch.cuda.synchronize()
    pset.close()
    seq_a = rt.mesh_seq(a, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    tb = [G.to_dev(ext[k]) for k in ("pos", "color", "idx", "meshes")]
    seq_b = capi.CacheDesc(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3].data_ptr(), ext["meshes"].shape[0], ext["pos"].shape[0], ext["idx"].shape[0])
    b_uv = G.to_dev(ext["uv"])
    guard = 16
    out = rt.MeshBuffers(dev, f.nv, f.ni, f.nm)
    out_uv = torch.full((f.nv + 2 * guard, 2), T.UV_GUARD | (T.UV_GUARD << 8), dtype=torch.int16, device=dev)
    rt.merge_uv_stream(warm_ctx, seq_a, seq_b, None, b_uv, 4, dd, draws.shape[0], out, out_uv[guard:])
    torch.cuda.synchronize()
    assert int(out.dev_status.item()) == capi.VGX_OK
    got_uv = out_uv.cpu().numpy()
    assert np.array_equal(got_uv[guard:guard + f.nv], f.uv)  # b's UVs at b's vertices, the pattern at a's: the model's merge
    assert np.all(got_uv[:guard].view(np.uint8) == T.UV_GUARD) and np.all(got_uv[guard + f.nv:].view(np.uint8) == T.UV_GUARD)
    assert np.array_equal(out.pos[:f.nv].cpu().numpy().view(np.uint32), f.pos.view(np.uint32))
    assert np.array_equal(out.idx[:f.ni].cpu().numpy().view(np.uint16), f.idx)

    class Dev:
        desc = capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), f.nm, f.nv, f.ni)
    ds = GF.DevState(f)
    dx = DevTex(f)
    dx.struct.uv = out_uv[guard:].data_ptr()
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        _, got = gpu_textured(rt, warm_ctx, Dev, ds, dx, tgt)
        want = T.expected("decoded", clear, rt)
        assert np.array_equal(got, want), G.where(got, want)
        assert R.guards_intact(tgt, got)
