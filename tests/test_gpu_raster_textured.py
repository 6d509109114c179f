"""GPU: vgx_raster_textured (csrc/vgx_raster.hip: the frame family k_rasterf_count / k_rasterf_entries / k_rasterf_tiles<TEX, false> at
the textured level) against the numpy statement
(tests/raster_textured_model.py) on its frames, against the GPU's own vgx_raster_frame where the images are white or no mesh is
sampled, and end to end from command-list bytes: vgx_text_quads -> vgx_merge_uv_stream -> vgx_raster_textured. Every comparison is
np.array_equal on the whole uint32 buffer: the stride padding and everything outside the scissor included."""
import ctypes as C

import numpy as np
import pytest

import raster_frame_model as M
import raster_harness as H
import raster_model as R
import raster_textured_model as T
from raster_harness import DevFrame, DevState, DevTex, gpu_bounds, rt, to_dev, warm_ctx, where  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = T.CLEAR


@pytest.mark.parametrize("name", T.NAMES + ("decoded",))
def test_kernels_equal_model(rt, warm_ctx, name):
    """Clear and no clear, with and without mesh_bounds, twice with the same bytes, inputs unchanged."""
    T.check_conditions(name, rt)
    f = T.frame(name, rt)
    df, ds, dx = DevFrame(f), DevState(f), DevTex(f)
    mb = gpu_bounds(rt, warm_ctx, df)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = T.expected(name, clear, rt)
        _, own = H.gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt)
        assert np.array_equal(own, want), where(own, want)
        assert R.guards_intact(tgt, own)
        _, given = H.gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt, bounds=mb)
        assert np.array_equal(given, want), where(given, want)
        _, again = H.gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt)
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
                ch = [H.div255(((s >> (8 * k)) & 255) * a + ((CLEAR >> (8 * k)) & 255) * (255 - a)) for k in range(3)]
                want[2 + y, 3 + x] = ch[0] | (ch[1] << 8) | (ch[2] << 16) | (H.div255(255 * a + (CLEAR >> 24) * (255 - a)) << 24)
    _, got = H.gpu_level(rt, warm_ctx, "textured", DevFrame(f), DevState(f), DevTex(f), tgt=tgt)
    assert np.array_equal(got, want), where(got, want)


@pytest.mark.parametrize("name", ("blit_linear", "wrap_f_l_00", "wrap_i_n_11", "seam", "crowd", "state", "decoded"))
def test_white_images_give_vgx_raster_frame(rt, warm_ctx, name):
    """(ii) every image all 0xFFFFFFFF: the GPU's vgx_raster_frame of the same streams with the kinds TEXT / TRILIST rewritten to FILL_AA."""
    f = T.frame(name, rt)
    g = T.as_fill(f)
    ds = DevState(f)
    dx = DevTex(f, images=[im.white() for im in f.images])
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        _, got = H.gpu_level(rt, warm_ctx, "textured", DevFrame(f), ds, dx, tgt=tgt)
        _, want = H.gpu_level(rt, warm_ctx, "frame", DevFrame(g), ds, tgt=tgt)
        assert np.array_equal(got, want), where(got, want)
        assert not np.array_equal(got, T.expected(name, tgt.clear is not None, rt))


@pytest.mark.parametrize("name", M.NAMES)
def test_no_sampled_mesh_equals_vgx_raster_frame(rt, warm_ctx, name):
    """(iii) raster_frame_model's frames through the new call, with no image at all and a UV stream of NaNs nobody reads."""
    f = M.frame(name)
    df, ds = DevFrame(f), DevState(f)
    dx = DevTex(f, images=[], uv=np.full((max(f.nv, 1), 2), np.nan, dtype=np.float32))
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        _, got = H.gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt)
        _, want = H.gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt)
        assert np.array_equal(got, want), where(got, want)
        assert np.array_equal(got, M.expected(name, tgt.clear is not None))


def big_frame():
    return H.big_frame(T.frame("crowd"))


def test_fresh_context_grows_then_succeeds(rt):
    """The VGX_E_GROWN protocol: a fresh context's first call writes NOTHING, the clear included, the repeat succeeds; after
    vgx_raster_reserve one call is enough."""
    f = big_frame()
    df, ds, dx = DevFrame(f), DevState(f), DevTex(f)
    H.check_fresh_context_grows_then_succeeds(rt, lambda ctx, tgt, **kw: H.gpu_level(rt, ctx, "textured", df, ds, dx, tgt=tgt, **kw), f,
                                              lambda tgt: T.render(f, tgt, tgt.background()), R.bin_entries(T.as_fill(f), f.target.with_clear(CLEAR)))


def test_invalid_image_writes_nothing(rt, warm_ctx):
    """VGX_E_INVALID_ARG writes nothing, the clear included; a bad image nobody samples is not looked at; the status ranks above
    VGX_E_GROWN."""
    f = T.frame("state")
    df, ds = DevFrame(f), DevState(f)
    rec = H.image_records(f.images)
    rec["stride"][1] = rec["width"][1] - 1
    bad = DevTex(f, records=rec)
    one = DevTex(f, images=f.images[:1])
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for dx in (bad, one):
            _, got = H.gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt, want=capi.VGX_E_INVALID_ARG)
            assert np.array_equal(got, tgt.background())
    _, got = H.gpu_level(rt, warm_ctx, "textured", df, ds, bad, tgt=f.target, begin=5)  # only the paint draw's mesh names image 1 there
    assert np.array_equal(got, T.render(f, f.target, f.target.background(), mesh_begin=5))
    g = big_frame()
    ctx = rt.Context(0)
    try:
        tgt = g.target.with_clear(CLEAR)
        _, got = H.gpu_level(rt, ctx, "textured", DevFrame(g), DevState(g), DevTex(g, images=g.images[:1]), tgt=tgt, want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
    finally:
        ctx.close()


def test_refused_calls(rt, warm_ctx):
    import torch
    f = T.frame("state")
    df, ds, dx = DevFrame(f), DevState(f), DevTex(f)
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
    f = T.frame("crowd")
    df, ds, dx = DevFrame(f), DevState(f), DevTex(f)
    call = lambda: rt.raster_textured(gpu_ctx, df.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], T.uv_bytes(f), dx.t[1], len(f.images),
                                      f.target.width, f.target.height, clear_color=CLEAR)
    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, call, T.expected("crowd", True))


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
    tb = [to_dev(ext[k]) for k in ("pos", "color", "idx", "meshes")]
    seq_b = capi.CacheDesc(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3].data_ptr(), ext["meshes"].shape[0], ext["pos"].shape[0], ext["idx"].shape[0])
    b_uv = to_dev(ext["uv"])
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
    ds = DevState(f)
    dx = DevTex(f)
    dx.struct.uv = out_uv[guard:].data_ptr()
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        _, got = H.gpu_level(rt, warm_ctx, "textured", Dev, ds, dx, tgt=tgt)
        want = T.expected("decoded", clear, rt)
        assert np.array_equal(got, want), where(got, want)
        assert R.guards_intact(tgt, got)
