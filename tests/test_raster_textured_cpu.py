"""CPU: the lane code of vgx_raster_textured (csrc/vgx_raster.h through libvgx_hosttest.so: vgxt_raster_textured, the host loop of
the frame-level calls at the textured level) against the numpy statement (tests/raster_textured_model.py), and against three things that do
not rest on that model: a blit computed here from div255, vgxt_raster_frame on white images, and vgxt_raster_frame on frames without
a sampled mesh. Exact everywhere: np.array_equal on the uint32 images, the stride padding and everything outside the scissor
included. tests/test_gpu_raster_textured.py makes the same comparisons on the kernels."""
import ctypes as C

import numpy as np
import pytest

import raster_frame_model as M
import raster_harness as H
import raster_model as R
import raster_textured_model as T
from raster_harness import div255, draws_struct, host, image_records, rt  # noqa: F401 (host, rt: fixtures)

capi = R.capi
CLEAR = T.CLEAR
ALL = T.NAMES + ("decoded",)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_lane_code_equals_model(host, rt, name, clear):
    T.check_conditions(name, rt)
    f = T.frame(name, rt)
    tgt = f.target.with_clear(CLEAR) if clear else f.target
    want = T.expected(name, clear, rt)
    got = H.host_level(host, "textured", f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
    assert R.guards_intact(tgt, got)
    assert np.array_equal(H.host_level(host, "textured", f, tgt, with_bounds=True), got)  # the boxes handed in: the same bytes


@pytest.mark.parametrize("name", ["blit_nearest", "blit_linear"])
def test_blit_is_the_clear_blended_with_the_texels(host, name):
    """(i) white opaque vertices, UVs that map texel (x, y) onto pixel (3 + x, 2 + y): modulating by 255 gives the texel back, so the
    image is the clear colour under the texels, channel by channel."""
    T.check_conditions(name)
    f = T.frame(name)
    tgt = f.target.with_clear(CLEAR)
    want = tgt.background()
    want[:, :tgt.width] = CLEAR
    for y in range(3):
        for x in range(5):
            s = int(f.images[0].pixels[y, x])
            a = s >> 24
            if a:
                ch = [div255(((s >> (8 * k)) & 255) * a + ((CLEAR >> (8 * k)) & 255) * (255 - a)) for k in range(3)]
                want[2 + y, 3 + x] = ch[0] | (ch[1] << 8) | (ch[2] << 16) | (div255(255 * a + (CLEAR >> 24) * (255 - a)) << 24)
    got = H.host_level(host, "textured", f, tgt)
    assert np.array_equal(got, want), H.where(got, want)
    assert int((got[:, :tgt.width] != CLEAR).sum()) >= 10


@pytest.mark.parametrize("name", ALL)
def test_white_images_give_vertex_colours(host, rt, name):
    """(ii) every image all 0xFFFFFFFF: vgxt_raster_frame of the same streams with the kinds TEXT / TRILIST rewritten to FILL_AA (all of
    them: vgxt_raster_frame would also skip the clip and the paint mesh of `state`, which the new call stamps and draws)."""
    f = T.frame(name, rt)
    g = T.as_fill(f)
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        got = H.host_level(host, "textured", f, tgt, images=[im.white() for im in f.images])
        want = H.host_level(host, "frame", g, tgt)
        assert np.array_equal(got, want), H.where(got, want)
        assert not np.array_equal(got, T.expected(name, tgt.clear is not None, rt))  # the texels did show


@pytest.mark.parametrize("name", M.NAMES + ("decoded",))
def test_no_sampled_mesh_equals_vgxt_raster_frame(host, rt, name):
    """(iii) raster_frame_model's frames hold no mesh of kind TEXT or TRILIST: vgxt_raster_frame's bytes, with no image at all and a UV
    stream nobody reads."""
    f = M.frame(name, rt)
    kinds = f.meshes["subpath_kind"] >> 28
    assert not ((kinds == R.TEXT) | (kinds == R.TRILIST)).any()
    uv = np.full((max(f.nv, 1), 2), np.nan, dtype=np.float32)
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        got = H.host_level(host, "textured", f, tgt, images=[], uv=uv)
        assert np.array_equal(got, H.host_level(host, "frame", f, tgt))
        assert np.array_equal(got, M.expected(name, tgt.clear is not None, rt))


def test_invalid_image_writes_nothing(host):
    f = T.frame("state")
    good = T.expected("state")
    bad_recs = []
    for k in range(4):
        rec = image_records(f.images)
        if k == 0:
            rec["width"][1] = 0
        elif k == 1:
            rec["height"][0] = 16385
        elif k == 2:
            rec["stride"][1] = rec["width"][1] - 1
        else:
            rec["pixels"][0] += 2
        bad_recs.append(rec)
    for tgt in (f.target, f.target.with_clear(CLEAR)):
        for rec in bad_recs:
            got = H.host_level(host, "textured", f, tgt, records=rec, want=capi.VGX_E_INVALID_ARG)
            assert np.array_equal(got, tgt.background())
        got = H.host_level(host, "textured", f, tgt, images=f.images[:1], want=capi.VGX_E_INVALID_ARG)  # handle 1 with one image
        assert np.array_equal(got, tgt.background())
        assert T.status(f, images=f.images[:1]) == capi.VGX_E_INVALID_ARG
    # the same bad image named only by meshes that are not sampled: mesh 6 (a paint draw) alone names image 1 once mesh 1's clip draw
    # and mesh 4 are left out of the range
    rec = image_records(f.images)
    rec["width"][1] = 0
    got = H.host_level(host, "textured", f, f.target, records=rec, begin=5)
    assert np.array_equal(got, T.render(f, f.target, f.target.background(), mesh_begin=5))
    assert not np.array_equal(got, f.target.background()) and not np.array_equal(got, good)
    # ... and by a path-kind mesh of a type-0 draw: the backdrop's draw, pointed at a handle outside the table
    g = T.state_frame()
    g.draws["state_key"][0] |= 0xFFFF
    assert np.array_equal(H.host_level(host, "textured", g, g.target), good)


def test_non_finite_and_huge_uvs_leave_the_pixel(host):
    """A sample whose texel coordinate is NaN or at or beyond 2^31 leaves its pixel; the rest of the mesh is drawn."""
    b = R.Builder()
    b.mesh(M.quad(2.0, 2.0, 12.0, 12.0), 0xFFFFFFFF, M.QUAD, kind=R.TRILIST)     # u grows to 2^31 / W at the right edge: the right part stays
    b.mesh(M.quad(14.0, 2.0, 24.0, 12.0), 0xFFFFFFFF, M.QUAD, kind=R.TRILIST)    # a NaN on vertex 1: every sample of triangle 0 (0 * NaN is NaN)
    b.mesh(M.quad(2.0, 14.0, 12.0, 24.0), 0xFFFFFFFF, M.QUAD, kind=R.TEXT)       # an infinity on vertex 0: every sample of both triangles
    fr = b.frame("huge", R.Target(26, 26, 27, 0, 0))
    uv = np.array([(0, 0), (2.0 ** 31 / 4 * 2, 0), (2.0 ** 31 / 4 * 2, 1), (0, 1),
                   (0, 0), (np.nan, 0), (1, 1), (0, 1),
                   (np.inf, 0), (1, 0), (1, 1), (0, 1)], dtype=np.float32)
    im = T.Image(T.texels(4, 4, 4, 9, [255]), 4, T.NEAREST)
    f = T.finish(fr, [0, 0, 0], [0], [M.state()], [0], uv, [im])
    got = H.host_level(host, "textured", f, f.target)
    want = T.render(f, f.target, f.target.background())
    assert np.array_equal(got, want), H.where(got, want)
    ch = got != f.target.background()
    assert ch[2:12, 2:7].all() and not ch[2:12, 7:12].any()                          # U = x' / 10 * 2^32 reaches 2^31 at the middle
    assert ch[2:12, 14:24].sum() > 20 and (~ch[2:12, 14:24]).sum() > 20               # the triangle without the NaN vertex is drawn
    assert not ch[14:24, 2:12].any()


def test_mesh_range_and_split_calls(host):
    """Two calls over two halves of `crowd` give the bytes of one call (no stamp is in use there), and the range is the model's."""
    f = T.frame("crowd")
    img = H.host_level(host, "textured", f, f.target, end=150)
    assert np.array_equal(img, T.render(f, f.target, f.target.background(), mesh_end=150))
    img = H.host_level(host, "textured", f, f.target, image=img, begin=150)
    assert np.array_equal(img, T.expected("crowd"))


def test_host_argument_checks(host):
    f = T.frame("state")
    img = f.target.background()
    d, s = f.desc(), draws_struct(f)
    rec = image_records(f.images)
    bad = capi.VGX_E_INVALID_ARG

    def call(tex=None, no_tex=False, begin=0):
        t = f.target.struct(img.ctypes.data)
        x = capi.RasterTextures(f.uv.ctypes.data, rec.ctypes.data, 8, 2) if tex is None else tex
        return host.vgxt_raster_textured(C.byref(d), None, begin, f.nm, C.byref(s), None if no_tex else C.byref(x), C.byref(t), None)

    uvp, recp = f.uv.ctypes.data, rec.ctypes.data
    assert call(no_tex=True) == bad
    assert call(capi.RasterTextures(uvp, recp, 0, 2)) == bad and call(capi.RasterTextures(uvp, recp, 6, 2)) == bad
    assert call(capi.RasterTextures(None, recp, 8, 2)) == bad and call(capi.RasterTextures(uvp + 4, recp, 8, 2)) == bad
    assert call(capi.RasterTextures(uvp + 2, recp, 4, 2)) == bad
    assert call(capi.RasterTextures(uvp, None, 8, 2)) == bad and call(capi.RasterTextures(uvp, recp + 4, 8, 2)) == bad
    assert np.array_equal(img, f.target.background())  # none of them wrote
    assert call(capi.RasterTextures(None, recp, 8, 2), begin=f.nm) == capi.VGX_OK  # an empty range needs no UV stream
    assert np.array_equal(img, f.target.background())


def test_struct_sizes():
    assert C.sizeof(capi.RasterImage) == 24 and C.sizeof(capi.RasterTextures) == 24 and capi.raster_image_dtype.itemsize == 24
