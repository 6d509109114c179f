"""GPU: vgx_raster_concave beside the older consumers. A frame without contour meshes gives vgx_raster_painted's bytes and status; a frame
WITH them through vgx_raster, vgx_raster_frame, vgx_raster_textured and vgx_raster_painted gives the image of the frame with those
meshes removed; vgx_pick never reports one; calls of different levels in alternation on one context do not leak state; VGX_E_GROWN,
then success on the second try; vgx_scratch_bytes counts the third tile bitmap; a counted state survives."""
import numpy as np
import pytest

import raster_concave_model as K
import raster_harness as H
import raster_model as R
import raster_painted_model as P
from raster_harness import DevFrame, dev_parts, gpu_level, rt, to_dev, warm_ctx, where  # noqa: F401 (rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = K.CLEAR


def test_levels(rt, warm_ctx):
    H.check_levels(H.DevRunner(rt, warm_ctx))


@pytest.mark.parametrize("name", ["state", "classes", "odd"])
def test_older_calls_skip_contour_meshes(rt, warm_ctx, name):
    f = K.frame(name)
    g = K.without_contours(f)
    tgt = f.target
    for fr, keep in ((f, "with"), (g, "without")):
        df, ds, dx, dp = dev_parts(fr)
        imgs = [gpu_level(rt, warm_ctx, "raster", df, tgt=tgt)[1], gpu_level(rt, warm_ctx, "frame", df, ds, tgt=tgt)[1], gpu_level(rt, warm_ctx, "textured", df, ds, dx, tgt=tgt)[1],
                gpu_level(rt, warm_ctx, "vgx_raster_painted", df, ds, dx, dp, tgt)[1]]
        if keep == "with":
            got = imgs
        else:
            for a, b in zip(got, imgs):
                assert np.array_equal(a, b), where(a, b)
    assert np.array_equal(got[3], P.render(g, tgt, tgt.background()))
    assert not np.array_equal(got[3], K.expected(name))


def test_pick_never_reports_a_contour_mesh(rt, warm_ctx):
    import torch
    f = K.frame("state")
    df = DevFrame(f)
    pts = [(14.0, 9.0), (48.0, 12.0), (12.0, 27.0), (48.0, 30.0), (60.0, 38.0)]   # inside contour meshes 1 / 2, 4, 5, 6, and on the backdrop alone
    q = np.zeros(len(pts), dtype=capi.pick_query_dtype)
    q["x"], q["y"], q["mesh_end"] = [p[0] for p in pts], [p[1] for p in pts], 0xFFFFFFFF
    hits = rt.pick(warm_ctx, df.desc, to_dev(q), len(pts)).cpu().numpy().view(capi.pick_hit_dtype)[:len(pts)]
    torch.cuda.synchronize()
    for (x, y), m in zip(pts[:4], (2, 4, 5, 6)):
        assert K.covered(f, m, f.target)[int(y), int(x)], m   # the query lies inside a contour mesh
    assert (hits["mesh"] != 0xFFFFFFFF).all() and not any(K.is_contours(f, int(m)) for m in hits["mesh"])   # the triangle mesh below is found instead


def test_alternating_levels_do_not_leak_state(rt):
    ctx = rt.Context(0)
    try:
        rt.raster_reserve(ctx, 8192, 1 << 17)
        c, p = K.frame("classes"), P.frame("classes")
        dc, dp_ = dev_parts(c), dev_parts(p)
        r = R.frame("lattice")
        for _ in range(2):
            _, got = gpu_level(rt, ctx, "vgx_raster_concave", *dc, c.target)
            assert np.array_equal(got, K.expected("classes"))
            _, got = gpu_level(rt, ctx, "vgx_raster_painted", *dp_, p.target)
            assert np.array_equal(got, P.expected("classes"))
            _, got = gpu_level(rt, ctx, "vgx_raster_concave", *dp_, p.target)   # no contour mesh: the bitmap of the call before is cleared
            assert np.array_equal(got, P.expected("classes"))
            _, got = gpu_level(rt, ctx, "raster", DevFrame(r), tgt=r.target)
            assert np.array_equal(got, R.expected("lattice"))
    finally:
        ctx.close()


def test_fresh_context_grows_then_succeeds_and_scratch_is_counted(rt):
    f = H.big_frame(K.frame("crowd"))
    tgt = f.target.with_clear(CLEAR)
    want = H.host_level(H.load_host(), "concave", f, tgt)   # the lane code, which equals the model on the shared frames
    assert int((want != tgt.background()).sum()) > 3000
    parts = dev_parts(f)
    painted = lambda ctx, tgt: gpu_level(rt, ctx, "painted", *parts, tgt)   # everything vgx_raster_painted allocates
    H.check_fresh_context_grows_then_succeeds(rt, lambda ctx, tgt, **kw: gpu_level(rt, ctx, "concave", *parts, tgt, **kw), f, lambda tgt: want, 1 << 15,
                                              prepare=painted, min_growth=4)   # one word of tile bits for 4 x 4 tiles


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_raster_concave of another stream -> vgx_tessellate_emit gives the meshes it gives without the call."""
    import torch
    f = K.frame("state")
    parts = dev_parts(f)
    ps, d = wl.tiger(2)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    img = torch.from_numpy(f.target.background().view(np.int32)).to("cuda:0")
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    import ctypes as C
    for _ in range(2):  # the first call of this context may end with VGX_E_GROWN; either way the counted state must survive
        t = f.target.with_clear(CLEAR).struct(img.data_ptr())
        assert rt.lib().vgx_raster_concave(gpu_ctx.handle, C.byref(parts[0].desc), None, 0, 2**64 - 1, C.byref(parts[1].struct), C.byref(parts[2].struct),
                                           C.byref(parts[3].struct), C.byref(t), status.data_ptr(), rt._stream_ptr()) == capi.VGX_OK
        torch.cuda.synchronize()
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), K.expected("state", True))
    bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(gpu_ctx, pset, dd, d.shape[0], bufs)
    torch.cuda.synchronize()
    pset.close()
    nv, ni = ref.sizes["num_vertices"], ref.sizes["num_indices"]
    assert np.array_equal(bufs.pos[:nv].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
    assert np.array_equal(bufs.idx[:ni].cpu().numpy().view(np.uint16), ref.idx)
