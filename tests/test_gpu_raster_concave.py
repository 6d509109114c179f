"""GPU: vgx_raster_concave (csrc/vgx_raster.hip: the frame family at the concave level, k_rasterf_tiles<true, true, true> on the tiles a
contour mesh reaches) against the numpy statement (tests/raster_concave_model.py) and the lane code on the shared frames, against the
checks of tests/raster_harness.py that do not rest on that model (the triangle twin, the
convex fan, libtess2's triangulations, the reference's AA mesh), run here through the kernels, and end to end from command-list bytes:
vgx_cmdlist_decode -> the tessellator -> vgx_flatten -> vgx_concave_contours -> vgx_merge -> vgx_raster_concave, no libtess2 and no host
visit between decode and image. Every comparison is np.array_equal on the whole uint32 buffer."""
import numpy as np
import pytest

import cmdlist_util as cu
import raster_concave_model as K
import raster_harness as H
import raster_model as R
import raster_painted_model as P
import test_gpu_concave as TC
from raster_harness import DevRunner, dev_parts, gpu_bounds, gpu_level, host, rt, warm_ctx, where  # noqa: F401 (host, rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = K.CLEAR


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


@pytest.fixture(scope="module")
def run(rt, warm_ctx):
    return DevRunner(rt, warm_ctx)


@pytest.mark.parametrize("name", K.NAMES)
def test_kernels_equal_model_and_lane_code(rt, warm_ctx, host, name):
    """Clear and no clear, with and without mesh_bounds, twice with the same bytes, inputs unchanged."""
    K.check_conditions(name)
    f = K.frame(name)
    df, ds, dx, dp = dev_parts(f)
    mb = gpu_bounds(rt, warm_ctx, df)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = K.expected(name, clear)
        _, own = gpu_level(rt, warm_ctx, "vgx_raster_concave", df, ds, dx, dp, tgt)
        assert np.array_equal(own, want), where(own, want)
        assert np.array_equal(own, H.host_level(host, "concave", f, tgt))
        assert R.guards_intact(tgt, own)
        _, given = gpu_level(rt, warm_ctx, "vgx_raster_concave", df, ds, dx, dp, tgt, bounds=mb)
        assert np.array_equal(given, want), where(given, want)
        _, again = gpu_level(rt, warm_ctx, "vgx_raster_concave", df, ds, dx, dp, tgt)
        assert np.array_equal(again, own)  # two runs, the same bytes
    assert df.unchanged() and dp.unchanged()


def test_mesh_range_and_invalid_draw(rt, warm_ctx, run):
    f = K.frame("state")
    for begin, end in ((0, 3), (2, 5), (3, 99)):
        want = K.render(f, f.target, f.target.background(), begin, end)
        assert np.array_equal(run.concave(f, f.target, begin=begin, end=end), want)
    g = K.state_frame()
    g.meshes["draw"][4] = 99  # a contour mesh outside the draw table: nothing is written, the clear included
    tgt = g.target.with_clear(CLEAR)
    assert np.array_equal(run.concave(g, tgt, want=capi.VGX_E_INVALID_ARG), tgt.background())


# ---- the checks that do not rest on the model --------------------------------------------------------------------------------
def test_triangle_twin(run):
    H.check_triangle_twin(run)


def test_convex_polygon_equals_fan(run):
    H.check_convex_fan(run)


def test_simple_concave_polygons_equal_libtess2(run, ref):
    H.check_simple_concave(run, ref)


def test_crossing_fixtures_equal_libtess2_away_from_rounded_vertices(run, ref):
    H.check_crossing(run, ref)


def test_aa_pair_image_equals_the_reference_mesh(run, host, ref):
    H.check_aa_pair_image(run, host, ref)


# ---- a decoded command list through the chain of the example -------------------------------------------------------------------
def decoded_bytes():
    """Concave fills of both rules, AA and not, a concave clip region and an AA concave shape under a linear gradient, between convex
    draws."""
    r = P.Rec()
    star = lambda cx, cy, r0, r1: [(cx + (r0 if k % 2 == 0 else r1) * np.cos(k * np.pi / 5 - 1.57), cy + (r0 if k % 2 == 0 else r1) * np.sin(k * np.pi / 5 - 1.57)) for k in range(10)]
    pent = lambda cx, cy, rad: [(cx + rad * np.cos(2 * k * 2 * np.pi / 5 - 1.57), cy + rad * np.sin(2 * k * 2 * np.pi / 5 - 1.57)) for k in range(5)]

    def path(pts):
        r.begin_path(); r.move_to(*pts[0])
        for p in pts[1:]:
            r.line_to(*p)
        r.close_path()

    r.begin_path(); r.rect(0, 0, 96, 64); r.fill_path(0xFF403020, cu.fill_flags(aa=False))
    path(pent(20.0, 20.0, 16.0)); r.fill_path(0xC020C0FF, cu.fill_flags(concave=True, aa=False))                  # a pentagram, NonZero
    path(pent(58.0, 20.0, 16.0)); r.fill_path(0xC0FF6020, cu.fill_flags(concave=True, even_odd=True, aa=False))   # ... EvenOdd
    r.begin_path(); r.rect(70, 6, 22, 22); r.rect(76, 12, 10, 10); r.fill_path(0xFF60E060, cu.fill_flags(concave=True, even_odd=True, aa=True))   # a ring with a hole, AA
    r.push_state(); r.transform_translate(2.0, 34.0); r.transform_rotate(0.1)
    r.linear_gradient(0.0, 0.0, 40.0, 20.0, 0xFF20C0FF, 0xFFFF4020)
    path(star(20.0, 14.0, 14.0, 6.0)); r.fill_gradient(cu.fill_flags(concave=True, aa=True), 0)                    # an AA concave shape under a gradient
    r.pop_state()
    r.begin_clip(0)
    path(star(70.0, 46.0, 15.0, 6.0)); r.fill_path(0xFF000000, cu.fill_flags(concave=True, aa=False))              # a concave clip region
    r.end_clip()
    r.begin_path(); r.rect(50, 30, 44, 32); r.fill_path(0xE0F0F020, cu.fill_flags(aa=False))                        # ... and what it clips
    r.reset_clip()
    return r.bytes()


def chain(rt, ctx, data, canvas):
    """decode -> tessellate -> flatten -> concave_contours -> merge on the device. Returns (frame of downloaded streams with draws, state
    and paint tables attached, MeshBuffers of the merged frame)."""
    import torch
    extra = {}
    rc, ps, draws, n = cu.decode(rt, data, canvas=canvas, extra=extra)
    assert rc == capi.VGX_OK and n["skipped"] == 0
    nd = draws.shape[0]
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(draws)
    sa = rt.tessellate_count(ctx, pset, dd, nd)
    A = rt.MeshBuffers(dd.device, sa["num_vertices"], sa["num_indices"], sa["num_meshes"])
    rt.tessellate_emit(ctx, pset, dd, nd, A)
    fl = rt.flatten(ctx, pset, dd, nd, apply_transform=True, to_host=False, entry="one_walk")
    V = int(sum(int(i["num_poly_vertices"]) for i, d in zip(fl.dinfo_dev[:nd * 40].cpu().numpy().view(capi.draw_info_dtype), draws) if int(d["fill_flags"]) & capi.FILL_CONCAVE))
    B = rt.MeshBuffers(dd.device, 3 * V, 8 * V, 2 * nd)   # a bound a caller has without looking at the output
    rt.concave_contours(ctx, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
    torch.cuda.synchronize()
    assert int(B.dev_status.item()) == capi.VGX_OK
    bs = B.dev_sizes.cpu().numpy()
    bnm, bnv, bni = int(bs[2]), int(bs[3]), int(bs[4])
    nv, ni, nm = sa["num_vertices"] + bnv, sa["num_indices"] + bni, sa["num_meshes"] + bnm
    out = rt.MeshBuffers(dd.device, nv, ni, nm)
    rt.merge(ctx, rt.mesh_seq(A, sa["num_vertices"], sa["num_indices"], sa["num_meshes"]), rt.mesh_seq(B, bnv, bni, bnm), None, dd, nd, out)
    torch.cuda.synchronize()
    assert int(out.dev_status.item()) == capi.VGX_OK
    pset.close()
    f = R.make("decoded", out.pos[:nv].cpu().numpy(), out.color[:nv].cpu().numpy().view(np.uint32), out.idx[:ni].cpu().numpy().view(np.uint16),
               out.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype), R.Target(int(canvas[0]), int(canvas[1]), int(canvas[0]) + 3, 0, 0))
    f.draws, f.dstate, f.paints = draws, extra["draw_state"], extra["paints"].copy()
    f.uv, f.images = np.full((max(nv, 1), 2), np.nan, dtype=np.float32), []
    f.gradients, f.patterns = P.scatter(f.paints)
    return f, out, (B, bnm, bnv, bni)


def test_decoded_command_list_through_the_chain(rt, warm_ctx, host):
    f, out, (B, bnm, bnv, bni) = chain(rt, warm_ctx, decoded_bytes(), (96.0, 64.0))
    kinds = f.meshes["subpath_kind"] >> 28
    cm = np.flatnonzero(kinds == capi.MESH_CONTOURS)
    assert cm.size == 5 and (kinds == capi.MESH_CONCAVE_FILL_AA).sum() == 2 and bnm == 7
    assert sorted((f.meshes["subpath_kind"][cm] & 1).tolist()) == [0, 0, 0, 1, 1]                       # both rules
    bm = B.meshes[:bnm * 32].cpu().numpy().view(capi.mesh_dtype)
    assert np.array_equal(f.meshes["subpath_kind"][np.isin(kinds, (capi.MESH_CONTOURS, capi.MESH_CONCAVE_FILL_AA))], bm["subpath_kind"])   # merge keeps kind, rule bit and order
    for k, m in enumerate(np.flatnonzero(np.isin(kinds, (capi.MESH_CONTOURS, capi.MESH_CONCAVE_FILL_AA)))):
        a, b = f.meshes[m], bm[k]
        assert (int(a["num_vertices"]), int(a["num_indices"]), int(a["draw"])) == (int(b["num_vertices"]), int(b["num_indices"]), int(b["draw"]))
        assert np.array_equal(f.idx[int(a["first_index"]):int(a["first_index"]) + int(a["num_indices"])],
                              B.idx[int(b["first_index"]):int(b["first_index"]) + int(b["num_indices"])].cpu().numpy().view(np.uint16))   # ... and the edges
    assert (np.diff(f.meshes["draw"].astype(np.int64)) >= 0).all()
    df, ds, dx, dp = dev_parts(f)

    class Dev:
        desc = rt.mesh_seq(out, f.nv, f.ni, f.nm)
    for clear in (False, True):
        tgt = f.target.with_clear(CLEAR) if clear else f.target
        want = K.render(f, tgt, tgt.background())
        _, got = gpu_level(rt, warm_ctx, "vgx_raster_concave", Dev, ds, dx, dp, tgt)
        assert np.array_equal(got, want), where(got, want)
        assert np.array_equal(got, H.host_level(host, "concave", f, tgt))
    st = P.Stats(f.target)
    K.render(f, f.target, f.target.background(), stats=st)
    for m in cm:
        assert (int(m) in st.per_mesh and int(st.per_mesh[int(m)].sum()) > 40) or ((int(f.draws["state_key"][int(f.meshes["draw"][m])]) >> 16) & 0xF) == P.CLIP, m   # every concave fill shows
    assert st.stamped.any()
    img, status = rt.raster_concave(warm_ctx, Dev.desc, ds.t[0], ds.t[1], f.draws.shape[0], dx.t[0], 8, dx.t[1], 0, dp.t[0], len(f.gradients), dp.t[1],
                                    len(f.patterns), 96, 64, clear_color=CLEAR)
    import torch
    torch.cuda.synchronize()
    want = K.render(f, R.Target(96, 64, 96, 0, 0, clear=CLEAR), np.zeros((64, 96), dtype=np.uint32))
    assert int(status.item()) == capi.VGX_OK and np.array_equal(img.cpu().numpy().view(np.uint32), want)
