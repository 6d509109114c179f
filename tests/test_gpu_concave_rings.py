"""GPU: vgx_concave_triangulate_rings (csrc/vgx_triangulate.hip: k_tri_decide_rings between the two scans, k_tri_emit_rings) on the
batches tests/test_concave_rings_cpu.py takes: against the model and, byte for byte with the guard regions, against the lane code; two
calls; the capacities; the image of the triangulated frame against the contour frame's, kernels against kernels; and what the feature
opens: a donut and a "B" triangulated -> vgx_merge under an armed assembly -> vgx_raster_commands gives the image vgx_raster_concave
gives for the contour route, and vgx_pick hits the annulus and misses the hole."""
import ctypes as C

import numpy as np
import pytest

import cmdlist_util as cu
import concave_rings_harness as RH
import concave_rings_model as RM
import concave_triangulate_model as TM
import raster_commands_harness as CH
import raster_harness as H
import raster_model as R
import raster_painted_model as P
import test_gpu_concave_contours as GC
from raster_harness import rt, to_dev, warm_ctx  # noqa: F401 (rt, warm_ctx: fixtures)
from test_gpu_concave_triangulate import dev_streams

pytestmark = pytest.mark.gpu
capi = R.capi
F = np.float32
OK = capi.VGX_OK
GUARD = H.OUT_GUARD


@pytest.fixture(scope="module")
def host():
    return RH.load_host()


def gpu_triangulate(rt, ctx, fl, out, with_routes=True):
    import torch
    d = [to_dev(a) for a in (fl.poly, fl.subs, fl.info, fl.draws)]
    n = len(fl.specs)
    routes = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    rc = rt.lib().vgx_concave_triangulate_rings(ctx.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, C.byref(out.struct),
                                                routes.data_ptr() if with_routes else None, out.dev_sizes.data_ptr(), out.dev_status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK
    s = out.dev_sizes.cpu().numpy()
    r = routes.cpu().numpy().view(np.uint32)
    assert (r[n:] == 0x5A5A5A5A).all()
    return int(out.dev_status.item()), (int(s[2]), int(s[3]), int(s[4])), r[:n]


def gpu_streams(rt, ctx, host, fl, triangulate=True):
    if triangulate:
        _, (nm, nv, ni), _, _ = RH.host_triangulate(host, fl, H.Out(0, 0, 0))   # the sizes alone
        out = GC.DevOut(nv, ni, nm)
        st, sizes, _ = gpu_triangulate(rt, ctx, fl, out)
    else:
        nm, nv, ni = fl.expected_sizes()
        out = GC.DevOut(nv, ni, nm)
        st, sizes = GC.gpu_contours(rt, ctx, fl, out)
    assert st == OK and sizes == (nm, nv, ni)
    return dev_streams(out, nm, nv, ni)


@pytest.mark.parametrize("name", ["fixtures", "mixed", "random", "grid", "cap", "cap_plus_1"])
def test_kernels_equal_model_and_lane_code(rt, gpu_ctx, host, name):
    def tri(fl, caps):
        out = GC.DevOut(*caps)
        st, sizes, routes = gpu_triangulate(rt, gpu_ctx, fl, out)
        hout = H.Out(*caps)
        assert (st, sizes) == RH.host_triangulate(host, fl, hout)[:2] and GC.same_bytes(out, hout)   # every byte, guard regions included
        return st, sizes, routes, dev_streams(out, *sizes), True
    RH.check_against_model(host, name, tri)
    # roomier capacities, no route word, a second run: the same bytes
    fl, routes, pos, _, idx, meshes, _ = RH.want(host, name)
    caps = (len(pos) + 5, len(idx) + 3, len(meshes) + 2)
    a, b, hout = GC.DevOut(*caps), GC.DevOut(*caps), H.Out(*caps)
    assert gpu_triangulate(rt, gpu_ctx, fl, a)[0] == OK and gpu_triangulate(rt, gpu_ctx, fl, b, with_routes=False)[0] == OK
    assert RH.host_triangulate(host, fl, hout)[0] == OK and GC.same_bytes(a, hout) and GC.same_bytes(b, hout)


def test_single_ring_draws_get_the_single_ring_entry_s_words(rt, gpu_ctx, host):
    import test_gpu_concave_triangulate as GT
    specs, meant = RH.batch("single")
    fl = H.Flat(specs)
    _, (nm, nv, ni), _, _ = RH.host_triangulate(host, fl, H.Out(0, 0, 0))
    a, b = GC.DevOut(nv, ni, nm), GC.DevOut(nv, ni, nm)
    sa, za, ra = GT.gpu_triangulate(rt, gpu_ctx, fl, a)
    sb, zb, rb = gpu_triangulate(rt, gpu_ctx, fl, b)
    assert sa == sb == OK and za == zb == (nm, nv, ni) and ra.tolist() == rb.tolist() == meant
    assert all(np.array_equal(x, y) for x, y in zip(a.raw(), b.raw()))


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_gives_the_need_and_writes_nothing(rt, gpu_ctx, host, short):
    fl, routes, pos, _, idx, meshes, _ = RH.want(host, "mixed")
    nv, ni, nm = len(pos), len(idx), len(meshes)
    caps = (nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    out, hout = GC.DevOut(*caps), H.Out(*caps)
    st, sizes, got = gpu_triangulate(rt, gpu_ctx, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni) and got.tolist() == routes.tolist()
    assert RH.host_triangulate(host, fl, hout)[:2] == (st, sizes) and GC.same_bytes(out, hout)
    assert all((r == GUARD).all() for r in out.raw()[:3])


def test_no_room_at_all_still_gives_routes_and_need(rt, gpu_ctx, host):
    fl, routes, pos, _, idx, meshes, _ = RH.want(host, "fixtures")
    out = GC.DevOut(0, 0, 0)
    st, sizes, got = gpu_triangulate(rt, gpu_ctx, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (len(meshes), len(pos), len(idx)) and got.tolist() == routes.tolist()
    assert all((r == GUARD).all() for r in out.raw())


@pytest.mark.parametrize("name", ["imaged", "random"])
def test_image_of_the_triangles_equals_image_of_the_contours(rt, gpu_ctx, warm_ctx, host, name):
    specs, _ = RH.batch(name)
    RH.check_images(H.DevRunner(rt, warm_ctx), specs, lambda fl: gpu_streams(rt, gpu_ctx, host, fl), lambda fl: gpu_streams(rt, gpu_ctx, host, fl, triangulate=False),
                    least=10)


# ---- what the feature opens: a frame with a donut and a "B" has an assembled form, and vgx_pick sees the annulus ----------------------
DONUT = [RM.sq(0, 0, 40), RM.rev(RM.sq(10, 10, 20))]
LETTER_B = [RM.sq(50, 10, 40), RM.rev(RM.sq(55, 15, 10)), RM.rev(RM.sq(55, 32, 10))]


def decoded_bytes():
    r = P.Rec()

    def path(rings):
        r.begin_path()
        for pts in rings:
            pts = [tuple(float(v) for v in p) for p in pts]
            r.move_to(*pts[0])
            for p in pts[1:]:
                r.line_to(*p)
            r.close_path()

    r.begin_path(); r.rect(0, 0, 96, 64); r.fill_path(0xFF403020, cu.fill_flags(aa=False))
    path(DONUT); r.fill_path(0x8020C0FF, cu.fill_flags(concave=True, aa=False))
    path(LETTER_B); r.fill_path(0x80FF6020, cu.fill_flags(concave=True, aa=True))
    r.begin_path(); r.rect(40, 40, 30, 20); r.fill_path(0x80F0F020, cu.fill_flags(aa=True))
    return r.bytes()


def test_donut_has_an_assembled_form_and_can_be_picked(rt, host):
    import torch
    canvas = (96.0, 64.0)
    c = rt.Context(0)
    try:
        rt.raster_reserve(c, 8192, 1 << 17)
        extra = {}
        rc, ps, draws, n = cu.decode(rt, decoded_bytes(), canvas=canvas, extra=extra)
        assert rc == OK and n["skipped"] == 0
        nd = draws.shape[0]
        pset = rt.PathSet(c, ps)
        dd = rt.upload_draws(draws)
        sa = rt.tessellate_count(c, pset, dd, nd)
        A = rt.MeshBuffers(dd.device, sa["num_vertices"], sa["num_indices"], sa["num_meshes"])
        rt.tessellate_emit(c, pset, dd, nd, A)
        fl = rt.flatten(c, pset, dd, nd, apply_transform=True, to_host=False, entry="one_walk")
        seq_a = rt.mesh_seq(A, sa["num_vertices"], sa["num_indices"], sa["num_meshes"])
        dstate = to_dev(extra["draw_state"])
        frames = {}
        for route in ("triangles", "old_entry", "contours"):
            B = rt.MeshBuffers(dd.device, 600, 1600, 2 * nd)
            if route == "triangles":
                routes = rt.concave_triangulate_rings(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
            elif route == "old_entry":
                old_routes = rt.concave_triangulate(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
            else:
                rt.concave_contours(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
            torch.cuda.synchronize()
            assert int(B.dev_status.item()) == OK
            bnm, bnv, bni = (int(v) for v in B.dev_sizes.cpu().numpy()[2:5])
            nv, ni, nm = sa["num_vertices"] + bnv, sa["num_indices"] + bni, sa["num_meshes"] + bnm
            out = rt.MeshBuffers(dd.device, nv, ni, nm)
            cap = 64
            dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda:0")
            num = torch.zeros(1, dtype=torch.int64, device="cuda:0")
            uv = torch.zeros((nv, 2), dtype=torch.int16, device="cuda:0")
            c.set_assembly(dcmds, max_vb_vertices=512, dev_num=num, split_state=True, uv=uv, uv_value=(0x3FFF3FFF, 0))
            try:
                rt.merge(c, seq_a, rt.mesh_seq(B, bnv, bni, bnm), None, dd, nd, out)
            finally:
                c.set_assembly(None)
            torch.cuda.synchronize()
            assert int(out.dev_status.item()) == OK
            cmds, n_dev, st = rt.raster_cmds_from_assembly(c, dcmds, cap, num, out.meshes, nm, dstate, nd)
            torch.cuda.synchronize()
            plain = rt.MeshBuffers(dd.device, nv, ni, nm)   # the same merge with no assembly armed: what vgx_raster_concave takes
            rt.merge(c, seq_a, rt.mesh_seq(B, bnv, bni, bnm), None, dd, nd, plain)
            torch.cuda.synchronize()
            assert int(plain.dev_status.item()) == OK
            frames[route] = (B, (bnm, bnv, bni), out, (nm, nv, ni), cmds, n_dev, int(st.item()), uv, plain)
        assert routes.cpu().numpy().view(np.uint32)[:nd].tolist() == [0, TM.TRIANGLES, TM.TRIANGLES, 0]
        assert old_routes.cpu().numpy().view(np.uint32)[:nd].tolist() == [0, TM.MULTI, TM.MULTI, 0]
        # neither the contour frame nor the single-ring entry's frame has an assembled form
        assert frames["contours"][6] == capi.VGX_E_INVALID_ARG and frames["old_entry"][6] == capi.VGX_E_INVALID_ARG and frames["triangles"][6] == OK
        # ... the triangulated one has, and its image is the contour route's through vgx_raster_concave
        B, _, out, (nm, nv, ni), cmds, n_dev, _, uv, _ = frames["triangles"]
        streams = rt.raster_streams(out.pos, out.color, out.idx, nv, ni, uv_dev=uv, uv_bytes=4)
        white = CH.DevScene(CH.scene("relative"))   # its one image: 2 x 2 white texels
        image = torch.full((64, 96), 0x11223344, dtype=torch.int32, device="cuda:0")
        for _ in range(3):
            _, status = rt.raster_commands(c, streams, cmds, 64, 96, 64, images_dev=white.images, num_images=1, clear_color=0xFF101010, dev_num_cmds=n_dev, image=image)
            torch.cuda.synchronize()
            if int(status.item()) != capi.VGX_E_GROWN:
                break
        assert int(status.item()) == OK
        _, _, _, (cnm, cnv, cni), _, _, _, _, cout = frames["contours"]
        f = R.make("contours", cout.pos[:cnv].cpu().numpy(), cout.color[:cnv].cpu().numpy().view(np.uint32), cout.idx[:cni].cpu().numpy().view(np.uint16),
                   cout.meshes[:cnm * 32].cpu().numpy().view(capi.mesh_dtype), R.Target(96, 64, 96, 0, 0, clear=0xFF101010))
        f.draws, f.dstate, f.paints = draws, extra["draw_state"], extra["paints"].copy()
        f.uv, f.images = np.full((max(cnv, 1), 2), np.nan, dtype=np.float32), []
        f.gradients, f.patterns = P.scatter(f.paints)
        want = H.DevRunner(rt, c).concave(f, f.target)
        got = image.cpu().numpy().view(np.uint32)
        assert int((want != 0xFF101010).sum()) > 5000 and np.array_equal(got, want), H.where(got, want)
        # vgx_pick: (5, 5) lies in the annulus, (20, 20) in the hole
        q = np.zeros(2, dtype=capi.pick_query_dtype)
        q["x"], q["y"], q["mesh_end"] = [5.0, 20.0], [5.0, 20.0], capi.PICK_NONE
        hits = {}
        for route in ("triangles", "contours"):
            B, (bnm, bnv, bni) = frames[route][:2]
            h = torch.full((2 * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            assert rt.lib().vgx_pick(c.handle, C.byref(rt.mesh_seq(B, bnv, bni, bnm)), None, to_dev(q).data_ptr(), 2, h.data_ptr(), rt._stream_ptr()) == OK
            torch.cuda.synchronize()
            hits[route] = h.cpu().numpy().view(capi.pick_hit_dtype)
        t, k = hits["triangles"], hits["contours"]
        assert (int(t["mesh"][0]), int(t["draw"][0]), int(t["subpath_kind"][0])) == (0, 1, TM.FILL_KIND) and int(t["triangle"][0]) < 8 + 2 - 2
        assert int(t["mesh"][1]) == capi.PICK_NONE and (k.view(np.uint32) == capi.PICK_NONE).all()
        pset.close()
    finally:
        c.close()


def test_entry_on_a_non_blocking_stream_behind_a_delay():
    import stream_order as SO
    import stream_order_rings as ST
    row = [r for r in SO.CASES if r.entry == ST.ENTRY]
    assert len(row) == 1
    env = SO.Env()
    SO.run_row(row[0], env, SO.side_stream(env.torch))
