"""GPU: vgx_concave_triangulate_nested (csrc/vgx_triangulate.hip: k_tri_decide_nested between the two scans, k_tri_emit_nested) on the
batches tests/test_concave_nested_cpu.py takes: against the model and, byte for byte with the guard regions, against the lane code; two
calls (the assignment of groups to waves does not show); the capacities; draws of one group and single groups against
vgx_concave_triangulate_rings, kernels against kernels; the image of the triangulated frame against the contour frame's; the scratch;
and what the feature opens: a word of outlined glyphs and a bullseye triangulated -> vgx_merge under an armed assembly ->
vgx_raster_commands gives the image vgx_raster_concave gives for the contour route, and vgx_pick hits the dot of an "i" and misses the
counter of an "o"."""
import ctypes as C

import numpy as np
import pytest

import cmdlist_util as cu
import concave_nested_harness as NH
import concave_nested_model as NM
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
TRIANGULATED = [n for n in list(NM.DRAWS) + list(NM.LARGE) if (NM.DRAWS.get(n) or NM.LARGE[n])[3] == TM.TRIANGLES]


@pytest.fixture(scope="module")
def host():
    return NH.load_host()


def gpu_triangulate(rt, ctx, fl, out, with_routes=True, entry="nested"):
    import torch
    d = [to_dev(a) for a in (fl.poly, fl.subs, fl.info, fl.draws)]
    n = len(fl.specs)
    routes = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    fn = rt.lib().vgx_concave_triangulate_nested if entry == "nested" else rt.lib().vgx_concave_triangulate_rings
    rc = fn(ctx.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, C.byref(out.struct),
            routes.data_ptr() if with_routes else None, out.dev_sizes.data_ptr(), out.dev_status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK
    s = out.dev_sizes.cpu().numpy()
    r = routes.cpu().numpy().view(np.uint32)
    assert (r[n:] == 0x5A5A5A5A).all()
    return int(out.dev_status.item()), (int(s[2]), int(s[3]), int(s[4])), r[:n]


def gpu_streams(rt, ctx, host, fl, entry="nested", with_routes=False):
    if entry == "contours":
        nm, nv, ni = fl.expected_sizes()
        out = GC.DevOut(nv, ni, nm)
        st, sizes = GC.gpu_contours(rt, ctx, fl, out)
        routes = None
    else:
        _, (nm, nv, ni), _, _ = NH.host_triangulate(host, fl, H.Out(0, 0, 0), entry=entry)   # the sizes alone
        out = GC.DevOut(nv, ni, nm)
        st, sizes, routes = gpu_triangulate(rt, ctx, fl, out, entry=entry)
    assert st == OK and sizes == (nm, nv, ni)
    return (dev_streams(out, nm, nv, ni), routes) if with_routes else dev_streams(out, nm, nv, ni)


@pytest.mark.parametrize("name", ["fixtures", "mixed", "random", "rings_fixtures", "rings_mixed", "rings_single", "grid_islands", "max_rings", "max_rings_plus_1",
                                  "cap_nested", "cap_nested_plus_1"])
def test_kernels_equal_model_and_lane_code(rt, gpu_ctx, host, name):
    def tri(fl, caps):
        out = GC.DevOut(*caps)
        st, sizes, routes = gpu_triangulate(rt, gpu_ctx, fl, out)
        hout = H.Out(*caps)
        assert (st, sizes) == NH.host_triangulate(host, fl, hout)[:2] and GC.same_bytes(out, hout)   # every byte, guard regions included
        return st, sizes, routes, dev_streams(out, *sizes), True
    NH.check_against_model(host, name, tri)
    # roomier capacities, no route word, a second run: the same bytes, whichever wave clipped which group
    fl, routes, pos, _, idx, meshes, _ = NH.want(host, name)
    caps = (len(pos) + 5, len(idx) + 3, len(meshes) + 2)
    a, b, hout = GC.DevOut(*caps), GC.DevOut(*caps), H.Out(*caps)
    assert gpu_triangulate(rt, gpu_ctx, fl, a)[0] == OK and gpu_triangulate(rt, gpu_ctx, fl, b, with_routes=False)[0] == OK
    assert NH.host_triangulate(host, fl, hout)[0] == OK and GC.same_bytes(a, hout) and GC.same_bytes(b, hout)


@pytest.mark.parametrize("name,least", [("rings_fixtures", 14), ("rings_mixed", 5), ("rings_single", 5)])
def test_draws_of_one_group_get_the_rings_entry_s_words(rt, gpu_ctx, host, name, least):
    fl = NH.want(host, name)[0]
    a, ra = gpu_streams(rt, gpu_ctx, host, fl, with_routes=True)
    b, rb = gpu_streams(rt, gpu_ctx, host, fl, entry="rings", with_routes=True)
    more = NH.check_one_group_draws_equal_the_rings_entry(host, name, a, b, ra, rb, least)
    assert more == {"rings_fixtures": 3, "rings_mixed": 2, "rings_single": 0}[name]   # island, island_eo, separate


@pytest.mark.parametrize("name", TRIANGULATED)
def test_every_group_gets_the_rings_entry_s_triangles(rt, gpu_ctx, host, name):
    n = NH.check_groups_equal_the_rings_entry(name, lambda specs: gpu_streams(rt, gpu_ctx, host, H.Flat(specs)),
                                              lambda specs: gpu_streams(rt, gpu_ctx, host, H.Flat(specs), entry="rings"))
    assert n == NM.fixture(name)[4]


@pytest.mark.parametrize("name,least", [("mixed", 5), ("fixtures", 3), ("rings_fixtures", 6)])
def test_refused_draws_hold_the_contour_route_bytes(rt, gpu_ctx, host, name, least):
    fl, routes = NH.want(host, name)[:2]
    a, b = gpu_streams(rt, gpu_ctx, host, fl), gpu_streams(rt, gpu_ctx, host, fl, entry="contours")
    refused = [d for d in range(len(routes)) if routes[d] > TM.TRIANGLES]
    assert len(refused) >= least
    for d in refused:
        assert NH.draw_bytes(a, d) == NH.draw_bytes(b, d) and len(NH.draw_bytes(a, d)) == (2 if fl.specs[d][1] & TM.AA else 1)


def test_triangles_tile_the_groups_in_exact_arithmetic(rt, gpu_ctx, host):
    """Exact rational areas on the kernels' output alone."""
    seen = 0
    for name in ("fixtures", "random", "grid_islands", "max_rings"):
        fl, routes = NH.want(host, name)[:2]
        pos, _, idx, meshes = gpu_streams(rt, gpu_ctx, host, fl)
        seen += NH.check_exact_areas(fl, routes, pos, idx, meshes)
    assert seen >= 14 + 10 + 2


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_gives_the_need_and_writes_nothing(rt, gpu_ctx, host, short):
    fl, routes, pos, _, idx, meshes, _ = NH.want(host, "mixed")
    nv, ni, nm = len(pos), len(idx), len(meshes)
    caps = (nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    out, hout = GC.DevOut(*caps), H.Out(*caps)
    st, sizes, got = gpu_triangulate(rt, gpu_ctx, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni) and got.tolist() == routes.tolist()
    assert NH.host_triangulate(host, fl, hout)[:2] == (st, sizes) and GC.same_bytes(out, hout)
    assert all((r == GUARD).all() for r in out.raw()[:3])


def test_no_room_at_all_still_gives_routes_and_need(rt, gpu_ctx, host):
    fl, routes, pos, _, idx, meshes, _ = NH.want(host, "fixtures")
    out = GC.DevOut(0, 0, 0)
    st, sizes, got = gpu_triangulate(rt, gpu_ctx, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (len(meshes), len(pos), len(idx)) and got.tolist() == routes.tolist()
    assert all((r == GUARD).all() for r in out.raw())


@pytest.mark.parametrize("name,least", [("imaged", None), ("random", 10)])
def test_image_of_the_triangles_equals_image_of_the_contours(rt, gpu_ctx, warm_ctx, host, name, least):
    specs, meant = NH.batch(name)
    if name == "imaged":
        least = meant.count(TM.TRIANGLES)   # the listed routes
        assert least >= 15
    NH.check_images(H.DevRunner(rt, warm_ctx), specs, lambda fl: gpu_streams(rt, gpu_ctx, host, fl), lambda fl: gpu_streams(rt, gpu_ctx, host, fl, entry="contours"),
                    least=least)


def test_scratch_is_on_the_context_s_list_and_grows_by_a_word_per_draw(rt, host):
    """include/vgx.h: the rings entry's scratch and 4 bytes per draw for G."""
    fl, _, pos, _, idx, meshes, _ = NH.want(host, "fixtures")
    n = len(fl.specs)
    c = rt.Context(0)
    try:
        cap_v = 2 * len(pos)   # room for either entry: what the rings entry refuses holds contour meshes
        out = GC.DevOut(cap_v, 3 * len(idx), 2 * len(meshes))
        before = int(rt.lib().vgx_scratch_bytes(c.handle))
        assert gpu_triangulate(rt, c, fl, out, entry="rings")[0] == OK
        rings = int(rt.lib().vgx_scratch_bytes(c.handle))
        slots = min(cap_v + 2 * (cap_v // 3), n * capi.TRIANGULATE_MAX_VERTICES)
        assert rings - before >= 36 * n + 6 * slots
        assert gpu_triangulate(rt, c, fl, out)[0] == OK
        nested = int(rt.lib().vgx_scratch_bytes(c.handle))
        words = 4 * (n + 1)
        assert 4 * n <= nested - rings <= words + words // 8 + 256   # the buffer list's head room
        assert gpu_triangulate(rt, c, fl, out)[0] == OK and int(rt.lib().vgx_scratch_bytes(c.handle)) == nested   # and stays
    finally:
        c.close()


# ---- what the feature opens: a line of outlined text and a target have an assembled form, and vgx_pick sees the glyphs ---------------
MOVE = np.array([8.0, 34.0], dtype=F)
WORD = NM.word_rings()
TARGET_RINGS = [r + MOVE for r in NM.BULLSEYE]


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

    r.begin_path(); r.rect(0, 0, 96, 120); r.fill_path(0xFF403020, cu.fill_flags(aa=False))
    path(WORD); r.fill_path(0x8020C0FF, cu.fill_flags(concave=True, aa=False))
    path(TARGET_RINGS); r.fill_path(0x80FF6020, cu.fill_flags(concave=True, aa=True))
    r.begin_path(); r.rect(40, 20, 30, 30); r.fill_path(0x80F0F020, cu.fill_flags(aa=True))
    return r.bytes()


def assembled_image(rt, list_bytes, width, height, clear):
    """decode -> tessellate (a) + flatten -> runtime.concave_triangulate_nested (b) -> merge under an armed assembly ->
    raster_cmds_from_assembly -> raster_commands: (routes, the image as uint32 [height, width], the merged sizes)."""
    import torch
    c = rt.Context(0)
    try:
        rt.raster_reserve(c, 8192, 1 << 17)
        extra = {}
        rc, ps, draws, n = cu.decode(rt, list_bytes, canvas=(float(width), float(height)), extra=extra)
        assert rc == OK and n["skipped"] == 0
        nd = draws.shape[0]
        pset = rt.PathSet(c, ps)
        dd = rt.upload_draws(draws)
        sa = rt.tessellate_count(c, pset, dd, nd)
        A = rt.MeshBuffers(dd.device, sa["num_vertices"], sa["num_indices"], sa["num_meshes"])
        rt.tessellate_emit(c, pset, dd, nd, A)
        fl = rt.flatten(c, pset, dd, nd, apply_transform=True, to_host=False, entry="one_walk")
        B = rt.MeshBuffers(dd.device, 1024, 4096, 2 * nd)
        routes = rt.concave_triangulate_nested(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
        torch.cuda.synchronize()
        assert int(B.dev_status.item()) == OK
        bnm, bnv, bni = (int(v) for v in B.dev_sizes.cpu().numpy()[2:5])
        nv, ni, nm = sa["num_vertices"] + bnv, sa["num_indices"] + bni, sa["num_meshes"] + bnm
        out = rt.MeshBuffers(dd.device, nv, ni, nm)
        cap = 64
        dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda:0")
        num = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        uv = torch.zeros((nv, 2), dtype=torch.int16, device="cuda:0")
        c.set_assembly(dcmds, max_vb_vertices=512, dev_num=num, split_state=True, uv=uv, uv_value=(0x40004000, 0))
        try:
            rt.merge(c, rt.mesh_seq(A, sa["num_vertices"], sa["num_indices"], sa["num_meshes"]), rt.mesh_seq(B, bnv, bni, bnm), None, dd, nd, out)
        finally:
            c.set_assembly(None)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == OK
        cmds, n_dev, st = rt.raster_cmds_from_assembly(c, dcmds, cap, num, out.meshes, nm, to_dev(extra["draw_state"]), nd)
        torch.cuda.synchronize()
        assert int(st.item()) == OK
        streams = rt.raster_streams(out.pos, out.color, out.idx, nv, ni, uv_dev=uv, uv_bytes=4)
        white = CH.DevScene(CH.scene("relative"))   # its one image: 2 x 2 white texels
        image = torch.full((height, width), 0x11223344, dtype=torch.int32, device="cuda:0")
        for _ in range(3):
            _, status = rt.raster_commands(c, streams, cmds, cap, width, height, images_dev=white.images, num_images=1, clear_color=clear, dev_num_cmds=n_dev, image=image)
            torch.cuda.synchronize()
            if int(status.item()) != capi.VGX_E_GROWN:
                break
        assert int(status.item()) == OK
        pset.close()
        return routes.cpu().numpy().view(np.uint32)[:nd].tolist(), image.cpu().numpy().view(np.uint32), (nm, nv, ni)
    finally:
        c.close()


def test_outlined_text_has_an_assembled_form_and_can_be_picked(rt, host):
    import torch
    canvas = (96.0, 120.0)
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
        frames, routes = {}, {}
        for route in ("nested", "rings", "contours"):
            B = rt.MeshBuffers(dd.device, 600, 1600, 2 * nd)
            if route == "nested":
                routes[route] = rt.concave_triangulate_nested(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
            elif route == "rings":
                routes[route] = rt.concave_triangulate_rings(c, fl.poly_dev, fl.subs_dev, fl.dinfo_dev, dd, nd, B)
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
        assert routes["nested"].cpu().numpy().view(np.uint32)[:nd].tolist() == [0, TM.TRIANGLES, TM.TRIANGLES, 0]
        assert routes["rings"].cpu().numpy().view(np.uint32)[:nd].tolist() == [0, RM.NESTING, RM.NESTING, 0]
        # neither the contour frame nor the rings entry's frame has an assembled form
        assert frames["contours"][6] == capi.VGX_E_INVALID_ARG and frames["rings"][6] == capi.VGX_E_INVALID_ARG and frames["nested"][6] == OK
        # ... the triangulated one has, and its image is the contour route's through vgx_raster_concave
        B, _, out, (nm, nv, ni), cmds, n_dev, _, uv, _ = frames["nested"]
        streams = rt.raster_streams(out.pos, out.color, out.idx, nv, ni, uv_dev=uv, uv_bytes=4)
        white = CH.DevScene(CH.scene("relative"))   # its one image: 2 x 2 white texels
        image = torch.full((120, 96), 0x11223344, dtype=torch.int32, device="cuda:0")
        for _ in range(3):
            _, status = rt.raster_commands(c, streams, cmds, 64, 96, 120, images_dev=white.images, num_images=1, clear_color=0xFF101010, dev_num_cmds=n_dev, image=image)
            torch.cuda.synchronize()
            if int(status.item()) != capi.VGX_E_GROWN:
                break
        assert int(status.item()) == OK
        _, _, _, (cnm, cnv, cni), _, _, _, _, cout = frames["contours"]
        f = R.make("contours", cout.pos[:cnv].cpu().numpy(), cout.color[:cnv].cpu().numpy().view(np.uint32), cout.idx[:cni].cpu().numpy().view(np.uint16),
                   cout.meshes[:cnm * 32].cpu().numpy().view(capi.mesh_dtype), R.Target(96, 120, 96, 0, 0, clear=0xFF101010))
        f.draws, f.dstate, f.paints = draws, extra["draw_state"], extra["paints"].copy()
        f.uv, f.images = np.full((max(cnv, 1), 2), np.nan, dtype=np.float32), []
        f.gradients, f.patterns = P.scatter(f.paints)
        want = H.DevRunner(rt, c).concave(f, f.target)
        got = image.cpu().numpy().view(np.uint32)
        assert int((want != 0xFF101010).sum()) > 5000 and np.array_equal(got, want), H.where(got, want)
        # vgx_pick on the concave draws alone. Hits: the dot of the "i" (glyph 2), the rim of the first "o", the innermost square of
        # the target. Misses: the counter of that "o", the gap between the first two glyphs, the second ring of the target
        pts = [(33.0, 11.0), (3.0, 15.0), (48.0, 74.0), (7.0, 15.0), (13.5, 15.0), (15.5, 74.0)]
        q = np.zeros(len(pts), dtype=capi.pick_query_dtype)
        q["x"], q["y"], q["mesh_end"] = [p[0] for p in pts], [p[1] for p in pts], capi.PICK_NONE
        hits = {}
        for route in ("nested", "contours"):
            B, (bnm, bnv, bni) = frames[route][:2]
            h = torch.full((len(pts) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            assert rt.lib().vgx_pick(c.handle, C.byref(rt.mesh_seq(B, bnv, bni, bnm)), None, to_dev(q).data_ptr(), len(pts), h.data_ptr(), rt._stream_ptr()) == OK
            torch.cuda.synchronize()
            hits[route] = h.cpu().numpy().view(capi.pick_hit_dtype)
        t, k = hits["nested"], hits["contours"]
        assert [(int(t["mesh"][i]), int(t["draw"][i]), int(t["subpath_kind"][i])) for i in range(3)] == [(0, 1, TM.FILL_KIND), (0, 1, TM.FILL_KIND), (1, 2, TM.FILL_KIND)]
        assert all(int(t["triangle"][i]) < 60 for i in range(2)) and int(t["triangle"][2]) >= 2 * 20   # behind the 2 V fringe triangles of the AA target
        assert all(int(t["mesh"][i]) == capi.PICK_NONE for i in range(3, 6)) and (k.view(np.uint32) == capi.PICK_NONE).all()
        pset.close()
    finally:
        c.close()


def test_entry_on_a_non_blocking_stream_behind_a_delay():
    """The row also runs with the whole table (tests/test_gpu_stream_order.py). The side stream here is made with the runtime's own call
    and wrapped, not taken from torch's pool: which pool stream the table's tests get later does not depend on this file."""
    import stream_order as SO
    import stream_order_nested as ST
    row = [r for r in SO.CASES if r.entry == ST.ENTRY]
    assert len(row) == 1
    env = SO.Env()
    hip = SO._hip()
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(h), SO.HIP_STREAM_NON_BLOCKING) == 0 and h.value
    try:
        SO.run_row(row[0], env, env.torch.cuda.ExternalStream(h.value))
    finally:
        env.torch.cuda.synchronize()
        assert hip.hipStreamDestroy(h) == 0
