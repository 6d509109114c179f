"""GPU: vgx_raster_commands (k_rasterc_*) on the hand-built scenes of raster_commands_harness against oracle A -- the model, and
vgx_raster_painted on the equivalent one-mesh-per-command frame -- in every byte, guards and stride padding included; the statuses and
the VGX_E_GROWN protocol; frames of the reference's own Context in vg::end order and in buffer order (oracles B and C); the product's
assembled frame through vgx_raster_cmds_from_assembly."""
import ctypes as C

import numpy as np
import pytest

import raster_commands_harness as CH
import raster_commands_model as CM
import raster_frame_model as M
import raster_harness as H
import raster_model as R
from raster_harness import rt  # noqa: F401

pytestmark = pytest.mark.gpu
capi = R.capi
OK, BAD, GROWN = CH.OK, CH.BAD, CH.GROWN


@pytest.fixture(scope="module")
def ctx(rt):
    """A context whose scratch has room for every scene: the tests of the result do not meet VGX_E_GROWN."""
    c = rt.Context(0)
    rt.raster_reserve(c, 1024, 1 << 14)
    rt.raster_commands_reserve(c, 64, 1024, 1 << 14)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    return CH.load_host()


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", sorted(CH.SCENES))
def test_scene_equals_oracle_a(rt, ctx, name, clear):
    CH.check_scene_on_device(rt, ctx, name, clear)


def test_seam_is_drawn_once(rt, ctx):
    sc = CH.scene("seam")
    CH.check_seam(CH.gpu_commands(rt, ctx, sc, sc.target.with_clear(CH.CLEAR))[1])


def test_empty_target_scissor_is_ok(rt, ctx):
    tgt = R.Target(24, 16, 24, 0, 0, scissor=(5, 5, 5, 9), clear=CH.CLEAR)
    assert np.array_equal(CH.gpu_commands(rt, ctx, CH.scene("relative"), tgt)[1], tgt.background())
    tgt = R.Target(64, 24, 64, 0, 0, scissor=(50, 0, 64, 4), clear=CH.CLEAR)
    want = tgt.background()
    want[0:4, 50:64] = CH.CLEAR
    assert np.array_equal(CH.gpu_commands(rt, ctx, CH.scene("scissors"), tgt)[1], want)


@pytest.mark.parametrize("case", sorted(CH.invalid_cases()))
def test_each_invalid_record_alone(rt, ctx, case):
    sc = CH.invalid_cases()[case]
    tgt = sc.target.with_clear(CH.CLEAR)
    assert np.array_equal(CH.gpu_commands(rt, ctx, sc, tgt, want=BAD)[1], tgt.background())


def test_grown_protocol_and_ranking(rt):
    """One command whose two triangles cover a 64 x 64 image: 16 entries against a fresh context's one. VGX_E_GROWN and nothing written,
    the clear included; VGX_OK on the repeat; VGX_E_INVALID_ARG ranks above VGX_E_GROWN; VGX_OK at once after the reserve."""
    import torch
    sc = CH.scene("full_quad")
    assert CM.totals(sc) == (1, 16)
    tgt = sc.target.with_clear(CH.CLEAR)
    want = CH.expected("full_quad", True)
    invalid = sc.with_cmds(np.concatenate([sc.cmds, sc.cmds]))
    invalid.cmds["type"][1] = 7
    c = rt.Context(0)
    try:
        assert np.array_equal(CH.gpu_commands(rt, c, invalid, tgt, want=BAD)[1], tgt.background())
    finally:
        c.close()
    c = rt.Context(0)
    try:
        dev = CH.DevScene(sc)
        img, got = CH.gpu_commands(rt, c, sc, tgt, want=GROWN, dev=dev)
        assert np.array_equal(got, tgt.background())
        _, got = CH.gpu_commands(rt, c, sc, tgt, image=img, dev=dev)
        assert np.array_equal(got, want), H.where(got, want)
    finally:
        c.close()
    c = rt.Context(0)
    try:
        before = int(rt.lib().vgx_scratch_bytes(c.handle))
        rt.raster_commands_reserve(c, 1, 1, 16)
        assert int(rt.lib().vgx_scratch_bytes(c.handle)) > before  # the scratch is on the context's list
        assert np.array_equal(CH.gpu_commands(rt, c, sc, tgt)[1], want)
    finally:
        c.close()
    assert rt.lib().vgx_raster_commands_reserve(None, 1, 1, 1) == BAD
    torch.cuda.synchronize()


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    sc = CH.scene("clip")
    dev = CH.DevScene(sc)
    tgt = sc.target

    def call():
        return rt.raster_commands(gpu_ctx, dev.streams, dev.t[3], sc.cmds.shape[0], tgt.width, tgt.height, images_dev=dev.images, num_images=len(sc.images),
                                  clear_color=CH.CLEAR)

    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, call, CH.expected("clip", True)[:, :tgt.width])


@pytest.mark.parametrize("again", [False, True])
def test_reference_frame_both_orders(rt, ctx, again):
    """Oracles B and C on the device."""
    rs = CH.RefScene(rt, again)

    def painted(f):
        df, ds, dx, dp = H.dev_parts(f)
        return H.gpu_level(rt, ctx, "painted", df, ds, dx, dp, f.target)[1]

    CH.check_reference_frame(rs, lambda sc: CH.gpu_commands(rt, ctx, sc)[1], painted)


@pytest.mark.parametrize("again", [False, True])
def test_product_assembly_to_image(rt, ctx, host, again):
    """The same scenario through the product: vgx_set_assembly (VGX_ASM_SPLIT_STATE, max_vb_vertices 512) -> vgx_raster_cmds_from_assembly
    -> vgx_raster_commands gives the image of vgx_raster_painted on the unassembled frame; the records equal the lane code's and the
    reference's two tables merged in buffer order, field by field."""
    import torch
    rs = CH.RefScene(rt, again)
    f = rs.unassembled((0, 0))
    c = rt.Context(0)
    try:
        pset = rt.PathSet(c, rs.ps)
        dd = rt.upload_draws(rs.draws)
        cap = 256
        dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda:0")
        num = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        uv = torch.zeros((f.nv, 2), dtype=torch.int16, device="cuda:0")
        bufs = rt.MeshBuffers(dd.device, f.nv, f.ni, f.nm)
        c.set_assembly(dcmds, max_vb_vertices=512, dev_num=num, split_state=True, uv=uv, uv_value=(int(rs.ref["white_uv"][0][0]), 0))
        try:
            sizes = rt.tessellate_count(c, pset, dd, rs.draws.shape[0])
            assert (sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]) == (f.nv, f.ni, f.nm)
            rt.tessellate_emit(c, pset, dd, rs.draws.shape[0], bufs)
        finally:
            c.set_assembly(None)
        torch.cuda.synchronize()
        dstate = H.to_dev(rs.dstate)
        out, n, status = rt.raster_cmds_from_assembly(c, dcmds, cap, num, bufs.meshes, f.nm, dstate, rs.dstate.shape[0])
        torch.cuda.synchronize()
        k = int(num.item())
        assert int(status.item()) == OK and int(n.item()) == k
        got = out.cpu().numpy()[:k * 56].view(capi.raster_cmd_dtype)
        # the lane code on the same tables
        hd = dcmds.cpu().numpy()[:k * 48].view(capi.drawcmd_dtype).copy()
        hm = bufs.meshes.cpu().numpy()[:f.nm * 32].view(capi.mesh_dtype).copy()
        st = capi.RasterDraws(None, rs.dstate.ctypes.data, rs.dstate.shape[0], 0)
        want, hn, hs = np.zeros(k, dtype=capi.raster_cmd_dtype), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        assert host.vgxt_raster_cmds_from_assembly(hd.ctypes.data, k, hm.ctypes.data, f.nm, C.byref(st), want.ctypes.data, hn.ctypes.data, hs.ctypes.data) == OK
        assert got.tobytes() == want.tobytes()
        # the reference's tables in buffer order
        ref = rs.buffer_order()
        assert len(ref) == k
        for name in ("first_vertex", "first_index", "num_vertices", "num_indices", "type", "scissor"):
            assert np.array_equal(got[name], ref[name]), name
        users = ref["type"] != CM.CLIP
        painted_cmds = users & (ref["type"] != 0)
        assert np.array_equal(got["handle"][painted_cmds], ref["handle"][painted_cmds])
        tested = users & (ref["clip_first_cmd"] != CM.NONE) & (ref["clip_num_cmds"] != 0)
        assert tested.any() and np.array_equal(got["clip_first_cmd"][users & ~tested], np.full(int((users & ~tested).sum()), CM.NONE, dtype=np.uint32))
        for name in ("clip_first_cmd", "clip_num_cmds", "clip_rule"):
            assert np.array_equal(got[name][tested], ref[name][tested]), name
        # the image
        streams = rt.raster_streams(bufs.pos, bufs.color, bufs.idx, f.nv, f.ni, uv_dev=uv, uv_bytes=4)
        images = CH.DevScene(rs.scene(ref, (0, 0), "images"))
        dp = H.DevPaints(rs.gradients, rs.patterns)
        for w in CH.REF_WINDOWS:
            fw = rs.unassembled(w)
            df, ds, dx, _ = H.dev_parts(fw)
            expect = H.gpu_level(rt, ctx, "painted", df, ds, dx, dp, fw.target)[1]
            image = torch.from_numpy(fw.target.background().view(np.int32)).to("cuda:0")
            _, status = rt.raster_commands(ctx, streams, out, k, 64, 48, images_dev=images.images, num_images=len(rs.images), gradients_dev=dp.t[0],
                                           num_gradients=len(rs.gradients), patterns_dev=dp.t[1], num_patterns=len(rs.patterns), x0=w[0], y0=w[1],
                                           clear_color=CH.CLEAR, dev_num_cmds=n, image=image)
            torch.cuda.synchronize()
            assert int(status.item()) == OK
            img = image.cpu().numpy().view(np.uint32)
            assert np.array_equal(img, expect), (w, H.where(img, expect))
        pset.close()
    finally:
        c.close()


def test_cmds_from_assembly_statuses(rt, ctx):
    """A first_mesh outside the table and a contour mesh give VGX_E_INVALID_ARG; the host refuses null and misaligned pointers."""
    import torch
    meshes = np.zeros(2, dtype=capi.mesh_dtype)
    meshes["draw"] = [0, 1]
    dstate = np.zeros(2, dtype=capi.draw_state_dtype)
    dstate["clip_first_draw"] = capi.CLIP_NONE
    dc = np.zeros(2, dtype=capi.drawcmd_dtype)
    dc["first_mesh"] = [0, 1]

    def run(dc, meshes, dev_num=None):
        out, n, status = rt.raster_cmds_from_assembly(ctx, H.to_dev(dc), len(dc), dev_num, H.to_dev(meshes), len(meshes), H.to_dev(dstate), 2)
        torch.cuda.synchronize()
        return int(n.item()), int(status.item())

    assert run(dc, meshes) == (2, OK)
    assert run(dc, meshes, torch.tensor([1], dtype=torch.int64, device="cuda:0")) == (1, OK)
    bad = dc.copy()
    bad["first_mesh"][1] = 2
    assert run(bad, meshes) == (2, BAD)
    contour = meshes.copy()
    contour["subpath_kind"][1] = capi.MESH_CONTOURS << 28
    assert run(dc, contour) == (2, BAD)
    assert rt.lib().vgx_raster_cmds_from_assembly(ctx.handle, None, 0, None, None, 0, None, None, None, None, None) == BAD
