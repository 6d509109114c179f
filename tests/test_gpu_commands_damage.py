"""GPU: vgx_raster_commands_damaged (the DAMAGE instantiations of k_rasterc_* in csrc/vgx_raster_cmds.hip) against vgx_raster_commands
on the same device: the checks of tests/test_commands_damage_cpu.py on the kernels, with the chain's own calls -- vgx_command_bounds,
vgx_damage_meshes -- run on the device too; the sort window; and the chain through the product's assembly: a cached frame submitted under
vgx_set_assembly, vgx_raster_cmds_from_assembly, vgx_damage_instances around vgx_cache_update, the vgx_command_bounds refresh."""
import types

import numpy as np
import pytest

import command_boxes_harness as B
import command_bounds_model as BM
import damage_model as DM
import raster_commands_harness as CH
import raster_commands_model as CM
import raster_concave_model as K
import raster_frame_model as M
import raster_harness as H
from raster_harness import rt  # noqa: F401

pytestmark = pytest.mark.gpu
capi = B.capi
OK, BAD, GROWN = B.OK, B.BAD, B.GROWN
CLEAR = B.CLEAR


@pytest.fixture(scope="module")
def ctx(rt):
    """A context whose scratch has room for every scene: the tests of the result do not meet VGX_E_GROWN."""
    c = rt.Context(0)
    rt.raster_commands_reserve(c, 64, 1024, 1 << 14)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side(rt, ctx):
    return B.DevSide(rt, ctx)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", sorted(CH.SCENES))
def test_every_bit_set_is_the_full_call(side, name, clear):
    B.check_all_bits(side, name, clear)


def test_no_bit_set_writes_nothing_and_still_reports_an_invalid_record(side):
    B.check_no_bits(side)


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("name", B.QUARTER_SCENES)
def test_a_random_quarter_of_the_tiles(side, name, clear):
    B.check_random_quarter(side, name, clear)


def test_clip_command_partly_in_unmarked_tiles(side):
    B.check_clip_partly_unmarked(side)


def test_tile_of_five_chunks_alone_then_its_neighbours_alone(side):
    B.check_trips_tile_and_neighbours(side)


def test_bits_across_a_word_boundary(side):
    B.check_word_boundary(side)


def test_what_the_box_table_holds_decides(side):
    B.check_boxes_decide(side)


def test_redraw_property(side):
    B.check_redraw_property(side)


# ---- the sort window -----------------------------------------------------------------------------------------------------------------------
def test_max_entries_too_small_grows_then_succeeds(rt):
    """A window of one entry against 16: VGX_E_GROWN with nothing written, the clear included; the same call repeated after a synchronise
    reaches VGX_OK, and so do the library's window and a wide one afterwards. On a fresh context with nothing reserved the initial window
    holds the frame at once."""
    sc = CH.scene("full_quad")
    tgt = sc.target.with_clear(CLEAR)
    bits = DM.all_bits(tgt.width, tgt.height)
    want = CH.expected("full_quad", True)
    c = rt.Context(0)
    rt.raster_commands_reserve(c, 4, 16, 64)
    try:
        s = B.DevSide(rt, c)
        dev = CH.DevScene(sc)
        got = s.damaged(sc, tgt, bits, want=GROWN, max_entries=1, dev=dev)
        assert np.array_equal(got, tgt.background())
        got = s.damaged(sc, tgt, bits, max_entries=1, dev=dev)
        assert np.array_equal(got, want), H.where(got, want)
        assert np.array_equal(s.damaged(sc, tgt, bits, max_entries=0, dev=dev), want)
        assert np.array_equal(s.damaged(sc, tgt, bits, BM.boxes(sc)[0], max_entries=1 << 20, dev=dev), want)
    finally:
        c.close()
    c = rt.Context(0)
    try:
        assert np.array_equal(B.DevSide(rt, c).damaged(sc, tgt, bits, max_entries=0), want)
    finally:
        c.close()


def full_quads(m):
    """m commands whose two triangles each cover a 64 x 64 image: m chunks, 16 m bin entries."""
    b = CM.Builder()
    rs = np.random.RandomState(m)
    for _ in range(m):
        b.add(M.quad(-1.0, -1.0, 65.0, 65.0), B.rgba(int(rs.randint(256)), int(rs.randint(256)), int(rs.randint(256)), 40), M.QUAD)
    return b.scene("full_quads_%d" % m, CH.scene("full_quad").target)


def test_full_renders_in_between_do_not_move_the_damaged_window(rt):
    """The library's window (max_entries = 0) follows the last DAMAGED call alone. After a damaged call of 16 entries (window 16 + 2 + 256)
    a full render of 3 200 entries does not widen it: the damaged call of 1 120 entries that follows ends with VGX_E_GROWN -- with one
    shared count its window would have been 3 856 and it would have passed. Its repeat passes; then a full render of 16 entries does not
    narrow the window either: the next damaged call of 1 120 entries passes at once."""
    small, mid, big = CH.scene("full_quad"), full_quads(70), full_quads(200)
    tgt = small.target.with_clear(CLEAR)
    bits = DM.all_bits(tgt.width, tgt.height)
    assert CM.totals(mid) == (70, 1120) and CM.totals(big) == (200, 3200) and 16 + 2 + 256 < 1120 < 3200
    c = rt.Context(0)
    rt.raster_commands_reserve(c, 256, 512, 8192)   # every table holds every scene: what ends a call below is its window alone
    try:
        s = B.DevSide(rt, c)
        want_mid = s.commands(mid, tgt)
        assert not np.array_equal(want_mid, tgt.background())
        assert np.array_equal(s.damaged(small, tgt, bits, max_entries=0), CH.expected("full_quad", True))
        s.commands(big, tgt)
        got = s.damaged(mid, tgt, bits, want=GROWN, max_entries=0)
        assert np.array_equal(got, tgt.background())
        assert np.array_equal(s.damaged(mid, tgt, bits, max_entries=0), want_mid)
        s.commands(small, tgt)
        assert np.array_equal(s.damaged(mid, tgt, bits, max_entries=0), want_mid)
    finally:
        c.close()


def test_a_chunk_without_a_marked_tile_costs_no_entry(rt):
    """16 entries with every bit set, 1 with one tile marked: a window of one entry is then enough at the first call."""
    sc = CH.scene("full_quad")
    tgt = sc.target.with_clear(CLEAR)
    c = rt.Context(0)
    rt.raster_commands_reserve(c, 4, 16, 64)
    try:
        s = B.DevSide(rt, c)
        bits = B.bits_of(tgt, [(2, 1)])
        got = s.damaged(sc, tgt, bits, max_entries=1)
        want = tgt.background()
        m = DM.tile_mask(bits, tgt)
        want[m] = CH.expected("full_quad", True)[m]
        assert np.array_equal(got, want)
    finally:
        c.close()


# ---- through the product's assembly ----------------------------------------------------------------------------------------------------------
class DevCache:
    def __init__(self, c):
        self.t = [H.to_dev(a) for a in (c.pos, c.color, c.idx, c.meshes)]
        self.nm, self.nv, self.ni = c.meshes.shape[0], c.pos.shape[0], c.idx.shape[0]
        self.bufs = types.SimpleNamespace(pos=self.t[0])

    def desc(self):
        return capi.CacheDesc(self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(), self.nm, self.nv, self.ni)


def small_cache():
    """Two ranges of one mesh each in local space around (0, 0): an AA fill with vertex colours of its own and a plain quad."""
    b = K.Builder()
    inn, out = M.quad(-5.0, -4.0, 5.0, 4.0), M.quad(-6.0, -5.0, 6.0, 5.0)
    verts, cols, idx = [], [], []
    for k in range(4):
        verts += [inn[k], out[k]]
        cols += [0xC040A0FF, 0x0040A0FF]
        i0, i2 = 2 * k, 2 * ((k + 1) % 4)
        idx += [i0, i2, i0 + 1, i2, i2 + 1, i0 + 1]
    idx += [0, 2, 4, 0, 4, 6]
    b.mesh(verts, cols, idx, kind=capi.MESH_FILL_AA)
    b.mesh(M.quad(-7.0, -1.5, 7.0, 1.5), 0xFFFFFFFF, M.QUAD, kind=capi.MESH_STROKE)
    f = b.frame("small_cache", None)
    f.meshes["draw"] = 0
    return f


def test_chain_through_the_assembly(rt):
    """Ten cached drawings submitted under an armed assembly with vertex buffers of 24 vertices -> vgx_raster_cmds_from_assembly -> a full
    render; two drawings moved and one recoloured by vgx_cache_update between two vgx_damage_instances over the frame's vgx_mesh_bounds
    table; vgx_command_bounds over the touched commands; the damaged redraw equals the full redraw of the edited frame."""
    import torch
    W, Hh, S = 96, 64, 99
    cache = DevCache(small_cache())
    rs = np.random.RandomState(6)
    n = 10
    inst = np.zeros(n, dtype=capi.cache_instance_dtype)
    for k in range(n):
        inst["first_mesh"][k], inst["num_meshes"][k] = (0, 2) if k % 3 == 0 else (k % 2, 1)
        inst["color"][k] = (0xD0 << 24) | int(rs.randint(0, 1 << 24))
        inst["mtx"][k] = [1.0, 0.0, 0.0, 1.0, 10.0 + 18.0 * (k % 5), 12.0 + 30.0 * (k // 5)]
    nm = int(inst["num_meshes"].sum())
    nv = int(sum(8 if m == 0 else 4 for k in range(n) for m in range(int(inst["first_mesh"][k]), int(inst["first_mesh"][k]) + int(inst["num_meshes"][k]))))
    ni = int(sum(30 if m == 0 else 6 for k in range(n) for m in range(int(inst["first_mesh"][k]), int(inst["first_mesh"][k]) + int(inst["num_meshes"][k]))))
    c = rt.Context(0)
    try:
        cap = 64
        dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda:0")
        num = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        uv = torch.zeros((nv, 2), dtype=torch.int16, device="cuda:0")
        bufs = rt.MeshBuffers("cuda:0", nv, ni, nm)
        inst_dev = H.to_dev(inst)
        c.set_assembly(dcmds, max_vb_vertices=24, dev_num=num, split_state=True, uv=uv, uv_value=(0x3FFF3FFF, 0))
        try:
            rt.cache_submit(c, cache, inst_dev, n, bufs)
        finally:
            c.set_assembly(None)
        torch.cuda.synchronize()
        assert int(bufs.dev_status.item()) == OK and [int(v) for v in bufs.dev_sizes[2:5].cpu()] == [nm, nv, ni]
        ncmd = int(num.item())
        assert 4 <= ncmd <= cap
        dstate = np.zeros(n, dtype=capi.draw_state_dtype)
        dstate["scissor"], dstate["clip_first_draw"] = (0, 0, 65535, 65535), 0xFFFFFFFF
        cmds, n_dev, st = rt.raster_cmds_from_assembly(c, dcmds, cap, num, bufs.meshes, nm, H.to_dev(dstate), n)
        slots, st2 = rt.cache_layout(c, cache, inst_dev, n)
        mesh_boxes = rt.mesh_bounds(c, bufs.pos, bufs.meshes, nm)
        streams = rt.raster_streams(bufs.pos, bufs.color, bufs.idx, nv, ni, uv_dev=uv, uv_bytes=4)
        cmd_boxes, st3 = rt.command_bounds(c, streams, cmds, cap, dev_num_cmds=n_dev)
        white = CH.DevScene(CH.scene("relative"))   # its one image: 2 x 2 white texels
        kw = dict(images_dev=white.images, num_images=1, clear_color=CLEAR, dev_num_cmds=n_dev)

        def full():
            for _ in range(3):
                image = torch.full((Hh, S), 0x11223344, dtype=torch.int32, device="cuda:0")
                _, status = rt.raster_commands(c, streams, cmds, cap, W, Hh, image=image, **kw)
                torch.cuda.synchronize()
                if int(status.item()) != GROWN:
                    break
            assert int(status.item()) == OK
            return image

        image0 = full()
        torch.cuda.synchronize()
        assert [int(s.item()) for s in (st, st2, st3)] == [OK] * 3
        assert int((image0[:, :W].cpu().numpy().view(np.uint32) != CLEAR).sum()) > 800
        # which command holds a mesh: the draw commands' first_mesh ascends
        first = dcmds.cpu().numpy()[:ncmd * 48].view(capi.drawcmd_dtype)["first_mesh"].astype(np.int64)
        hslots = slots.cpu().numpy().view(capi.cache_slot_dtype)["first_mesh"].astype(np.int64)
        dirty = np.array([2, 6, 9], dtype=np.uint32)
        touched = sorted({int(np.searchsorted(first, m, side="right") - 1) for d in dirty for m in range(hslots[d], hslots[d + 1])})
        assert len(touched) < ncmd
        inst1 = inst.copy()
        inst1["mtx"][2][4:6] += (21.0, 9.0)
        inst1["mtx"][6][4:6] += (-13.0, -17.0)
        inst1["color"][9] = 0xFF20E0E0
        inst1_dev, dirty_dev = H.to_dev(inst1), H.to_dev(dirty)
        bits = torch.zeros(rt.damage_words(W, Hh), dtype=torch.int32, device="cuda:0")
        s4 = rt.damage_instances(c, mesh_boxes, nm, slots, n, dirty_dev, 3, W, Hh, bits)
        s5 = rt.cache_update(c, cache, inst1_dev, n, slots, dirty_dev, 3, bufs.pos, bufs.color, nv, nm, mesh_bounds=mesh_boxes)
        s6 = rt.damage_instances(c, mesh_boxes, nm, slots, n, dirty_dev, 3, W, Hh, bits)
        _, s7 = rt.command_bounds(c, streams, cmds, cap, cmd_begin=touched[0], cmd_end=touched[-1] + 1, dev_num_cmds=n_dev, bounds_dev=cmd_boxes)
        image1 = image0.clone()
        _, s8 = rt.raster_commands_damaged(c, streams, cmds, cap, W, Hh, bits, image1, bounds_dev=cmd_boxes, **kw)
        torch.cuda.synchronize()
        assert [int(s.item()) for s in (s4, s5, s6, s7, s8)] == [OK] * 5
        fresh, _ = rt.command_bounds(c, streams, cmds, cap, dev_num_cmds=n_dev)
        want = full()
        assert torch.equal(fresh, cmd_boxes)   # the refresh of the touched range leaves the whole table true
        assert torch.equal(image1, want) and not torch.equal(want, image0)
        marked = DM.marked(bits.cpu().numpy().view(np.uint32), W, Hh)
        assert 1 <= marked < 6 * 4
        # without the boxes: the same bytes
        image2 = image0.clone()
        _, s9 = rt.raster_commands_damaged(c, streams, cmds, cap, W, Hh, bits, image2, **kw)
        torch.cuda.synchronize()
        assert int(s9.item()) == OK and torch.equal(image2, want)
    finally:
        c.close()
