"""GPU: the damage redraw on the device -- k_damage_meshes / k_damage_instances (csrc/vgx_damage.hip) and the DAMAGE instantiations of the
frame-level raster kernels (csrc/vgx_raster.hip, vgx_raster_damaged) -- against the numpy statement (tests/damage_model.py) and the lane
code, with guard words around the bit array and the image; the sort window and its VGX_E_GROWN protocol; and the property that matters,
product against product: after mark -> vgx_cache_update -> mark -> vgx_raster_damaged the image equals vgx_raster_concave of the edited
frame on the whole buffer (check_damage_property of tests/raster_harness.py, run here over the kernels). Every comparison is np.array_equal."""
import ctypes as C
import types

import numpy as np
import pytest

import damage_model as DM
import raster_concave_model as K
import raster_harness as H
import raster_model as R
from raster_harness import DevBits, dev_parts, gpu_bounds, gpu_level, host, rt, to_dev, warm_ctx, where  # noqa: F401 (host, rt, warm_ctx: fixtures)

pytestmark = pytest.mark.gpu
capi = R.capi
CLEAR = DM.CLEAR
F = np.float32


def dev_bits(bits, width, height):
    return DevBits(width, height, fill=bits)


def gpu_mark_meshes(rt, ctx, bounds_dev, begin, end, nm, width, height, x0, y0, bits):
    t = H.mark_target(width, height, x0, y0)
    assert rt.lib().vgx_damage_meshes(ctx.handle, bounds_dev.data_ptr(), begin, end, nm, C.byref(t), bits.t.data_ptr(), rt._stream_ptr()) == capi.VGX_OK


def gpu_mark_instances(rt, ctx, bounds_dev, nm, slots_dev, ninst, dirty, limit, width, height, x0, y0, bits):
    """Returns dev_status (synchronised); a 77 in the words beside it stays."""
    import torch
    t = H.mark_target(width, height, x0, y0)
    dd = to_dev(np.ascontiguousarray(dirty, dtype=np.uint32))
    lim = None if limit is None else torch.tensor([int(limit)], dtype=torch.int64, device="cuda:0")
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
    assert rt.lib().vgx_damage_instances(ctx.handle, bounds_dev.data_ptr(), nm, slots_dev.data_ptr(), ninst, dd.data_ptr() if dirty.shape[0] else None,
                                         dirty.shape[0], None if lim is None else lim.data_ptr(), C.byref(t), bits.t.data_ptr(), status[1:].data_ptr(),
                                         rt._stream_ptr()) == capi.VGX_OK
    torch.cuda.synchronize()
    s = status.cpu().tolist()
    assert s[0] == 77 and s[2] == 77
    return s[1]


def sentinel_image(tgt):
    import torch
    return torch.from_numpy(np.full((tgt.rows(), tgt.stride), DM.SENTINEL, dtype=np.uint32).view(np.int32)).to("cuda:0")


# ---- marking ------------------------------------------------------------------------------------------------------------------------
def test_words(rt):
    for w, h in ((0, 0), (1, 1), (16, 16), (17, 16), (40, 24), (528, 20), (512, 16), (513, 16), (4096, 4096), (16384, 16384)):
        assert rt.damage_words(w, h) == DM.words(w, h), (w, h)


@pytest.mark.parametrize("case", DM.mark_cases(), ids=lambda c: c[0])
def test_mark_meshes_equals_model_and_lane_code(rt, warm_ctx, host, case):
    import torch
    assert DM.mark_case_conditions()
    name, width, height, x0, y0, boxes = case
    bounds = np.array(boxes, dtype=F)
    nm = bounds.shape[0]
    bd = torch.from_numpy(bounds).to("cuda:0")
    want = DM.mark_meshes(np.zeros(DM.words(width, height), np.uint32), bounds, 0, nm, nm, width, height, x0, y0)
    lane = np.zeros_like(want)
    H.host_mark_meshes(host, bounds, 0, nm, nm, width, height, x0, y0, lane)
    assert np.array_equal(lane, want)
    bits = DevBits(width, height)
    gpu_mark_meshes(rt, warm_ctx, bd, 0, 2**64 - 1, nm, width, height, x0, y0, bits)
    first = bits.read()
    assert np.array_equal(first, want), (name, first, want)
    gpu_mark_meshes(rt, warm_ctx, bd, 0, nm, nm, width, height, x0, y0, bits)
    assert np.array_equal(bits.read(), want)  # two runs, the same words
    for k in range(nm):
        one = DevBits(width, height)
        gpu_mark_meshes(rt, warm_ctx, bd, k, k + 1, nm, width, height, x0, y0, one)
        assert np.array_equal(one.read(), DM.mark_meshes(np.zeros_like(want), bounds, k, k + 1, nm, width, height, x0, y0)), (name, k)
    cut = DevBits(width, height)
    gpu_mark_meshes(rt, warm_ctx, bd, 1, 99, nm - 1, width, height, x0, y0, cut)   # the range cut by num_meshes
    assert np.array_equal(cut.read(), DM.mark_meshes(np.zeros_like(want), bounds, 1, 99, nm - 1, width, height, x0, y0))
    keep = np.uint32(0x00010004) & DM.all_bits(width, height)
    pre = dev_bits(keep, width, height)
    gpu_mark_meshes(rt, warm_ctx, bd, 0, nm, nm, width, height, x0, y0, pre)
    assert np.array_equal(pre.read(), want | keep)  # bits set before the call stay set
    assert np.array_equal(bd.cpu().numpy().view(np.uint32), bounds.view(np.uint32))


def test_mark_meshes_through_the_runtime(rt, warm_ctx):
    import torch
    name, width, height, x0, y0, boxes = DM.mark_cases()[-1]
    bounds = np.array(boxes, dtype=F)
    bits = torch.zeros(rt.damage_words(width, height), dtype=torch.int32, device="cuda:0")
    rt.damage_meshes(warm_ctx, torch.from_numpy(bounds).to("cuda:0"), bounds.shape[0], width, height, bits, x0=x0, y0=y0)
    torch.cuda.synchronize()
    want = DM.mark_meshes(np.zeros(DM.words(width, height), np.uint32), bounds, 0, 99, bounds.shape[0], width, height, x0, y0)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("kind", sorted(DM.dirty_lists()))
def test_mark_instances_equals_model_and_lane_code(rt, warm_ctx, host, kind):
    import torch
    bounds, slots, width, height, x0, y0 = DM.list_scene()
    dirty, limit, status = DM.dirty_lists()[kind]
    nm, ninst = bounds.shape[0], slots.shape[0] - 1
    want = np.zeros(DM.words(width, height), np.uint32)
    assert DM.mark_instances(want, bounds, nm, slots, ninst, dirty, limit, width, height, x0, y0) == status
    lane = np.zeros_like(want)
    assert H.host_mark_instances(host, bounds, nm, slots, ninst, dirty, limit, width, height, x0, y0, lane) == status and np.array_equal(lane, want)
    bd, sd = torch.from_numpy(bounds).to("cuda:0"), to_dev(slots)
    bits = DevBits(width, height)
    assert gpu_mark_instances(rt, warm_ctx, bd, nm, sd, ninst, dirty, limit, width, height, x0, y0, bits) == status
    first = bits.read()
    assert np.array_equal(first, want), (kind, first, want)
    assert gpu_mark_instances(rt, warm_ctx, bd, nm, sd, ninst, dirty, limit, width, height, x0, y0, bits) == status
    assert np.array_equal(bits.read(), want)  # two runs, the same words
    keep = np.uint32(0x80000001) & DM.all_bits(width, height)
    pre = dev_bits(keep, width, height)
    assert gpu_mark_instances(rt, warm_ctx, bd, nm, sd, ninst, dirty, limit, width, height, x0, y0, pre) == status
    assert np.array_equal(pre.read(), want | keep)


def test_slot_pairs_outside_the_table(rt, warm_ctx):
    import torch
    bounds, slots, width, height, x0, y0 = DM.list_scene()
    ninst = slots.shape[0] - 1
    bd = torch.from_numpy(bounds).to("cuda:0")
    dirty = np.array([2, 49, 3], dtype=np.uint32)
    short = int(slots["first_mesh"][49])
    want = np.zeros(DM.words(width, height), np.uint32)
    assert DM.mark_instances(want, bounds, short, slots, ninst, dirty, None, width, height, x0, y0) == capi.VGX_E_INVALID_ARG
    bits = DevBits(width, height)
    assert gpu_mark_instances(rt, warm_ctx, bd, short, to_dev(slots), ninst, dirty, None, width, height, x0, y0, bits) == capi.VGX_E_INVALID_ARG
    assert np.array_equal(bits.read(), want) and want.any()
    bad = slots.copy()
    bad["first_mesh"][11] = 5
    d2 = np.array([10, 12], np.uint32)
    want = np.zeros_like(want)
    assert DM.mark_instances(want, bounds, bounds.shape[0], bad, ninst, d2, None, width, height, x0, y0) == capi.VGX_E_INVALID_ARG
    bits = DevBits(width, height)
    assert gpu_mark_instances(rt, warm_ctx, bd, bounds.shape[0], to_dev(bad), ninst, d2, None, width, height, x0, y0, bits) == capi.VGX_E_INVALID_ARG
    assert np.array_equal(bits.read(), want)


# ---- the restricted raster ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.DAMAGE_FRAMES)
def test_all_bits_equals_the_full_call(rt, warm_ctx, name):
    f = K.frame(name)
    t = f.target
    df, ds, dx, dp = dev_parts(f)
    bits = dev_bits(DM.all_bits(t.width, t.height), t.width, t.height)
    for tgt in (t, t.with_clear(CLEAR)):
        _, full = gpu_level(rt, warm_ctx, "vgx_raster_concave", df, ds, dx, dp, tgt)
        _, got = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, tgt, bits=bits)
        assert np.array_equal(got, full), where(got, full)
        assert np.array_equal(got, K.expected(name, tgt.clear is not None))
        _, given = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, tgt, bits=bits, bounds=gpu_bounds(rt, warm_ctx, df))
        assert np.array_equal(given, full)
    bits.read()
    assert df.unchanged()


@pytest.mark.parametrize("name", H.DAMAGE_FRAMES)
def test_no_bit_and_checkerboard(rt, warm_ctx, host, name):
    f = K.frame(name)
    t = f.target
    tgt = t.with_clear(CLEAR)
    df, ds, dx, dp = dev_parts(f)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    _, got = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, tgt, bits=DevBits(t.width, t.height), image=sentinel_image(tgt))
    assert np.array_equal(got, sentinel)  # no bit set: nothing is written, the clear included
    for phase in (0, 1):
        host_bits = DM.checkerboard(t.width, t.height, phase)
        bits = dev_bits(host_bits, t.width, t.height)
        _, got = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, tgt, bits=bits, image=sentinel_image(tgt))
        want = DM.render_damaged(f, tgt, sentinel.copy(), host_bits)
        assert np.array_equal(got, want), where(got, want)
        assert np.array_equal(got, H.host_level(host, "damaged", f, tgt, bits=host_bits, image=sentinel.copy()))
        m = DM.tile_mask(host_bits, tgt)
        sx0, sy0, sx1, sy1 = tgt.scissor
        inside = np.zeros_like(m)
        inside[sy0:sy1, sx0:sx1] = True
        assert (got[~(m & inside)] == DM.SENTINEL).all() and np.array_equal(got[m & inside], K.expected(name, True)[m & inside])
        _, again = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, tgt, bits=bits, image=sentinel_image(tgt))
        assert np.array_equal(again, got)
        _, over = gpu_level(rt, warm_ctx, "damaged", df, ds, dx, dp, t, bits=bits)  # without the clear, over the background
        assert np.array_equal(over, DM.render_damaged(f, t, t.background(), host_bits))
        assert np.array_equal(bits.read(), host_bits)
    if name == "crowd":
        assert f.nm > 256 and DM.bit_set(DM.checkerboard(t.width, t.height, 0), 1 * DM.tiles_wh(t.width, t.height)[0] + 1)  # more than 256 meshes on a marked tile


def test_marked_tile_cut_by_the_scissor(rt, warm_ctx):
    f = K.frame("state")
    t = f.target
    tgt = R.Target(t.width, t.height, t.stride, t.x0, t.y0, scissor=(5, 3, 41, 27), clear=CLEAR)
    host_bits = DM.checkerboard(t.width, t.height)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    _, got = gpu_level(rt, warm_ctx, "damaged", *dev_parts(f), tgt, bits=dev_bits(host_bits, t.width, t.height), image=sentinel_image(tgt))
    assert np.array_equal(got, DM.render_damaged(f, tgt, sentinel.copy(), host_bits))
    assert (got[3:16, 5:16] != DM.SENTINEL).all() and (got[:3] == DM.SENTINEL).all() and (got[3:16, 16:32] == DM.SENTINEL).all()


def test_invalid_draw_with_no_bit_set_and_mesh_ranges(rt, warm_ctx):
    g = K.state_frame()
    g.meshes["draw"][4] = 99
    tgt = g.target.with_clear(CLEAR)
    parts = dev_parts(g)
    for host_bits in (np.zeros(DM.words(tgt.width, tgt.height), np.uint32), DM.all_bits(tgt.width, tgt.height)):
        _, got = gpu_level(rt, warm_ctx, "damaged", *parts, tgt, bits=dev_bits(host_bits, tgt.width, tgt.height), want=capi.VGX_E_INVALID_ARG)
        assert np.array_equal(got, tgt.background())
    f = K.frame("state")
    host_bits = DM.checkerboard(f.target.width, f.target.height, 1)
    bits = dev_bits(host_bits, f.target.width, f.target.height)
    for begin, end in ((0, 3), (2, 5), (3, 99)):
        _, got = gpu_level(rt, warm_ctx, "damaged", *dev_parts(f), f.target, bits=bits, begin=begin, end=end)
        assert np.array_equal(got, DM.render_damaged(f, f.target, f.target.background(), host_bits, begin, end))


def test_host_refusals(rt, warm_ctx):
    f = K.frame("state")
    df, ds, dx, dp = dev_parts(f)
    import torch
    image = torch.zeros((f.target.rows(), f.target.stride), dtype=torch.int32, device="cuda:0")
    t = f.target.struct(image.data_ptr())
    bits = DevBits(f.target.width, f.target.height)
    call = lambda dm: rt.lib().vgx_raster_damaged(warm_ctx.handle, C.byref(df.desc), None, 0, 99, C.byref(ds.struct), C.byref(dx.struct), C.byref(dp.struct),
                                                  C.byref(t), dm, None, rt._stream_ptr())
    assert call(None) == capi.VGX_E_INVALID_ARG
    assert call(C.byref(capi.RasterDamage(None, 0, 0))) == capi.VGX_E_INVALID_ARG
    assert call(C.byref(capi.RasterDamage(bits.t.data_ptr() + 2, 0, 0))) == capi.VGX_E_INVALID_ARG
    assert call(C.byref(capi.RasterDamage(bits.t.data_ptr(), 0, 1))) == capi.VGX_E_INVALID_ARG
    mt = H.mark_target(40, 24, 0, 0)
    bd = torch.zeros((4, 4), dtype=torch.float32, device="cuda:0")
    lib = rt.lib()
    assert lib.vgx_damage_meshes(warm_ctx.handle, bd.data_ptr(), 0, 4, 4, C.byref(mt), None, rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_damage_meshes(warm_ctx.handle, bd.data_ptr() + 4, 0, 4, 4, C.byref(mt), bits.t.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_damage_meshes(warm_ctx.handle, bd.data_ptr(), 0, 4, 2**32, C.byref(mt), bits.t.data_ptr(), rt._stream_ptr()) == capi.VGX_E_RANGE
    assert lib.vgx_damage_meshes(warm_ctx.handle, bd.data_ptr(), 0, 4, 4, None, bits.t.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    torch.cuda.synchronize()
    assert not bits.read().any()


# ---- the sort window ---------------------------------------------------------------------------------------------------------------------
def test_max_entries_too_small_grows_then_succeeds(rt):
    """A window of two entries: VGX_E_GROWN with nothing written, the clear included; the same call repeated reaches VGX_OK. A full render
    in between leaves the damaged call's window alone."""
    ctx = rt.Context(0)
    rt.raster_reserve(ctx, 8192, 1 << 17)
    try:
        f = K.frame("state")
        tgt = f.target.with_clear(CLEAR)
        parts = dev_parts(f)
        bits = dev_bits(DM.all_bits(tgt.width, tgt.height), tgt.width, tgt.height)
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, want=capi.VGX_E_GROWN, max_entries=2)
        assert np.array_equal(got, tgt.background())
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, max_entries=2)
        assert np.array_equal(got, K.expected("state", True))
        _, full = gpu_level(rt, ctx, "vgx_raster_concave", *parts, tgt)
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, max_entries=0)   # the library's window: what the last damaged call measured
        assert np.array_equal(got, full)
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, max_entries=1 << 20)
        assert np.array_equal(got, full)
    finally:
        ctx.close()


def many_quads(n=1100, side=64):
    """n translucent quads over a whole side x side image: n x 16 bin entries, more than the initial window of 16384."""
    import raster_frame_model as M
    rs = np.random.RandomState(3)
    b = K.Builder()
    for k in range(n):
        b.mesh(M.quad(-1.0, -1.0, side + 1.0, side + 1.0), (8 << 24) | int(rs.randint(0, 1 << 24)), M.QUAD)
    return K.finish(b.frame("many_quads", R.Target(side, side, side + 1, 0, 0)))


def test_library_window_on_a_fresh_context_converges_within_two_calls(rt):
    ctx = rt.Context(0)
    try:
        f = many_quads()
        assert f.nm * 16 > 16384
        tgt = f.target.with_clear(CLEAR)
        parts = dev_parts(f)
        bits = dev_bits(DM.all_bits(tgt.width, tgt.height), tgt.width, tgt.height)
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, want=capi.VGX_E_GROWN, max_entries=0)
        assert np.array_equal(got, tgt.background())
        _, got = gpu_level(rt, ctx, "damaged", *parts, tgt, bits=bits, max_entries=0)
        status = capi.VGX_E_GROWN
        for _ in range(3):
            if status != capi.VGX_E_GROWN:
                break
            import torch
            image = torch.from_numpy(tgt.background().view(np.int32)).to("cuda:0")
            image, st = rt.raster_concave(ctx, parts[0].desc, parts[1].t[0], parts[1].t[1], f.draws.shape[0], parts[2].t[0], 8, None, 0, None, 0, None, 0,
                                          tgt.width, tgt.height, clear_color=CLEAR, image=image)
            torch.cuda.synchronize()
            status = int(st.item())
        assert status == capi.VGX_OK
        assert np.array_equal(got, image.cpu().numpy().view(np.uint32))
        # a small frame on a fresh context: the initial window holds it at once
        g = K.frame("classes")
        ctx2 = rt.Context(0)
        try:
            tg = g.target.with_clear(CLEAR)
            _, got = gpu_level(rt, ctx2, "damaged", *dev_parts(g), tg, bits=dev_bits(DM.all_bits(tg.width, tg.height), tg.width, tg.height), max_entries=0)
            assert np.array_equal(got, K.expected("classes", True))
        finally:
            ctx2.close()
    finally:
        ctx.close()


# ---- the property, without the model ----------------------------------------------------------------------------------------------------------
class DevCache:
    def __init__(self, c):
        self.t = [to_dev(a) for a in (c.pos, c.color, c.idx, c.meshes)]
        self.nm, self.nv, self.ni = c.meshes.shape[0], c.pos.shape[0], c.idx.shape[0]
        self.bufs = types.SimpleNamespace(pos=self.t[0])

    def desc(self):
        return capi.CacheDesc(self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(), self.nm, self.nv, self.ni)


class DevScene:
    """The chain on the device, all on one stream: vgx_cache_submit / vgx_cache_layout / vgx_mesh_bounds once, then per step
    vgx_damage_instances, vgx_cache_update, vgx_damage_instances, vgx_raster_damaged; vgx_raster_concave for the full renders."""

    def __init__(self, rt, ctx):
        import torch
        self.rt, self.ctx = rt, ctx
        c = DM.scene_cache()
        self.cache = DevCache(c)
        self.inst = DM.scene_instances()
        f, slots = DM.scene_frame(c, self.inst)   # the frame the CPU oracle submits: the device's must equal it
        self.f = f
        self.tgt = f.target.with_clear(CLEAR)
        self.bufs = rt.MeshBuffers("cuda:0", f.nv, f.ni, f.nm)
        self.inst_dev = to_dev(self.inst)
        rt.cache_submit(ctx, self.cache, self.inst_dev, self.inst.shape[0], self.bufs)
        self.slots_dev, st = rt.cache_layout(ctx, self.cache, self.inst_dev, self.inst.shape[0])
        self.bounds = rt.mesh_bounds(ctx, self.bufs.pos, self.bufs.meshes, f.nm)
        torch.cuda.synchronize()
        assert int(self.bufs.dev_status.item()) == capi.VGX_OK and int(st.item()) == capi.VGX_OK
        assert np.array_equal(self.slots_dev.cpu().numpy().view(capi.cache_slot_dtype), slots)
        assert np.array_equal(self.bufs.pos[:f.nv].cpu().numpy().view(np.uint32), f.pos.view(np.uint32))
        assert np.array_equal(self.bufs.color[:f.nv].cpu().numpy().view(np.uint32), f.color)
        gm = self.bufs.meshes[:f.nm * 32].cpu().numpy().view(capi.mesh_dtype)
        assert all(np.array_equal(gm[k], f.meshes[k]) for k in gm.dtype.names)
        self.ds, self.dx, self.dp = H.DevState(f), H.DevTex(f), H.DevPaints(f.gradients, f.patterns)
        self.df = types.SimpleNamespace(desc=rt.mesh_seq(self.bufs, f.nv, f.ni, f.nm))
        self.keep = []

    def full(self):
        return gpu_level(self.rt, self.ctx, "vgx_raster_concave", self.df, self.ds, self.dx, self.dp, self.tgt, bounds=self.bounds)[1]

    def zero_bits(self):
        return DevBits(self.tgt.width, self.tgt.height)

    def read_bits(self, bits):
        return bits.read()

    def mark(self, dirty, bits):
        t = self.tgt
        dd = to_dev(np.ascontiguousarray(dirty, dtype=np.uint32))
        st = self.rt.damage_instances(self.ctx, self.bounds, self.f.nm, self.slots_dev, self.inst.shape[0], dd, dirty.shape[0], t.width, t.height, bits.t,
                                      x0=t.x0, y0=t.y0)
        self.keep += [dd, st]   # alive until the scene goes: the calls are asynchronous
        self.statuses = getattr(self, "statuses", []) + [st]

    def update(self, inst, dirty):
        self.inst = inst
        di, dd = to_dev(inst), to_dev(np.ascontiguousarray(dirty, dtype=np.uint32))
        st = self.rt.cache_update(self.ctx, self.cache, di, inst.shape[0], self.slots_dev, dd, dirty.shape[0], self.bufs.pos, self.bufs.color, self.f.nv, self.f.nm,
                                  mesh_bounds=self.bounds)
        self.keep += [di, dd, st]
        self.statuses = getattr(self, "statuses", []) + [st]

    def damaged(self, image, bits):
        import torch
        dev = torch.from_numpy(np.ascontiguousarray(image).view(np.int32)).to("cuda:0")
        _, got = gpu_level(self.rt, self.ctx, "damaged", self.df, self.ds, self.dx, self.dp, self.tgt, bits=bits, image=dev, bounds=self.bounds)
        assert all(int(s.item()) == capi.VGX_OK for s in self.statuses)
        return got


def test_property_through_the_kernels(rt, warm_ctx):
    H.check_damage_property(DevScene(rt, warm_ctx))
