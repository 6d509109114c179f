"""CPU: the lane code of the damage redraw (csrc/vgx_damage.h and the frame-level host loop, through libvgx_hosttest.so: vgxt_damage_meshes,
vgxt_damage_instances, vgxt_raster_damaged) against the numpy statement (tests/damage_model.py), and the property that matters without
the model: after mark -> vgxt_cache_update -> mark -> vgxt_raster_damaged the image equals a full vgxt_raster_concave of the edited frame.
tests/test_gpu_damage.py makes the same comparisons on the kernels."""
import ctypes as C

import numpy as np
import pytest

import damage_model as DM
import raster_concave_model as K
import raster_model as R
import test_raster_concave_cpu as ccpu
import test_raster_cpu as base
import test_raster_frame_cpu as fcpu
import test_raster_painted_cpu as pcpu
import test_raster_textured_cpu as tcpu

capi = R.capi
CLEAR = DM.CLEAR
F = np.float32


def load_host():
    lib = ccpu.load_host()
    if not hasattr(lib, "vgxt_raster_damaged"):  # a library from before these calls: build again
        import __graft_entry__ as g
        g.build()
        lib = ccpu.load_host()
    lib.vgxt_damage_words.restype = C.c_uint64
    lib.vgxt_damage_words.argtypes = [C.c_uint32, C.c_uint32]
    lib.vgxt_damage_meshes.restype = C.c_int
    lib.vgxt_damage_meshes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(capi.RasterTarget), C.c_void_p]
    lib.vgxt_damage_instances.restype = C.c_int
    lib.vgxt_damage_instances.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(capi.RasterTarget), C.c_void_p]
    lib.vgxt_raster_damaged.restype = C.c_int
    lib.vgxt_raster_damaged.argtypes = ccpu.LEVEL_ARGS[:8] + [C.POINTER(capi.RasterDamage), C.c_void_p]
    lib.vgxt_cache_update.restype = C.c_int
    lib.vgxt_cache_update.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(capi.UpdateFrame)]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


def mark_target(width, height, x0, y0):
    return capi.RasterTarget(None, width, height, width, x0, y0, (C.c_uint32 * 4)(0, 0, width, height), 0, 0)


GUARD = 0xC3C3C3C3


def guarded_bits(width, height, fill=0):
    """(whole array with one guard word on either side, the view the call gets)."""
    n = DM.words(width, height)
    a = np.full(n + 2, GUARD, dtype=np.uint32)
    a[1:n + 1] = fill
    return a, a[1:n + 1]


def host_mark_meshes(host, bounds, begin, end, nm, width, height, x0, y0, bits):
    t = mark_target(width, height, x0, y0)
    b = np.ascontiguousarray(bounds, dtype=F)
    assert host.vgxt_damage_meshes(b.ctypes.data, begin, end, nm, C.byref(t), bits.ctypes.data) == capi.VGX_OK


def host_mark_instances(host, bounds, nm, slots, ninst, dirty, limit, width, height, x0, y0, bits):
    t = mark_target(width, height, x0, y0)
    b, s, d = np.ascontiguousarray(bounds, dtype=F), np.ascontiguousarray(slots), np.ascontiguousarray(dirty, dtype=np.uint32)
    lim = None if limit is None else np.array([limit], dtype=np.uint64)
    return host.vgxt_damage_instances(b.ctypes.data, nm, s.ctypes.data, ninst, d.ctypes.data if d.size else None, d.shape[0],
                                      None if lim is None else lim.ctypes.data, C.byref(t), bits.ctypes.data)


def host_damaged(host, f, tgt, bits, image=None, begin=0, end=2**64 - 1, want=capi.VGX_OK, max_entries=0):
    """vgxt_raster_damaged over the target's background (or `image`, changed in place); returns the image."""
    img = tgt.background() if image is None else image
    rec = tcpu.image_records(f.images)
    g, p = np.ascontiguousarray(f.gradients), np.ascontiguousarray(f.patterns)
    d, s, t = f.desc(), fcpu.draws_struct(f), tgt.struct(img.ctypes.data)
    x = capi.RasterTextures(f.uv.ctypes.data, rec.ctypes.data if len(f.images) else None, 8 if f.uv.dtype == np.float32 else 4, len(f.images))
    pt = pcpu.paints_struct(g, p)
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    dm = capi.RasterDamage(bits.ctypes.data, max_entries, 0)
    status = np.full(1, 77, dtype=np.uint32)
    assert host.vgxt_raster_damaged(C.byref(d), None, begin, end, C.byref(s), C.byref(x), C.byref(pt), C.byref(t), C.byref(dm), status.ctypes.data) == capi.VGX_OK
    assert status[0] == want
    return img


# ---- marking ------------------------------------------------------------------------------------------------------------------------
def test_words(host):
    for w, h in ((0, 0), (1, 1), (16, 16), (17, 16), (40, 24), (528, 20), (512, 16), (513, 16), (4096, 4096), (16384, 16384)):
        assert host.vgxt_damage_words(w, h) == DM.words(w, h), (w, h)


@pytest.mark.parametrize("case", DM.mark_cases(), ids=lambda c: c[0])
def test_mark_meshes_equals_model(host, case):
    assert DM.mark_case_conditions()
    name, width, height, x0, y0, boxes = case
    bounds = np.array(boxes, dtype=F)
    nm = bounds.shape[0]
    want = DM.mark_meshes(np.zeros(DM.words(width, height), np.uint32), bounds, 0, nm, nm, width, height, x0, y0)
    whole, bits = guarded_bits(width, height)
    host_mark_meshes(host, bounds, 0, 2**64 - 1, nm, width, height, x0, y0, bits)
    assert np.array_equal(bits, want) and whole[0] == GUARD and whole[-1] == GUARD
    for k in range(nm):  # box by box, and a range cut by num_meshes
        one = np.zeros_like(want)
        host_mark_meshes(host, bounds, k, k + 1, nm, width, height, x0, y0, one)
        assert np.array_equal(one, DM.mark_meshes(np.zeros_like(want), bounds, k, k + 1, nm, width, height, x0, y0)), (name, k)
    cut = np.zeros_like(want)
    host_mark_meshes(host, bounds, 1, 99, nm - 1, width, height, x0, y0, cut)
    assert np.array_equal(cut, DM.mark_meshes(np.zeros_like(want), bounds, 1, 99, nm - 1, width, height, x0, y0))
    # bits set before the call stay set
    _, pre = guarded_bits(width, height, fill=0x00010004 & int(DM.all_bits(width, height)[0]))
    keep = pre.copy()
    host_mark_meshes(host, bounds, 0, nm, nm, width, height, x0, y0, pre)
    assert np.array_equal(pre, want | keep)


@pytest.mark.parametrize("kind", sorted(DM.dirty_lists()))
def test_mark_instances_equals_model(host, kind):
    bounds, slots, width, height, x0, y0 = DM.list_scene()
    dirty, limit, status = DM.dirty_lists()[kind]
    nm, ninst = bounds.shape[0], slots.shape[0] - 1
    want = np.zeros(DM.words(width, height), np.uint32)
    assert DM.mark_instances(want, bounds, nm, slots, ninst, dirty, limit, width, height, x0, y0) == status
    whole, bits = guarded_bits(width, height)
    assert host_mark_instances(host, bounds, nm, slots, ninst, dirty, limit, width, height, x0, y0, bits) == status
    assert np.array_equal(bits, want) and whole[0] == GUARD and whole[-1] == GUARD
    if kind in ("empty", "culled", "limit_zero"):
        assert not want.any()
    else:
        assert 0 < DM.marked(want, width, height)
    if kind == "one_big":
        assert int(slots["first_mesh"][41]) - int(slots["first_mesh"][40]) == 300


def test_slot_pairs_outside_the_table(host):
    """slots[d + 1].first_mesh > num_meshes, and a decreasing pair: invalid, skipped, the valid entries still marked."""
    bounds, slots, width, height, x0, y0 = DM.list_scene()
    ninst = slots.shape[0] - 1
    dirty = np.array([2, 49, 3], dtype=np.uint32)
    short = int(slots["first_mesh"][49])  # the table ends before instance 49's mesh
    want = np.zeros(DM.words(width, height), np.uint32)
    assert DM.mark_instances(want, bounds, short, slots, ninst, dirty, None, width, height, x0, y0) == capi.VGX_E_INVALID_ARG
    bits = np.zeros_like(want)
    assert host_mark_instances(host, bounds, short, slots, ninst, dirty, None, width, height, x0, y0, bits) == capi.VGX_E_INVALID_ARG
    assert np.array_equal(bits, want) and want.any()
    bad = slots.copy()
    bad["first_mesh"][11] = 5  # < slots[10].first_mesh
    want = np.zeros_like(want)
    assert DM.mark_instances(want, bounds, bounds.shape[0], bad, ninst, np.array([10, 12], np.uint32), None, width, height, x0, y0) == capi.VGX_E_INVALID_ARG
    bits = np.zeros_like(want)
    assert host_mark_instances(host, bounds, bounds.shape[0], bad, ninst, np.array([10, 12], np.uint32), None, width, height, x0, y0, bits) == capi.VGX_E_INVALID_ARG
    assert np.array_equal(bits, want)


# ---- the restricted raster ---------------------------------------------------------------------------------------------------------------
FRAMES = ("state", "classes", "crowd", "inner")


@pytest.mark.parametrize("name", FRAMES)
def test_all_bits_equals_the_full_call(host, name):
    f = K.frame(name)
    t = f.target
    for tgt in (t, t.with_clear(CLEAR)):
        full = ccpu.host_level(host, "vgxt_raster_concave", f, tgt)
        assert np.array_equal(host_damaged(host, f, tgt, DM.all_bits(t.width, t.height)), full)
        assert np.array_equal(full, K.expected(name, tgt.clear is not None))


@pytest.mark.parametrize("name", FRAMES)
def test_no_bit_and_checkerboard(host, name):
    f = K.frame(name)
    t = f.target
    tgt = t.with_clear(CLEAR)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    none = np.zeros(DM.words(t.width, t.height), np.uint32)
    assert np.array_equal(host_damaged(host, f, tgt, none, image=sentinel.copy()), sentinel)
    for phase in (0, 1):
        bits = DM.checkerboard(t.width, t.height, phase)
        got = host_damaged(host, f, tgt, bits, image=sentinel.copy())
        want = DM.render_damaged(f, tgt, sentinel.copy(), bits)
        assert np.array_equal(got, want), base.where(got, want)
        m = DM.tile_mask(bits, tgt)
        sx0, sy0, sx1, sy1 = tgt.scissor
        inside = np.zeros_like(m)
        inside[sy0:sy1, sx0:sx1] = True
        assert (got[~(m & inside)] == DM.SENTINEL).all() and (got[m & inside] != DM.SENTINEL).all()
        assert np.array_equal(got[m & inside], K.expected(name, True)[m & inside])
        # without the clear: over the background, the unmarked tiles keep it
        got = host_damaged(host, f, t, bits)
        assert np.array_equal(got, DM.render_damaged(f, t, t.background(), bits))


def test_marked_tile_cut_by_the_scissor(host):
    f = K.frame("state")
    t = f.target
    tgt = R.Target(t.width, t.height, t.stride, t.x0, t.y0, scissor=(5, 3, 41, 27), clear=CLEAR)
    bits = DM.checkerboard(t.width, t.height)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    got = host_damaged(host, f, tgt, bits, image=sentinel.copy())
    assert np.array_equal(got, DM.render_damaged(f, tgt, sentinel.copy(), bits))
    assert (got[3:16, 5:16] != DM.SENTINEL).all() and (got[:3] == DM.SENTINEL).all() and (got[3:16, 16:32] == DM.SENTINEL).all()


def test_invalid_draw_with_no_bit_set(host):
    g = K.state_frame()
    g.meshes["draw"][4] = 99
    tgt = g.target.with_clear(CLEAR)
    for bits in (np.zeros(DM.words(tgt.width, tgt.height), np.uint32), DM.all_bits(tgt.width, tgt.height)):
        assert np.array_equal(host_damaged(host, g, tgt, bits, want=capi.VGX_E_INVALID_ARG), tgt.background())


def test_mesh_range(host):
    f = K.frame("state")
    bits = DM.checkerboard(f.target.width, f.target.height, 1)
    for begin, end in ((0, 3), (2, 5), (3, 99)):
        want = DM.render_damaged(f, f.target, f.target.background(), bits, begin, end)
        assert np.array_equal(host_damaged(host, f, f.target, bits, begin=begin, end=end), want)


# ---- the property, without the model ----------------------------------------------------------------------------------------------------------
class HostScene:
    """The chain on host arrays: vgxt_damage_instances, vgxt_cache_update, vgxt_raster_damaged / vgxt_raster_concave."""

    def __init__(self, host):
        self.host = host
        self.cache = DM.scene_cache()
        c = self.cache
        self.cdesc = capi.CacheDesc(c.pos.ctypes.data, c.color.ctypes.data, c.idx.ctypes.data, c.meshes.ctypes.data, c.meshes.shape[0], c.pos.shape[0], c.idx.shape[0])
        self.inst = DM.scene_instances()
        self.f, self.slots = DM.scene_frame(self.cache, self.inst)
        self.bounds = np.zeros((self.f.nm, 4), dtype=F)
        host.vgxt_mesh_bounds(self.f.pos.ctypes.data, self.f.meshes.ctypes.data, self.f.nm, self.bounds.ctypes.data)
        self.tgt = self.f.target.with_clear(CLEAR)

    def full(self):
        return ccpu.host_level(self.host, "vgxt_raster_concave", self.f, self.tgt)

    def mark(self, dirty, bits):
        t = self.tgt
        assert host_mark_instances(self.host, self.bounds, self.f.nm, self.slots, self.inst.shape[0], dirty, None, t.width, t.height, t.x0, t.y0, bits) == capi.VGX_OK

    def update(self, inst, dirty):
        self.inst = inst
        fr = capi.UpdateFrame(self.f.pos.ctypes.data, self.f.color.ctypes.data, self.f.nv, self.f.nm, self.bounds.ctypes.data)
        d = np.ascontiguousarray(dirty, dtype=np.uint32)
        assert self.host.vgxt_cache_update(C.byref(self.cdesc), inst.ctypes.data, inst.shape[0], self.slots.ctypes.data, d.ctypes.data, d.shape[0], None,
                                           C.byref(fr)) == capi.VGX_OK

    def damaged(self, image, bits):
        return host_damaged(self.host, self.f, self.tgt, bits, image=image)

    def zero_bits(self):
        return np.zeros(DM.words(self.tgt.width, self.tgt.height), np.uint32)


def check_property(scene):
    """Shared with the GPU test, which hands in a scene over the kernels. Every step: mark the old boxes, update, mark the new boxes,
    redraw the marked tiles over the previous image; the result equals a full render of the edited frame on the whole buffer. Then the
    control: the same step with the new boxes alone leaves a stale pixel."""
    marks = DM.scene_marks()
    assert DM.scene_conditions(marks)
    image = scene.full()
    assert int((image != scene.tgt.background()).sum()) > 2000
    stale_seen = 0
    for name, dirty, both, new, inst1 in marks:
        before = image.copy()
        bits = scene.zero_bits()
        scene.mark(dirty, bits)
        scene.update(inst1, dirty)
        only_new = scene.zero_bits()
        scene.mark(dirty, only_new)
        scene.mark(dirty, bits)
        got_bits, got_new = scene.read_bits(bits), scene.read_bits(only_new)
        assert np.array_equal(got_bits, both), name
        assert np.array_equal(got_new, new), name
        n = DM.marked(got_bits, scene.tgt.width, scene.tgt.height)
        tw, th = DM.tiles_wh(scene.tgt.width, scene.tgt.height)
        assert 1 <= n < tw * th, (name, n)
        image = scene.damaged(image, bits)
        want = scene.full()
        assert np.array_equal(image, want), (name, base.where(image, want))
        assert not np.array_equal(want, before), name  # the edit shows
        control = scene.damaged(before.copy(), only_new)
        stale_seen += int(not np.array_equal(control, want))
        assert R.guards_intact(scene.tgt, image)
    assert stale_seen >= 3  # the check can see a stale pixel: skipping the old boxes is found out


def test_property_through_the_lane_code(host):
    scene = HostScene(host)
    scene.read_bits = lambda b: b
    check_property(scene)
