"""CPU: the lane code of the damage redraw (csrc/vgx_damage.h and the frame-level host loop, through libvgx_hosttest.so: vgxt_damage_meshes,
vgxt_damage_instances, vgxt_raster_damaged) against the numpy statement (tests/damage_model.py), and the property that matters without
the model: after mark -> vgxt_cache_update -> mark -> vgxt_raster_damaged the image equals a full vgxt_raster_concave of the edited frame.
tests/test_gpu_damage.py makes the same comparisons on the kernels."""
import ctypes as C

import numpy as np
import pytest

import damage_model as DM
import raster_concave_model as K
import raster_harness as H
import raster_model as R
from raster_harness import host, host_mark_instances, host_mark_meshes  # noqa: F401 (host: fixture)

capi = R.capi
CLEAR = DM.CLEAR
F = np.float32
GUARD = H.BITS_GUARD
FRAMES = H.DAMAGE_FRAMES


def guarded_bits(width, height, fill=0):
    """(whole array with one guard word on either side, the view the call gets)."""
    n = DM.words(width, height)
    a = np.full(n + 2, GUARD, dtype=np.uint32)
    a[1:n + 1] = fill
    return a, a[1:n + 1]


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


@pytest.mark.parametrize("name", FRAMES)
def test_all_bits_equals_the_full_call(host, name):
    f = K.frame(name)
    t = f.target
    for tgt in (t, t.with_clear(CLEAR)):
        full = H.host_level(host, "concave", f, tgt)
        assert np.array_equal(H.host_level(host, "damaged", f, tgt, bits=DM.all_bits(t.width, t.height)), full)
        assert np.array_equal(full, K.expected(name, tgt.clear is not None))


@pytest.mark.parametrize("name", FRAMES)
def test_no_bit_and_checkerboard(host, name):
    f = K.frame(name)
    t = f.target
    tgt = t.with_clear(CLEAR)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    none = np.zeros(DM.words(t.width, t.height), np.uint32)
    assert np.array_equal(H.host_level(host, "damaged", f, tgt, bits=none, image=sentinel.copy()), sentinel)
    for phase in (0, 1):
        bits = DM.checkerboard(t.width, t.height, phase)
        got = H.host_level(host, "damaged", f, tgt, bits=bits, image=sentinel.copy())
        want = DM.render_damaged(f, tgt, sentinel.copy(), bits)
        assert np.array_equal(got, want), H.where(got, want)
        m = DM.tile_mask(bits, tgt)
        sx0, sy0, sx1, sy1 = tgt.scissor
        inside = np.zeros_like(m)
        inside[sy0:sy1, sx0:sx1] = True
        assert (got[~(m & inside)] == DM.SENTINEL).all() and (got[m & inside] != DM.SENTINEL).all()
        assert np.array_equal(got[m & inside], K.expected(name, True)[m & inside])
        # without the clear: over the background, the unmarked tiles keep it
        got = H.host_level(host, "damaged", f, t, bits=bits)
        assert np.array_equal(got, DM.render_damaged(f, t, t.background(), bits))


def test_marked_tile_cut_by_the_scissor(host):
    f = K.frame("state")
    t = f.target
    tgt = R.Target(t.width, t.height, t.stride, t.x0, t.y0, scissor=(5, 3, 41, 27), clear=CLEAR)
    bits = DM.checkerboard(t.width, t.height)
    sentinel = np.full((t.rows(), t.stride), DM.SENTINEL, dtype=np.uint32)
    got = H.host_level(host, "damaged", f, tgt, bits=bits, image=sentinel.copy())
    assert np.array_equal(got, DM.render_damaged(f, tgt, sentinel.copy(), bits))
    assert (got[3:16, 5:16] != DM.SENTINEL).all() and (got[:3] == DM.SENTINEL).all() and (got[3:16, 16:32] == DM.SENTINEL).all()


def test_invalid_draw_with_no_bit_set(host):
    g = K.state_frame()
    g.meshes["draw"][4] = 99
    tgt = g.target.with_clear(CLEAR)
    for bits in (np.zeros(DM.words(tgt.width, tgt.height), np.uint32), DM.all_bits(tgt.width, tgt.height)):
        assert np.array_equal(H.host_level(host, "damaged", g, tgt, bits=bits, want=capi.VGX_E_INVALID_ARG), tgt.background())


def test_mesh_range(host):
    f = K.frame("state")
    bits = DM.checkerboard(f.target.width, f.target.height, 1)
    for begin, end in ((0, 3), (2, 5), (3, 99)):
        want = DM.render_damaged(f, f.target, f.target.background(), bits, begin, end)
        assert np.array_equal(H.host_level(host, "damaged", f, f.target, bits=bits, begin=begin, end=end), want)


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
        return H.host_level(self.host, "concave", self.f, self.tgt)

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
        return H.host_level(self.host, "damaged", self.f, self.tgt, bits=bits, image=image)

    def zero_bits(self):
        return np.zeros(DM.words(self.tgt.width, self.tgt.height), np.uint32)


def test_property_through_the_lane_code(host):
    scene = HostScene(host)
    scene.read_bits = lambda b: b
    H.check_damage_property(scene)
