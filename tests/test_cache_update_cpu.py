"""CPU: the lane code of vgx_cache_layout / vgx_cache_update (csrc/vgx_update.h through libvgx_hosttest.so: vgxt_cache_layout,
vgxt_cache_update) against the reference's frames, and the numpy statement of the specification (tests/cache_update_model.py) against
the same frames. The assertions live in cache_update_model.check_*; the GPU suite (tests/test_gpu_cache_update.py) runs them on the
kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import cache_cull_model as M
import cache_update_model as U

capi = M.capi
F = np.float32
POS_PATTERN, COLOR_PATTERN, BOX_PATTERN = F(-12345.5), np.uint32(0xC0FFEE11), F(7.0)


class Frame:
    pass


def guarded(n, width, dtype, pattern):
    """An array of n + 2 * GUARD rows filled with `pattern`, and the view of its n inner rows."""
    shape = (n + 2 * U.GUARD,) + ((width,) if width else ())
    whole = np.full(shape, pattern, dtype=dtype)
    return whole, whole[U.GUARD:U.GUARD + n]


class HostBackend:
    """vgxt_cache_layout / vgxt_cache_update of libvgx_hosttest.so: the functions the kernels call, run sequentially."""

    def __init__(self, lib):
        self.lib = lib

    def desc(self, c):
        k = c.cache
        return capi.CacheDesc(k.pos.ctypes.data, k.color.ctypes.data, k.idx.ctypes.data, k.meshes.ctypes.data, k.meshes.shape[0], k.pos.shape[0], k.idx.shape[0])

    def layout(self, c, inst, guard):
        n = inst.shape[0]
        slots = np.full((n + 1 + guard) * 4, U.SLOT_PATTERN, dtype=np.uint64)
        inst = np.ascontiguousarray(inst)
        d = self.desc(c)
        st = self.lib.vgxt_cache_layout(C.byref(d), inst.ctypes.data, n, slots.ctypes.data)
        return st, slots.view(capi.cache_slot_dtype)

    def frame(self, c, inst0, ref0):
        fr = Frame()
        nv, nm = ref0.frame.pos.shape[0], ref0.frame.meshes.shape[0]
        fr.nv, fr.nm = nv, nm
        fr.pos_all, fr.pos = guarded(nv, 2, F, POS_PATTERN)
        fr.color_all, fr.color = guarded(nv, 0, np.uint32, COLOR_PATTERN)
        fr.box_all, fr.box = guarded(nm, 4, F, BOX_PATTERN)
        fr.pos[:], fr.color[:] = ref0.frame.pos, ref0.frame.color
        meshes = np.ascontiguousarray(ref0.frame.meshes)
        if nm:
            self.lib.vgxt_mesh_bounds(fr.pos.ctypes.data, meshes.ctypes.data, nm, fr.box.ctypes.data)
        return fr

    def update(self, fr, c, inst, slots, dirty, limit, with_bounds, num_vertices=None):
        inst, slots, dirty = np.ascontiguousarray(inst), np.ascontiguousarray(slots), np.ascontiguousarray(dirty, dtype=np.uint32)
        lim = None if limit is None else np.array([limit], dtype=np.uint64)
        f = capi.UpdateFrame(fr.pos.ctypes.data, fr.color.ctypes.data, fr.nv if num_vertices is None else num_vertices, fr.nm,
                             fr.box.ctypes.data if with_bounds else None)
        d = self.desc(c)
        return self.lib.vgxt_cache_update(C.byref(d), inst.ctypes.data, inst.shape[0], slots.ctypes.data, dirty.ctypes.data, dirty.shape[0],
                                          None if lim is None else lim.ctypes.data, C.byref(f))

    def read(self, fr):
        g = U.GUARD
        intact = all(bool(np.all(a[:g] == p)) and bool(np.all(a[a.shape[0] - g:] == p))
                     for a, p in ((fr.pos_all, POS_PATTERN), (fr.color_all, COLOR_PATTERN), (fr.box_all, BOX_PATTERN)))
        return fr.pos.copy(), fr.color.copy(), fr.box.copy(), intact, True  # idx and the mesh table are not handed to the call at all


class ModelBackend(HostBackend):
    """The numpy statement of the specification in the place of the product: the same assertions pin it on the reference."""

    def layout(self, c, inst, guard):
        st, slots = U.layout_model(c.cache, inst)
        tail = np.full(guard * 4, U.SLOT_PATTERN, dtype=np.uint64).view(capi.cache_slot_dtype)
        return st, np.concatenate([slots, tail])

    def update(self, fr, c, inst, slots, dirty, limit, with_bounds, num_vertices=None):
        st, _ = U.update_model(c.cache, inst, slots, dirty, limit, fr.pos, fr.color, fr.nv if num_vertices is None else num_vertices, fr.nm,
                               fr.box if with_bounds else None)
        return st


@pytest.fixture(scope="module")
def hostlib():
    path = os.path.join(M.ROOT, "vg-renderer_amd", "libvgx_hosttest.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(path)
    lib.vgxt_mesh_bounds.restype = None
    lib.vgxt_mesh_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vgxt_cache_layout.restype = C.c_int
    lib.vgxt_cache_layout.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vgxt_cache_update.restype = C.c_int
    lib.vgxt_cache_update.argtypes = [C.POINTER(capi.CacheDesc), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.POINTER(capi.UpdateFrame)]
    return lib


@pytest.fixture(scope="module", params=["host", "model"])
def backend(request, hostlib):
    return HostBackend(hostlib) if request.param == "host" else ModelBackend(hostlib)


LISTS = [(name, n, kind) for name, n in U.SCENES for kind in U.list_kinds(n)]


def test_inputs_cover_the_ranges_the_issue_names():
    """Ranges of 0, 1, 3 and 435 meshes; meshes from a fraction of a wave to 8 008 vertices; instances with a NaN / infinite matrix among
    the listed ones."""
    c, inst0, inst1 = U.arrays("tiger", 257)
    assert set(np.unique(inst0["num_meshes"]).tolist()) == {0, 1, 3, 435}
    assert int(c.cache.meshes["num_vertices"].min()) < 64 < int(c.cache.meshes["num_vertices"].max())
    assert int(M.case("walk").cache.meshes["num_vertices"].max()) == 8008
    assert not M.finite_mask(inst1).all() and np.array_equal(M.finite_mask(inst0), M.finite_mask(inst1))
    assert not np.array_equal(inst0["mtx"], inst1["mtx"]) and not np.array_equal(inst0["color"], inst1["color"])
    assert np.array_equal(inst0["first_mesh"], inst1["first_mesh"]) and np.array_equal(inst0["num_meshes"], inst1["num_meshes"])
    uniform = (capi.MESH_FILL, capi.MESH_STROKE)  # the issue's caches are all AA; 'plain' brings the meshes that take the instance's colour
    assert not np.isin(c.cache.meshes["subpath_kind"] >> 28, uniform).any()
    kinds = U.case("plain").cache.meshes["subpath_kind"] >> 28
    assert all((kinds == k).any() for k in uniform) and not np.isin(kinds, uniform).all()


@pytest.mark.parametrize("name,n", U.LAYOUT_SCENES)
def test_slots_against_the_reference(backend, name, n):
    U.check_slots(backend, name, n)


def test_layout_of_a_range_outside_the_cache(backend):
    U.check_layout_invalid(backend)


# the model walks every mesh in Python: three lists of the largest frame pin it, the lane code takes them all
MODEL_LISTS = [(name, n, kind) for name, n, kind in LISTS if n < 257 or kind in ("one", "k64", "limit")]


@pytest.mark.parametrize("name,n,kind", LISTS)
def test_dirty_lists(hostlib, name, n, kind):
    U.check_dirty_list(HostBackend(hostlib), name, n, kind)


@pytest.mark.parametrize("name,n,kind", MODEL_LISTS)
def test_dirty_lists_model(hostlib, name, n, kind):
    U.check_dirty_list(ModelBackend(hostlib), name, n, kind)


@pytest.mark.parametrize("name,n", [("tiger", 65), ("walk", 65)])
def test_without_mesh_bounds(backend, name, n):
    U.check_without_bounds(backend, name, n)


@pytest.mark.parametrize("what", ["range", "stale", "both"])
def test_errors(backend, what):
    U.check_errors(backend, what)


def test_frame_shorter_than_a_slice(backend):
    U.check_short_frame(backend)
    # frame->num_meshes below a slice's mesh end: the same rule, through the model and the lane code alike
    c, inst0, inst1 = U.arrays("tiger", 65)
    _, slots = U.layout_model(c.cache, inst0)
    fr = backend.frame(c, inst0, U.reference(c, inst0))
    d = [i for i in range(65) if int(inst0["num_meshes"][i])][-1]
    before = fr.pos.copy()
    fr.nm = int(slots["first_mesh"][d + 1]) - 1
    assert backend.update(fr, c, inst1, slots, np.array([d], dtype=np.uint32), None, False) == capi.VGX_E_INVALID_ARG
    assert np.array_equal(fr.pos.view(np.uint32), before.view(np.uint32))


def test_slots_of_another_array_are_stale(backend):
    """Slots whose vertex span differs from the range's count in the cache (the third stale rule): nothing is written."""
    c, inst0, inst1 = U.arrays("tiger", 65)
    _, slots = U.layout_model(c.cache, inst0)
    d = U.whole_drawing(c, inst0)
    bent = slots.copy()
    bent["first_vertex"][d + 1:] += 1
    fr = backend.frame(c, inst0, U.reference(c, inst0))
    before = fr.pos.copy()
    assert backend.update(fr, c, inst1, bent, np.array([d], dtype=np.uint32), None, True) == capi.VGX_E_STALE
    assert np.array_equal(fr.pos.view(np.uint32), before.view(np.uint32))
