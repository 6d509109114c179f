"""GPU: vgx_cache_layout / vgx_cache_update (csrc/vgx_update.hip) against the reference's frames. The inputs and the assertions are those
of tests/test_cache_update_cpu.py (cache_update_model.check_*); here vgx_cache_submit writes the frame, vgx_mesh_bounds its box table,
and the kernels answer. Then what only a device run can show: the boxes against a fresh vgx_mesh_bounds of the updated frame, an
assembled frame, a counted state across the calls, two updates on one stream."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cache_cull_model as M
import cache_update_model as U

pytestmark = pytest.mark.gpu
capi = M.capi
F = np.float32
G = U.GUARD
POS_PATTERN, COLOR_PATTERN, BOX_PATTERN = -12345.5, 0x3C0FFEE1, 7.0


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def to_dev(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(8, dtype=np.uint8)).to("cuda:0")


_caches = {}


def gpu_cache(rt, gpu_ctx, name):
    """The product's cache of the case, built once per session (tessellate_count / _emit + vgx_cache_localize); == the reference's."""
    import torch
    if name not in _caches:
        c = U.case(name)
        pset = rt.PathSet(gpu_ctx, c.ps)
        dd = rt.upload_draws(c.draws)
        sizes = rt.tessellate_count(gpu_ctx, pset, dd, c.draws.shape[0])
        bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
        rt.tessellate_emit(gpu_ctx, pset, dd, c.draws.shape[0], bufs)
        cache = rt.MeshCache(gpu_ctx, bufs, sizes, dd, c.draws.shape[0])
        torch.cuda.synchronize()
        pset.close()
        assert np.array_equal(bufs.pos[:cache.nv].cpu().numpy().view(np.uint32), c.cache.pos.view(np.uint32))
        assert np.array_equal(bufs.color[:cache.nv].cpu().numpy().view(np.uint32), c.cache.color)
        _caches[name] = cache
    return _caches[name]


class Frame:
    pass


class GpuBackend:
    def __init__(self, rt, ctx):
        self.rt, self.ctx = rt, ctx

    def layout(self, c, inst, guard):
        import torch
        n = inst.shape[0]
        slots = torch.full(((n + 1 + guard) * 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")  # 0xA5A5...
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
        d = gpu_cache(self.rt, self.ctx, c.name).desc()
        st = self.rt.lib().vgx_cache_layout(self.ctx.handle, C.byref(d), to_dev(inst).data_ptr(), n, slots.data_ptr(), status.data_ptr(), self.rt._stream_ptr())
        torch.cuda.synchronize()
        assert st == 0
        return int(status.item()), slots.cpu().numpy().view(capi.cache_slot_dtype)

    def frame(self, c, inst0, ref0):
        """vgx_cache_submit of inst0 into the inner part of pattern-filled buffers, vgx_mesh_bounds of it into a pattern-filled table."""
        import torch
        rt = self.rt
        fr = Frame()
        nv, ni, nm = ref0.frame.pos.shape[0], ref0.frame.idx.shape[0], ref0.frame.meshes.shape[0]
        fr.nv, fr.ni, fr.nm = nv, ni, nm
        fr.all = rt.MeshBuffers("cuda:0", nv + 2 * G, ni + 2 * G, nm + 2 * G)
        fr.all.pos.fill_(POS_PATTERN), fr.all.color.fill_(COLOR_PATTERN), fr.all.idx.fill_(0x5EED), fr.all.meshes.fill_(0xEE)
        fr.view = fr.all.view(G, nv, G, ni, G, nm)
        fr.cache = gpu_cache(rt, self.ctx, c.name)
        rt.cache_submit(self.ctx, fr.cache, to_dev(inst0), inst0.shape[0], fr.view)
        fr.box_all = torch.full((nm + 2 * G, 4), BOX_PATTERN, dtype=torch.float32, device="cuda:0")
        fr.box = fr.box_all[G:G + nm]
        if nm:
            assert rt.lib().vgx_mesh_bounds(self.ctx.handle, fr.view.pos.data_ptr(), fr.view.meshes.data_ptr(), nm, fr.box.data_ptr(), rt._stream_ptr()) == 0
        torch.cuda.synchronize()
        assert int(fr.view.dev_status.item()) == 0
        sz = fr.view.dev_sizes.cpu().numpy()
        assert (int(sz[3]), int(sz[4]), int(sz[2])) == (nv, ni, nm)
        fr.idx0, fr.meshes0 = fr.all.idx.clone(), fr.all.meshes.clone()
        return fr

    def update(self, fr, c, inst, slots, dirty, limit, with_bounds, num_vertices=None, sync=True):
        import torch
        rt = self.rt
        lim = None if limit is None else torch.tensor([int(limit)], dtype=torch.int64, device="cuda:0")
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
        di, ds, dd = to_dev(inst), to_dev(slots), to_dev(np.ascontiguousarray(dirty, dtype=np.uint32))
        fr.keep = getattr(fr, "keep", []) + [di, ds, dd, lim]  # alive until the frame goes: the call is asynchronous
        rt.cache_update(self.ctx, fr.cache, di, inst.shape[0], ds, dd, dirty.shape[0],
                        fr.view.pos, fr.view.color, fr.nv if num_vertices is None else num_vertices, fr.nm,
                        mesh_bounds=fr.box if with_bounds else None, dev_ndirty=lim, dev_status=status)
        if not sync:
            return status
        torch.cuda.synchronize()
        return int(status.item())

    def read(self, fr):
        import torch
        torch.cuda.synchronize()
        pos, color, box = fr.all.pos.cpu().numpy(), fr.all.color.cpu().numpy().view(np.uint32), fr.box_all.cpu().numpy()
        nv, nm = fr.nv, fr.nm
        intact = (bool(np.all(pos[:G] == F(POS_PATTERN))) and bool(np.all(pos[G + nv:] == F(POS_PATTERN)))
                  and bool(np.all(color[:G] == COLOR_PATTERN)) and bool(np.all(color[G + nv:] == COLOR_PATTERN))
                  and bool(np.all(box[:G] == F(BOX_PATTERN))) and bool(np.all(box[G + nm:] == F(BOX_PATTERN))))
        others = bool(torch.equal(fr.all.idx, fr.idx0)) and bool(torch.equal(fr.all.meshes, fr.meshes0))
        return pos[G:G + nv].copy(), color[G:G + nv].copy(), box[G:G + nm].copy(), intact, others


@pytest.fixture(scope="module")
def backend(rt, gpu_ctx):
    return GpuBackend(rt, gpu_ctx)


LISTS = [(name, n, kind) for name, n in U.SCENES for kind in U.list_kinds(n)]


@pytest.mark.parametrize("name,n", U.LAYOUT_SCENES)
def test_slots_against_the_reference(backend, name, n):
    U.check_slots(backend, name, n)


def test_layout_of_a_range_outside_the_cache(backend):
    U.check_layout_invalid(backend)


@pytest.mark.parametrize("name,n,kind", LISTS)
def test_dirty_lists(rt, gpu_ctx, backend, name, n, kind):
    fr, r1 = U.check_dirty_list(backend, name, n, kind)
    # the frame the submit wrote is the reference's mesh table, so the boxes below are those of the same meshes
    gm = fr.view.meshes[:fr.nm * 32].cpu().numpy().view(capi.mesh_dtype)
    for f in r1.frame.meshes.dtype.names:
        assert np.array_equal(gm[f], r1.frame.meshes[f]), f
    # the refreshed table == a fresh vgx_mesh_bounds of the updated frame, exactly, over the meshes of finite instances
    _, _, bounds, _, _ = backend.read(fr)
    fresh = rt.mesh_bounds(gpu_ctx, fr.view.pos, fr.view.meshes, fr.nm).cpu().numpy()
    fm = r1.fin[r1.mesh_owner]
    assert np.array_equal(bounds[fm].view(np.uint32), fresh[fm].view(np.uint32))


@pytest.mark.parametrize("name,n", [("tiger", 65), ("walk", 65)])
def test_without_mesh_bounds(backend, name, n):
    U.check_without_bounds(backend, name, n)


@pytest.mark.parametrize("what", ["range", "stale", "both"])
def test_errors(backend, what):
    U.check_errors(backend, what)


def test_frame_shorter_than_a_slice(backend):
    U.check_short_frame(backend)


def test_host_argument_checks(rt, gpu_ctx, backend):
    c, inst0, inst1 = U.arrays("tiger", 65)
    cache = gpu_cache(rt, gpu_ctx, "tiger")
    d = cache.desc()
    lib, h = rt.lib(), gpu_ctx.handle
    inst, slots = to_dev(inst0), to_dev(U.layout_model(c.cache, inst0)[1])
    dirty = to_dev(np.arange(8, dtype=np.uint32))
    fr = backend.frame(c, inst0, U.reference(c, inst0))
    f = capi.UpdateFrame(fr.view.pos.data_ptr(), fr.view.color.data_ptr(), fr.nv, fr.nm, fr.box.data_ptr())
    E = capi.VGX_E_INVALID_ARG
    assert lib.vgx_cache_layout(h, C.byref(d), inst.data_ptr(), 65, None, None, None) == E
    assert lib.vgx_cache_layout(h, C.byref(d), None, 65, slots.data_ptr(), None, None) == E
    assert lib.vgx_cache_layout(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr() + 4, None, None) == E
    assert lib.vgx_cache_layout(h, C.byref(d), inst.data_ptr(), 1 << 32, slots.data_ptr(), None, None) == capi.VGX_E_RANGE
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr(), None, 8, None, C.byref(f), None, None) == E
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, None, dirty.data_ptr(), 8, None, C.byref(f), None, None) == E
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr(), dirty.data_ptr(), 8, None, None, None, None) == E
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr(), dirty.data_ptr() + 2, 8, None, C.byref(f), None, None) == E
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr(), dirty.data_ptr(), 1 << 32, None, C.byref(f), None, None) == capi.VGX_E_RANGE
    bad = capi.UpdateFrame(fr.view.pos.data_ptr(), fr.view.color.data_ptr(), fr.nv, fr.nm, fr.box.data_ptr() + 8)
    assert lib.vgx_cache_update(h, C.byref(d), inst.data_ptr(), 65, slots.data_ptr(), dirty.data_ptr(), 8, None, C.byref(bad), None, None) == E
    # ndirty == 0 is valid, with no list at all, and writes nothing but the status
    st = backend.update(fr, c, inst1, U.layout_model(c.cache, inst0)[1], np.zeros(0, dtype=np.uint32), None, True)
    assert st == capi.VGX_OK
    pos, color, _, guards, others = backend.read(fr)
    assert guards and others
    U.assert_frame(pos, color, U.reference(c, inst0))


def test_assembled_frame(rt, gpu_ctx, backend):
    """Submit under vgx_set_assembly (vertex buffers of 1 024 vertices, a UV stream), lay out and update while it is armed: pos / color
    == a fresh assembled submit of the mixed array; idx, uv and the draw commands keep their bytes."""
    import torch
    c, inst0, inst1 = U.arrays("tiger", 65)
    dirty, _ = U.dirty_list("tiger", 65, "k63")
    mixed = U.mix(inst0, inst1, [int(d) for d in dirty])
    r0, r1 = U.reference(c, inst0), U.reference(c, mixed)
    nv = r0.frame.pos.shape[0]
    ncap = 2 * (nv // 1024) + r0.frame.meshes.shape[0] + 2

    def armed_submit(inst, ref):
        cmds = torch.zeros(ncap * 48, dtype=torch.uint8, device="cuda:0")
        ncmd = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        uv = torch.zeros((nv + 3, 2), dtype=torch.int16, device="cuda:0")
        gpu_ctx.set_assembly(cmds, 1024, ncmd, uv=uv, uv_value=(0x7FFF0001,))
        fr = backend.frame(c, inst, ref)
        return fr, cmds, ncmd, uv

    try:
        fr, cmds, ncmd, uv = armed_submit(inst0, r0)
        assert int(ncmd.item()) > 10
        cmds0, uv0 = cmds.clone(), uv.clone()
        assert not np.array_equal(fr.view.idx[:fr.ni].cpu().numpy().view(np.uint16), r0.frame.idx)  # command-relative indices
        st, slots = backend.layout(c, inst0, 0)  # ignores the armed assembly
        assert st == 0 and np.array_equal(slots.view(np.uint64), U.layout_model(c.cache, inst0)[1].view(np.uint64))
        assert backend.update(fr, c, inst1, slots, dirty, None, True) == capi.VGX_OK
        pos, color, bounds, guards, others = backend.read(fr)
        assert guards and others and torch.equal(cmds, cmds0) and torch.equal(uv, uv0)
        fresh, cmds1, ncmd1, _ = armed_submit(mixed, r1)
        fpos, fcolor, _, _, _ = backend.read(fresh)
        assert int(ncmd1.item()) == int(ncmd.item()) and torch.equal(cmds1, cmds0) and torch.equal(fresh.all.idx, fr.all.idx)
    finally:
        gpu_ctx.set_assembly(None)
    fv = r1.fin[r1.owner]
    assert np.array_equal(pos[fv].view(np.uint32), fpos[fv].view(np.uint32)) and U.same_or_nan(pos[~fv], fpos[~fv])
    assert np.array_equal(color, fcolor)
    U.assert_frame(pos, color, r1)


def test_counted_state_survives(rt, gpu_ctx, backend, wl, oracle):
    """vgx_tessellate_count -> vgx_cache_layout + vgx_cache_update -> vgx_tessellate_emit gives the counted batch's bytes."""
    import torch
    c, inst0, inst1 = U.arrays("tiger", 65)
    r0 = U.reference(c, inst0)
    fr = backend.frame(c, inst0, r0)
    dirty, _ = U.dirty_list("tiger", 65, "shuffled")
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    st, slots = backend.layout(c, inst0, 0)
    assert st == 0 and backend.update(fr, c, inst1, slots, dirty, None, True) == capi.VGX_OK
    bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(gpu_ctx, pset, dd, d.shape[0], bufs)
    torch.cuda.synchronize()
    pset.close()
    nv, ni, nm = ref.sizes["num_vertices"], ref.sizes["num_indices"], ref.sizes["num_meshes"]
    assert (sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]) == (nv, ni, nm)
    assert np.array_equal(bufs.pos[:nv].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
    assert np.array_equal(bufs.color[:nv].cpu().numpy().view(np.uint32), ref.color)
    assert np.array_equal(bufs.idx[:ni].cpu().numpy().view(np.uint16), ref.idx)
    gm = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    for f in ref.meshes.dtype.names:
        assert np.array_equal(gm[f], ref.meshes[f]), f
    pos, color, _, guards, others = backend.read(fr)
    assert guards and others
    U.assert_frame(pos, color, U.reference(c, U.mix(inst0, inst1, range(65))))


def test_two_updates_on_one_stream(backend):
    """Update A, then update B with an overlapping list and other records, no synchronisation between: the B-over-A frame."""
    import torch
    c, inst0, inst1 = U.arrays("tiger", 65)
    other, _ = M.make_instances(c, 65, seed=7)
    inst2 = inst0.copy()
    inst2["mtx"], inst2["color"] = other["mtx"], other["color"]
    perm, _ = U.dirty_list("tiger", 65, "shuffled")
    la, lb = perm[:40], perm[20:60]
    _, slots = U.layout_model(c.cache, inst0)
    fr = backend.frame(c, inst0, U.reference(c, inst0))
    sa = backend.update(fr, c, inst1, slots, la, None, True, sync=False)
    sb = backend.update(fr, c, inst2, slots, lb, None, True, sync=False)
    torch.cuda.synchronize()
    assert int(sa.item()) == 0 and int(sb.item()) == 0
    mixed = U.mix(U.mix(inst0, inst1, [int(d) for d in la]), inst2, [int(d) for d in lb])
    r = U.reference(c, mixed)
    pos, color, bounds, guards, others = backend.read(fr)
    assert guards and others
    U.assert_frame(pos, color, r)
    fm = r.fin[r.mesh_owner]
    assert M.boxes_equal(bounds[fm], U.ref_boxes(r)[fm])
