"""GPU: vgx_mesh_bounds / vgx_cache_cull (csrc/vgx_bounds.hip) against the reference's caches and frames and the numpy statement of
the specification (tests/cache_cull_model.py). Every comparison is exact. The inputs and the assertions on the outputs are those of
tests/test_cache_cull_cpu.py; here the kernels answer, and the culled list goes on through vgx_cache_submit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cache_cull_model as M

pytestmark = pytest.mark.gpu
capi = M.capi
F = np.float32


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.from_numpy(raw.copy() if raw.size else np.zeros(1, dtype=np.uint8)).to("cuda:0")
    return t


def f32_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F).copy()).to("cuda:0")


_caches = {}


def gpu_cache(rt, gpu_ctx, name):
    """The product's cache of the case, built once per session (tessellate_count / _emit + vgx_cache_localize); == the reference's."""
    import torch
    if name not in _caches:
        c = M.case(name)
        pset = rt.PathSet(gpu_ctx, c.ps)
        dd = rt.upload_draws(c.draws)
        sizes = rt.tessellate_count(gpu_ctx, pset, dd, c.draws.shape[0])
        bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
        rt.tessellate_emit(gpu_ctx, pset, dd, c.draws.shape[0], bufs)
        cache = rt.MeshCache(gpu_ctx, bufs, sizes, dd, c.draws.shape[0])
        torch.cuda.synchronize()
        pset.close()
        assert np.array_equal(bufs.pos[:cache.nv].cpu().numpy().view(np.uint32), c.cache.pos.view(np.uint32))
        _caches[name] = cache
    return _caches[name]


def gpu_mesh_bounds(rt, gpu_ctx, pos_dev, meshes, guard=2):
    """vgx_mesh_bounds into a pattern-filled table with `guard` entries behind it, which must stay as they were."""
    import torch
    nm = meshes.shape[0]
    out = torch.full((nm + guard, 4), 7.0, dtype=torch.float32, device="cuda:0")
    md = to_dev(meshes)
    st = rt.lib().vgx_mesh_bounds(gpu_ctx.handle, pos_dev.data_ptr(), md.data_ptr(), nm, out.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    got = out.cpu().numpy()
    assert np.all(got[nm:] == 7.0)
    return got[:nm]


def gpu_cull(rt, gpu_ctx, cache, mb_dev, inst, views, inst_view, in_place=False, want_bounds=True, want_kept=True, guard=3):
    """One vgx_cache_cull call into pattern-filled arrays with `guard` entries behind ninst. Returns (status, inst, bounds, kept,
    num_kept, untouched, inst tensor) -- untouched = nothing behind the ninst (num_kept) entries changed."""
    import torch
    n = inst.shape[0]
    src_np = np.concatenate([inst, np.zeros(guard, dtype=inst.dtype)])
    src = to_dev(src_np)
    dst = src if in_place else torch.zeros_like(src)
    bounds = torch.full((n + guard, 4), 7.0, dtype=torch.float32, device="cuda:0")
    kept = torch.full((n + guard,), -559038737, dtype=torch.int32, device="cuda:0")  # 0xDEADBEEF
    nk = torch.full((1,), 123456789, dtype=torch.int64, device="cuda:0")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    vd = f32_dev(views)
    ivd = None if inst_view is None else to_dev(np.ascontiguousarray(inst_view, dtype=np.uint32))
    d = cache.desc()
    out = capi.CullOut(dst.data_ptr(), bounds.data_ptr() if want_bounds else None, kept.data_ptr() if want_kept else None,
                       nk.data_ptr() if want_kept else None)
    st = rt.lib().vgx_cache_cull(gpu_ctx.handle, C.byref(d), mb_dev.data_ptr(), src.data_ptr(), n, vd.data_ptr(), views.shape[0],
                                 None if ivd is None else ivd.data_ptr(), C.byref(out), status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    gi = dst.cpu().numpy()[:(n + guard) * 40].view(capi.cache_instance_dtype)
    gb, gk, count = bounds.cpu().numpy(), kept.cpu().numpy().view(np.uint32), int(nk.item())
    tail = np.zeros(guard, dtype=inst.dtype)
    untouched = (np.array_equal(gi[n:].view(np.uint8), tail.view(np.uint8)) and bool(np.all(gb[n if want_bounds else 0:] == 7.0))
                 and bool(np.all(gk[count if want_kept else 0:] == 0xDEADBEEF)) and (want_kept or count == 123456789))
    return int(status.item()), gi[:n], gb[:n] if want_bounds else None, gk[:n] if want_kept else None, count if want_kept else None, untouched, dst


@pytest.mark.parametrize("name", ["tiger", "walk"])
def test_mesh_bounds_of_the_cache(rt, gpu_ctx, name):
    c = M.case(name)
    cache = gpu_cache(rt, gpu_ctx, name)
    assert np.array_equal(cache.bounds.cpu().numpy(), c.mesh_boxes)
    assert np.array_equal(gpu_mesh_bounds(rt, gpu_ctx, cache.bufs.pos, c.cache.meshes), c.mesh_boxes)
    # 0-vertex meshes (hand-made records in the real table): the empty box, the others unchanged
    meshes, src = M.with_empty_meshes(c.cache.meshes)
    got = gpu_mesh_bounds(rt, gpu_ctx, cache.bufs.pos, meshes)
    assert np.array_equal(got[src >= 0], c.mesh_boxes)
    assert np.array_equal(got[src < 0], np.tile(M.EMPTY, (int((src < 0).sum()), 1)))
    # a table that starts in the middle of the stream, and a single mesh
    assert np.array_equal(gpu_mesh_bounds(rt, gpu_ctx, cache.bufs.pos, c.cache.meshes[c.nm // 2:]), c.mesh_boxes[c.nm // 2:])
    assert np.array_equal(gpu_mesh_bounds(rt, gpu_ctx, cache.bufs.pos, c.cache.meshes[1:2]), c.mesh_boxes[1:2])


def submit(rt, gpu_ctx, cache, inst_dev, n, frame):
    """vgx_cache_submit into buffers of exactly the oracle frame's size."""
    import torch
    bufs = rt.MeshBuffers("cuda:0", frame.sizes["num_vertices"], frame.sizes["num_indices"], frame.sizes["num_meshes"])
    bufs.pos.fill_(float("nan"))
    rt.cache_submit(gpu_ctx, cache, inst_dev, n, bufs)
    torch.cuda.synchronize()
    return bufs


def assert_frame_equal(rt, bufs, ref):
    nv, ni, nm = ref.sizes["num_vertices"], ref.sizes["num_indices"], ref.sizes["num_meshes"]
    assert int(bufs.dev_status.item()) == 0
    sz = bufs.dev_sizes.cpu().numpy()
    assert (int(sz[3]), int(sz[4]), int(sz[2])) == (nv, ni, nm)
    assert np.array_equal(bufs.pos[:nv].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
    assert np.array_equal(bufs.color[:nv].cpu().numpy().view(np.uint32), ref.color)
    assert np.array_equal(bufs.idx[:ni].cpu().numpy().view(np.uint16), ref.idx)
    gm = bufs.meshes[:nm * 32].cpu().numpy().view(capi.mesh_dtype)
    for f in ref.meshes.dtype.names:
        assert np.array_equal(gm[f], ref.meshes[f]), f


@pytest.mark.parametrize("name,n", [("tiger", 257), ("walk", 65)])
def test_mesh_bounds_of_a_submitted_frame(rt, gpu_ctx, name, n):
    """Device-space boxes: vgx_mesh_bounds on what vgx_cache_submit wrote == min / max of the reference's frame, mesh by mesh. The
    tiger frame has 2.7 M vertices in meshes of 4 .. a few hundred; the walk frame meshes of 8 008 vertices that cross range boundaries."""
    c, inst, _, _ = M.scene(name, n)
    inst = inst[M.finite_mask(inst)]
    ref = M.oracle.cache_submit(c.cache, inst)
    cache = gpu_cache(rt, gpu_ctx, name)
    bufs = submit(rt, gpu_ctx, cache, to_dev(inst), inst.shape[0], ref)
    assert_frame_equal(rt, bufs, ref)
    got = gpu_mesh_bounds(rt, gpu_ctx, bufs.pos, ref.meshes)
    assert np.array_equal(got, M.mesh_boxes(ref.pos, ref.meshes))


@pytest.mark.parametrize("with_view", [True, False])
@pytest.mark.parametrize("name,n", [("tiger", n) for n in M.COUNTS] + [("walk", n) for n in M.WALK_COUNTS])
def test_cull_against_reference_and_model(rt, gpu_ctx, name, n, with_view):
    c, inst, special, t = M.scene(name, n)
    views = M.make_views(c)
    iv = M.make_inst_view(n) if with_view else None
    if n >= M.BIG:
        M.check_input_conditions(inst, t, views, iv)
    cache = gpu_cache(rt, gpu_ctx, name)
    mb = cache.bounds
    mb_host = mb.cpu().numpy()
    assert np.array_equal(mb_host, c.mesh_boxes)
    st, gi, gb, gk, nk, untouched, _ = gpu_cull(rt, gpu_ctx, cache, mb, inst, views, iv)
    assert untouched
    kept = M.check_cull(c, mb_host, inst, special, views, iv, t, st, gi, gb, gk, nk)
    # in place without the dense list, and out of place without the boxes: the rest unchanged
    st2, gi2, gb2, _, _, untouched, _ = gpu_cull(rt, gpu_ctx, cache, mb, inst, views, iv, in_place=True, want_kept=False)
    assert untouched and st2 == st and np.array_equal(gi2.view(np.uint8), gi.view(np.uint8)) and M.boxes_equal(gb2, gb)
    st3, gi3, _, gk3, nk3, untouched, _ = gpu_cull(rt, gpu_ctx, cache, mb, inst, views, iv, want_bounds=False)
    assert untouched and st3 == st and np.array_equal(gi3.view(np.uint8), gi.view(np.uint8)) and nk3 == nk and np.array_equal(gk3[:nk], gk[:nk])
    if n >= M.BIG:
        assert 0 < int(kept.sum()) < n


@pytest.mark.parametrize("n,armed", [(257, False), (257, True), (5000, False)])
def test_submission_of_the_culled_list(rt, gpu_ctx, n, armed):
    """vgx_cache_cull -> vgx_cache_submit(out->inst, ninst) with no count from the device == the reference's frame of the same zeroed
    list, bit for bit, and its vertices are exactly those of the kept instances in the reference's all-instances frame."""
    import torch
    c, inst, special, t = M.scene("tiger", n)
    views, iv = M.make_views(c), M.make_inst_view(n)
    cache = gpu_cache(rt, gpu_ctx, "tiger")
    res = rt.cache_cull(gpu_ctx, cache, cache.bounds, to_dev(inst), n, f32_dev(views), to_dev(iv), want_bounds=False)
    torch.cuda.synchronize()
    assert int(res.dev_status.item()) == 0
    zeroed = res.inst.cpu().numpy()[:n * 40].view(capi.cache_instance_dtype)
    _, m_inst, _, m_kept = M.cull_model(c.nm, c.mesh_boxes, inst, views, iv)
    assert np.array_equal(zeroed.view(np.uint8), m_inst.view(np.uint8)) and int(res.num_kept.item()) == m_kept.shape[0]
    ref = M.oracle.cache_submit(c.cache, zeroed)
    if armed:
        stt, rcmds, ridx = M.oracle.assemble(ref.meshes, ref.idx, 8192)
        assert stt == 0 and len(rcmds) > 10
        cmds = torch.zeros((2 * (ref.sizes["num_vertices"] // 8192) + 2) * 48, dtype=torch.uint8, device="cuda:0")
        ncmd = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        gpu_ctx.set_assembly(cmds, 8192, ncmd)
        try:
            bufs = submit(rt, gpu_ctx, cache, res.inst, n, ref)
        finally:
            gpu_ctx.set_assembly(None)
        assert int(bufs.dev_status.item()) == 0 and int(ncmd.item()) == len(rcmds)
        gc = cmds[:len(rcmds) * 48].cpu().numpy().view(capi.drawcmd_dtype)
        for f in rcmds.dtype.names:
            assert np.array_equal(gc[f], rcmds[f]), f
        assert np.array_equal(bufs.idx[:ref.sizes["num_indices"]].cpu().numpy().view(np.uint16), ridx)
        assert np.array_equal(bufs.pos[:ref.sizes["num_vertices"]].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
        return
    bufs = submit(rt, gpu_ctx, cache, res.inst, n, ref)
    assert_frame_equal(rt, bufs, ref)
    # the kept instances' vertices of the all-instances frame, in order
    kept_mask = zeroed["num_meshes"] != 0
    own = np.repeat(t.frame.meshes["draw"].astype(np.int64), t.frame.meshes["num_vertices"].astype(np.int64))
    want = t.frame.pos[kept_mask[own]]
    assert np.array_equal(bufs.pos[:ref.sizes["num_vertices"]].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.unique(ref.meshes["draw"]), np.nonzero(kept_mask)[0])  # `draw` still names the original instance


def test_invalid_arguments(rt, gpu_ctx):
    c, inst, special, _ = M.scene("tiger", 65)
    cache = gpu_cache(rt, gpu_ctx, "tiger")
    views, iv = M.make_views(c), M.make_inst_view(65)
    for what in ("range", "first", "view"):
        bad, biv = inst.copy(), iv.copy()
        if what == "range":
            bad["first_mesh"][5], bad["num_meshes"][5] = c.nm - 1, 2
        elif what == "first":
            bad["first_mesh"][5], bad["num_meshes"][5] = c.nm + 1, 0
        else:
            biv[5] = views.shape[0]
        st, gi, gb, gk, nk, untouched, _ = gpu_cull(rt, gpu_ctx, cache, cache.bounds, bad, views, biv)
        ms, mi, mbnd, mk = M.cull_model(c.nm, c.mesh_boxes, bad, views, biv)
        assert st == ms == capi.VGX_E_INVALID_ARG and untouched
        assert gi["num_meshes"][5] == 0 and 5 not in gk[:nk].tolist() and np.array_equal(gb[5], M.EMPTY)
        assert np.array_equal(gi.view(np.uint8), mi.view(np.uint8)) and M.boxes_equal(gb, mbnd) and np.array_equal(gk[:nk], mk)
    # host-side argument checks
    d = cache.desc()
    out = capi.CullOut(None, None, None, None)
    assert rt.lib().vgx_cache_cull(gpu_ctx.handle, C.byref(d), cache.bounds.data_ptr(), to_dev(inst).data_ptr(), 65, f32_dev(views).data_ptr(), 3,
                                   None, C.byref(out), None, None) == capi.VGX_E_INVALID_ARG
    assert rt.lib().vgx_mesh_bounds(gpu_ctx.handle, None, None, 3, None, None) == capi.VGX_E_INVALID_ARG


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_mesh_bounds / vgx_cache_cull -> vgx_tessellate_emit still equals the oracle."""
    import torch
    c, inst, special, _ = M.scene("tiger", 257)
    cache = gpu_cache(rt, gpu_ctx, "tiger")
    mb = cache.bounds
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    got_mb = rt.mesh_bounds(gpu_ctx, cache.bufs.pos, cache.bufs.meshes, cache.nm)
    res = rt.cache_cull(gpu_ctx, cache, mb, to_dev(inst), 257, f32_dev(M.make_views(c)), to_dev(M.make_inst_view(257)))
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
    assert np.array_equal(got_mb.cpu().numpy(), c.mesh_boxes) and int(res.dev_status.item()) == 0
    assert int(res.num_kept.item()) == M.cull_model(c.nm, c.mesh_boxes, inst, M.make_views(c), M.make_inst_view(257))[3].shape[0]
