"""CPU: the lane code of vgx_mesh_bounds / vgx_cache_cull (csrc/vgx_bounds.h through libvgx_hosttest.so: vgxt_mesh_bounds,
vgxt_cache_cull) against the reference's caches and frames and against the numpy statement of the specification
(tests/cache_cull_model.py). Exact everywhere; the GPU suite (tests/test_gpu_cache_cull.py) makes the same assertions on the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import cache_cull_model as M

capi = M.capi
F = np.float32


@pytest.fixture(scope="module")
def host():
    path = os.path.join(M.ROOT, "vg-renderer_amd", "libvgx_hosttest.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(path)
    lib.vgxt_mesh_bounds.restype = None
    lib.vgxt_mesh_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.vgxt_cache_cull.restype = C.c_int
    lib.vgxt_cache_cull.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(capi.CullOut)]
    lib.vgxt_ord_from_float.restype = C.c_uint32
    lib.vgxt_ord_from_float.argtypes = [C.c_float]
    lib.vgxt_float_from_ord.restype = C.c_float
    lib.vgxt_float_from_ord.argtypes = [C.c_uint32]
    return lib


def host_mesh_bounds(host, pos, meshes):
    pos, meshes = np.ascontiguousarray(pos, dtype=F), np.ascontiguousarray(meshes)
    out = np.full((meshes.shape[0], 4), 7.0, dtype=F)
    host.vgxt_mesh_bounds(pos.ctypes.data, meshes.ctypes.data, meshes.shape[0], out.ctypes.data)
    return out


def host_cull(host, nm, mb, inst, views, inst_view, in_place=False, want_bounds=True, want_kept=True, guard=3):
    """One vgxt_cache_cull call into arrays with `guard` extra entries behind the ninst the call may write: returns
    (status, inst, bounds, kept, num_kept, untouched) -- untouched = nothing behind ninst changed."""
    n = inst.shape[0]
    src = np.concatenate([inst, np.zeros(guard, dtype=inst.dtype)])
    dst = src if in_place else np.full(n + guard, 0, dtype=inst.dtype)
    dst_tail = dst[n:].copy()
    bounds = np.full((n + guard, 4), 7.0, dtype=F)
    kept = np.full(n + guard, 0xDEADBEEF, dtype=np.uint32)
    nk = np.full(1, 123456789, dtype=np.uint64)
    out = capi.CullOut(dst.ctypes.data, bounds.ctypes.data if want_bounds else None, kept.ctypes.data if want_kept else None,
                       nk.ctypes.data if want_kept else None)
    mb = np.ascontiguousarray(mb, dtype=F)
    iv = None if inst_view is None else np.ascontiguousarray(inst_view, dtype=np.uint32)
    st = host.vgxt_cache_cull(nm, mb.ctypes.data, src.ctypes.data, n, views.ctypes.data, views.shape[0], None if iv is None else iv.ctypes.data, C.byref(out))
    count = int(nk[0]) if want_kept else 0
    untouched = (np.array_equal(dst[n:].view(np.uint8), dst_tail.view(np.uint8)) and np.all(bounds[n:] == 7.0)
                 and np.all(kept[count if want_kept else 0:] == 0xDEADBEEF))
    return st, dst[:n], bounds[:n] if want_bounds else None, kept[:n] if want_kept else None, count if want_kept else None, untouched


def test_ordered_image_is_monotone_and_round_trips(host):
    vals = np.array([-np.inf, -3.0e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, 2.5, 3.0e38, np.inf], dtype=F)
    img = [host.vgxt_ord_from_float(float(v)) for v in vals]
    assert all(a < b for a, b in zip(img, img[1:]))
    assert img[0] == 0x007FFFFF and img[-1] == 0xFF800000
    for v, o in zip(vals, img):
        assert np.array([host.vgxt_float_from_ord(o)], dtype=F).view(np.uint32)[0] == np.array([v], dtype=F).view(np.uint32)[0]
    rs = np.random.RandomState(1)
    r = rs.randint(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32).view(F)
    r = r[np.isfinite(r)]
    o = np.array([host.vgxt_ord_from_float(float(v)) for v in r], dtype=np.uint64)
    k = np.argsort(r, kind="stable")
    assert np.all(np.diff(o[k].astype(np.int64)) >= 0)


@pytest.mark.parametrize("name", ["tiger", "walk"])
def test_mesh_bounds_of_the_cache(host, name):
    c = M.case(name)
    got = host_mesh_bounds(host, c.cache.pos, c.cache.meshes)
    assert np.array_equal(got, c.mesh_boxes)
    # 0-vertex meshes (hand-made records in a real table, see cache_cull_model): the empty box, the others unchanged
    meshes, src = M.with_empty_meshes(c.cache.meshes)
    got = host_mesh_bounds(host, c.cache.pos, meshes)
    assert np.array_equal(got[src >= 0], c.mesh_boxes)
    assert np.array_equal(got[src < 0], np.tile(M.EMPTY, (int((src < 0).sum()), 1)))


def test_fuzz_paths_yield_no_empty_mesh():
    """Why the 0-vertex records are hand-made (cache_cull_model.with_empty_meshes): the fuzzers produce none. If this fails, use theirs."""
    for seed in range(1, 25):
        ps = M.wl.fuzz_paths(seed)
        r = M.oracle.tessellate(ps, M.wl.fuzz_draws(ps, seed))
        assert r.meshes.shape[0] > 0 and int(r.meshes["num_vertices"].min()) > 0, seed


@pytest.mark.parametrize("n", [65, 257])
def test_mesh_bounds_of_a_submitted_frame(host, n):
    c = M.case("tiger")
    inst, _ = M.make_instances(c, n)
    inst = inst[np.isfinite(inst["mtx"]).all(axis=1)]
    frame = M.oracle.cache_submit(c.cache, inst)
    got = host_mesh_bounds(host, frame.pos, frame.meshes)
    assert np.array_equal(got, M.mesh_boxes(frame.pos, frame.meshes))


@pytest.mark.parametrize("with_view", [True, False])
@pytest.mark.parametrize("name,n", [("tiger", n) for n in M.COUNTS] + [("walk", n) for n in M.WALK_COUNTS])
def test_cull_against_reference_and_model(host, name, n, with_view):
    c, inst, special, t = M.scene(name, n)
    views = M.make_views(c)
    iv = M.make_inst_view(n) if with_view else None
    if n >= M.BIG:
        M.check_input_conditions(inst, t, views, iv)
    mb = host_mesh_bounds(host, c.cache.pos, c.cache.meshes)
    st, gi, gb, gk, nk, untouched = host_cull(host, c.nm, mb, inst, views, iv)
    assert untouched
    kept = M.check_cull(c, mb, inst, special, views, iv, t, st, gi, gb, gk, nk)
    # in place, and without the dense list: the same records
    st2, gi2, gb2, _, _, untouched = host_cull(host, c.nm, mb, inst, views, iv, in_place=True, want_kept=False)
    assert untouched and st2 == st and np.array_equal(gi2.view(np.uint8), gi.view(np.uint8)) and M.boxes_equal(gb2, gb)
    st3, gi3, _, gk3, nk3, untouched = host_cull(host, c.nm, mb, inst, views, iv, want_bounds=False)
    assert untouched and st3 == st and np.array_equal(gi3.view(np.uint8), gi.view(np.uint8)) and nk3 == nk and np.array_equal(gk3[:nk], gk[:nk])
    if n >= M.BIG:
        assert 0 < int(kept.sum()) < n


def test_cull_of_empty_meshes_and_empty_views(host):
    """A range of nothing but 0-vertex meshes is culled with the empty box; a view with x0 > x1 or y0 > y1 culls everything."""
    c = M.case("tiger")
    meshes, src = M.with_empty_meshes(c.cache.meshes)
    mb = host_mesh_bounds(host, c.cache.pos, meshes)
    z = int(np.nonzero(src < 0)[0][1])  # the two records in the middle
    inst = np.zeros(3, dtype=capi.cache_instance_dtype)
    inst["mtx"][:] = [1, 0, 0, 1, 0, 0]
    inst["first_mesh"], inst["num_meshes"] = [z, z, 0], [2, 3, meshes.shape[0]]
    everything = np.array([[-1e30, -1e30, 1e30, 1e30]], dtype=F)
    st, gi, gb, gk, nk, _ = host_cull(host, meshes.shape[0], mb, inst, everything, None)
    assert st == 0 and gi["num_meshes"].tolist() == [0, 3, meshes.shape[0]] and nk == 2 and gk[:2].tolist() == [1, 2]
    assert np.array_equal(gb[0], M.EMPTY) and np.array_equal(gb[2], c.box)
    for v in ([5, 0, 4, 10], [0, 5, 10, 4]):
        st, gi, gb, gk, nk, _ = host_cull(host, meshes.shape[0], mb, inst, np.array([v], dtype=F), None)
        assert st == 0 and nk == 0 and not gi["num_meshes"].any()


def test_invalid_arguments(host):
    c = M.case("tiger")
    mb = host_mesh_bounds(host, c.cache.pos, c.cache.meshes)
    inst, special = M.make_instances(c, 65)
    views = M.make_views(c)
    iv = M.make_inst_view(65)
    for what in ("range", "first", "view"):
        bad, biv = inst.copy(), iv.copy()
        if what == "range":
            bad["first_mesh"][5], bad["num_meshes"][5] = c.nm - 1, 2
        elif what == "first":
            bad["first_mesh"][5], bad["num_meshes"][5] = c.nm + 1, 0
        else:
            biv[5] = views.shape[0]
        st, gi, gb, gk, nk, untouched = host_cull(host, c.nm, mb, bad, views, biv)
        ms, mi, mbnd, mk = M.cull_model(c.nm, mb, bad, views, biv)
        assert st == ms == capi.VGX_E_INVALID_ARG and untouched
        assert gi["num_meshes"][5] == 0 and 5 not in gk[:nk].tolist() and np.array_equal(gb[5], M.EMPTY)
        assert np.array_equal(gi.view(np.uint8), mi.view(np.uint8)) and M.boxes_equal(gb, mbnd) and np.array_equal(gk[:nk], mk)
