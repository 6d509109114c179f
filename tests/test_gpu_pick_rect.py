"""GPU: vgx_pick_rect (csrc/vgx_pick_rect.hip) against the numpy statement of the specification (tests/pick_rect_model.py) on frames written
by the reference. Every comparison is exact: every word of top, count and list, the untouched entries included. The frames, the query sets
and the model's answers are those of tests/test_pick_rect_cpu.py; here the kernels answer. The shapes are the smallest at which the kernels
can go wrong: the `walk` meshes (8 008 vertices) cross several 256-triangle tiles, the 1-3-mesh Tiger ranges put many tiny meshes into one
wave, a whole-drawing instance (435 meshes) is a run longer than a workgroup of 256 meshes and crosses scan blocks, `empty` has 0-vertex
meshes inside runs, and a hand-made frame of 132 000 one-triangle meshes takes the per-query walk over the blocks into its second step;
nothing is full size."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import pick_rect_model as R
import test_gpu_pick as G  # the device frames and vgx_pick's harness

pytestmark = pytest.mark.gpu
P = R.P
capi = R.capi
F = np.float32
NONE = R.NONE
PATTERN = 0x5A5A5A5A
SKIP, WINDOW, BY_DRAW = R.SKIP, R.WINDOW, R.BY_DRAW


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


class Got:
    pass


def gpu_pick_rect(rt, ctx, df, queries, cap=R.LIST_CAP, bounds=None, want=("top", "list", "count"), guard=2):
    """vgx_pick_rect in calls of at most 64 queries, each into pattern-filled arrays with guard rows, which must stay as they were, as must
    the queries. Returns top, count and the list rows as the calls left them."""
    import torch
    nq = queries.shape[0]
    g = Got()
    g.top = np.full(nq * 4, PATTERN, dtype=np.uint32).view(capi.pick_hit_dtype)
    g.count = np.full(nq, PATTERN, dtype=np.uint32)
    g.list = np.full((nq, cap), PATTERN, dtype=np.uint32)
    for a, b in R.chunks(nq):
        n = b - a
        q = G.to_dev(queries[a:b])
        top = torch.full(((n + guard) * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
        lst = torch.full(((n + guard) * max(cap, 1),), PATTERN, dtype=torch.int32, device="cuda:0")
        cnt = torch.full((n + guard,), PATTERN, dtype=torch.int32, device="cuda:0")
        out = capi.PickRectOut(top.data_ptr() if "top" in want else None, lst.data_ptr() if "list" in want and cap else None,
                               cnt.data_ptr() if "count" in want else None, cap if "list" in want else 0, 0)
        st = rt.lib().vgx_pick_rect(ctx.handle, C.byref(df.desc), None if bounds is None else bounds.data_ptr(), q.data_ptr(), n, C.byref(out), rt._stream_ptr())
        torch.cuda.synchronize()
        assert st == capi.VGX_OK
        top, lst, cnt = (t.cpu().numpy().view(np.uint32) for t in (top, lst, cnt))
        assert np.all(top[n * 4:] == PATTERN) and np.all(lst[n * cap:] == PATTERN) and np.all(cnt[n:] == PATTERN)
        assert q.cpu().numpy()[:n * 32].tobytes() == np.ascontiguousarray(queries[a:b]).tobytes()
        g.top[a:b] = top[:n * 4].view(capi.pick_hit_dtype)
        g.count[a:b] = cnt[:n]
        g.list[a:b] = lst[:n * cap].reshape(n, cap)
    return g


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_equals_model(g, r, cap, sl=slice(None), want=("top", "list", "count")):
    import test_pick_rect_cpu as cpu
    cpu.assert_equals_model(g, r, cap, sl, want)


@pytest.mark.parametrize("name,n", R.CASES)
def test_kernels_equal_model(rt, gpu_ctx, name, n):
    r = R.frame(name, n)
    R.check_query_conditions(r)
    df = G.dev_frame(r.f)
    mb = G.gpu_bounds(rt, gpu_ctx, df)
    with_boxes = gpu_pick_rect(rt, gpu_ctx, df, r.queries, bounds=mb)
    assert_equals_model(with_boxes, r, R.LIST_CAP)
    own_boxes = gpu_pick_rect(rt, gpu_ctx, df, r.queries)
    assert same(own_boxes.top, with_boxes.top) and same(own_boxes.count, with_boxes.count) and same(own_boxes.list, with_boxes.list)
    assert df.unchanged()
    assert np.array_equal(mb.cpu().numpy()[:df.nm], r.boxes)  # mesh_bounds as it was, too


def test_frame_of_many_small_meshes(rt, gpu_ctx):
    """132 000 one-triangle meshes: more than the 131 072 the per-query walk over the blocks takes in one step, so the second step's
    entries are listed behind the first step's count; three passes of the device scan instead of one workgroup."""
    r = R.many_meshes()
    df = G.DevFrame(r.f.pos, r.f.color, r.f.idx, r.f.meshes)
    g = gpu_pick_rect(rt, gpu_ctx, df, r.queries, cap=64)
    assert_equals_model(g, r, 64)
    assert df.unchanged()


@pytest.mark.parametrize("name,n", R.CASES)
def test_degenerate_rectangle_is_vgx_pick(rt, gpu_ctx, name, n):
    """Kernels against kernels: a rectangle that is a point gives vgx_pick's four words for the same point, mesh_end and flags."""
    import test_pick_rect_cpu as cpu
    r = R.frame(name, n)
    df = G.dev_frame(r.f)
    sel, pq = cpu.point_queries(r)
    assert sel.size >= 40
    hits = G.gpu_pick(rt, gpu_ctx, df, pq)
    g = gpu_pick_rect(rt, gpu_ctx, df, r.queries[sel])
    assert same(g.top, hits), np.nonzero((g.top.view(np.uint32).reshape(-1, 4) != hits.view(np.uint32).reshape(-1, 4)).any(axis=1))[0][:8]


@pytest.mark.parametrize("grid", [1, 3])
def test_many_tiles_per_workgroup(rt, grid):
    """VGX_PICK_GRID (read when the context is created): one and three workgroups stride over every tile of the 257-instance frame, the
    last tile partial."""
    r = R.frame(*R.BIG)
    df = G.dev_frame(r.f)
    os.environ["VGX_PICK_GRID"] = str(grid)
    try:
        ctx2 = rt.Context(0)
    finally:
        del os.environ["VGX_PICK_GRID"]
    try:
        sl = slice(0, 64)
        g = gpu_pick_rect(rt, ctx2, df, r.queries[sl])
    finally:
        ctx2.close()
    assert_equals_model(g, r, R.LIST_CAP, sl)
    assert int((g.count > 0).sum()) > 20


@pytest.mark.parametrize("nq", [1, 63, 64])
@pytest.mark.parametrize("cap", [0, 1, 8])
def test_query_counts_and_capacities(rt, gpu_ctx, nq, cap):
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    sl = slice(64, 64 + nq)
    g = gpu_pick_rect(rt, gpu_ctx, df, r.queries[sl], cap=cap)
    assert_equals_model(g, r, cap, sl, ("top", "list", "count") if cap else ("top", "count"))


@pytest.mark.parametrize("mask,value", [(WINDOW | BY_DRAW, 0), (WINDOW | BY_DRAW, BY_DRAW), (WINDOW | BY_DRAW, WINDOW), (WINDOW | BY_DRAW, WINDOW | BY_DRAW)])
def test_one_kind_of_query_per_call(rt, gpu_ctx, mask, value):
    """Calls whose queries all lack VGX_PICK_RECT_WINDOW, VGX_PICK_RECT_BY_DRAW or both, on a context whose scratch holds the planes of
    earlier calls: a plane that such a call does not write must not be read from what an earlier call left."""
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    mixed = gpu_pick_rect(rt, gpu_ctx, df, r.queries[:64])  # every plane written, with other queries' bits
    assert_equals_model(mixed, r, R.LIST_CAP, slice(0, 64))
    sel = np.nonzero((r.queries["flags"] & mask) == value)[0][:64]
    assert sel.size >= 8 and int((r.answer.count[sel] > 0).sum()) >= 4
    g = gpu_pick_rect(rt, gpu_ctx, df, r.queries[sel])
    assert same(g.top, r.answer.top[sel]) and np.array_equal(g.count, r.answer.count[sel])
    assert np.array_equal(g.list, R.lists(r.answer, R.LIST_CAP, PATTERN)[sel])


@pytest.mark.parametrize("want", [("list", "count"), ("top", "count"), ("top", "list")])
def test_null_outputs(rt, gpu_ctx, want):
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    sl = slice(0, 64)
    assert_equals_model(gpu_pick_rect(rt, gpu_ctx, df, r.queries[sl], want=want), r, R.LIST_CAP, sl, want)


def test_refused_and_empty_calls(rt, gpu_ctx):
    import torch
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    q = G.to_dev(np.resize(r.queries, 65))
    top = torch.full((66 * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
    lst = torch.full((66 * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((66,), PATTERN, dtype=torch.int32, device="cuda:0")
    lib = rt.lib()

    def call(desc=df.desc, bounds=None, queries=q.data_ptr(), nq=1, top_p=top.data_ptr(), list_p=lst.data_ptr(), count_p=cnt.data_ptr(), cap=4, reserved=0):
        o = capi.PickRectOut(top_p, list_p, count_p, cap, reserved)
        return lib.vgx_pick_rect(gpu_ctx.handle, C.byref(desc), bounds, queries, nq, C.byref(o), rt._stream_ptr())

    assert call(nq=65) == capi.VGX_E_RANGE
    assert call(queries=None) == capi.VGX_E_INVALID_ARG
    assert call(list_p=None) == capi.VGX_E_INVALID_ARG
    assert call(reserved=1) == capi.VGX_E_INVALID_ARG
    assert call(queries=q.data_ptr() + 4) == capi.VGX_E_INVALID_ARG
    assert call(top_p=top.data_ptr() + 8) == capi.VGX_E_INVALID_ARG
    assert call(list_p=lst.data_ptr() + 2) == capi.VGX_E_INVALID_ARG
    assert call(bounds=df.t[0].data_ptr() + 8) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_pick_rect(gpu_ctx.handle, C.byref(df.desc), None, q.data_ptr(), 1, None, rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert call(queries=None, nq=0) == capi.VGX_OK
    torch.cuda.synchronize()
    assert bool((top == PATTERN).all()) and bool((lst == PATTERN).all()) and bool((cnt == PATTERN).all())
    # no meshes: valid, every count 0, every top "none", no list entry
    none = capi.CacheDesc(None, None, None, None, 0, 0, 0)
    assert call(desc=none, nq=5) == capi.VGX_OK
    torch.cuda.synchronize()
    t, c = top.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert np.all(t[:20] == NONE) and np.all(t[20:] == PATTERN) and np.all(c[:5] == 0) and np.all(c[5:] == PATTERN) and bool((lst == PATTERN).all())


def test_consecutive_calls_keep_nothing(rt, gpu_ctx):
    """Two calls on one context, nothing synchronised in between, through the runtime wrapper: the first selects almost everywhere, the
    second nowhere (an empty range): words that a call did not reset would carry bits over. And the same bytes on every run."""
    import torch
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    sel = np.nonzero(r.answer.count > 0)[0][:64]
    qa = r.queries[sel]
    qb = qa.copy()
    qb["mesh_end"] = 0
    da, db = G.to_dev(qa), G.to_dev(qb)
    ra = rt.pick_rect(gpu_ctx, df.desc, da, sel.size, list_cap=R.LIST_CAP)
    rb = rt.pick_rect(gpu_ctx, df.desc, db, sel.size, list_cap=R.LIST_CAP)
    rc = rt.pick_rect(gpu_ctx, df.desc, da, sel.size, list_cap=R.LIST_CAP, bounds_dev=G.gpu_bounds(rt, gpu_ctx, df), want_top=False)
    torch.cuda.synchronize()
    assert same(ra.top.cpu().numpy()[:sel.size * 16].view(capi.pick_hit_dtype), r.answer.top[sel])
    assert np.array_equal(ra.count.cpu().numpy().view(np.uint32), r.answer.count[sel])
    assert np.all(rb.count.cpu().numpy() == 0) and np.all(rb.top.cpu().numpy()[:sel.size * 16].view(np.uint32) == NONE)
    assert rc.top is None and np.array_equal(rc.count.cpu().numpy().view(np.uint32), r.answer.count[sel])
    la, lc = ra.list.cpu().numpy().view(np.uint32), rc.list.cpu().numpy().view(np.uint32)
    for i, k in enumerate(sel):
        n = min(int(r.answer.count[k]), R.LIST_CAP)
        assert np.array_equal(la[i, :n], r.answer.entries[k][:n]) and np.array_equal(lc[i, :n], la[i, :n])


def test_pick_tables_survive(rt, gpu_ctx):
    """vgx_pick -> vgx_pick_rect -> vgx_pick gives the same hits: the region query has scratch of its own."""
    import torch
    r = R.frame("tiger", 65)
    f = r.f
    df = G.dev_frame(f)
    dq = G.to_dev(f.queries[:256])
    h1 = rt.pick(gpu_ctx, df.desc, dq, 256)
    rr = rt.pick_rect(gpu_ctx, df.desc, G.to_dev(r.queries[:64]), 64, list_cap=R.LIST_CAP)
    h2 = rt.pick(gpu_ctx, df.desc, dq, 256)
    torch.cuda.synchronize()
    assert same(h1.cpu().numpy()[:256 * 16].view(capi.pick_hit_dtype), f.hits[:256])
    assert same(h2.cpu().numpy()[:256 * 16].view(capi.pick_hit_dtype), f.hits[:256])
    assert np.array_equal(rr.count.cpu().numpy().view(np.uint32), r.answer.count[:64])


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_pick_rect -> vgx_tessellate_emit gives the meshes it gives without the region query (the oracle's)."""
    import torch
    r = R.frame("tiger", 65)
    df = G.dev_frame(r.f)
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    rr = rt.pick_rect(gpu_ctx, df.desc, G.to_dev(r.queries[:64]), 64, list_cap=R.LIST_CAP)
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
    for name in ref.meshes.dtype.names:
        assert np.array_equal(gm[name], ref.meshes[name]), name
    assert np.array_equal(rr.count.cpu().numpy().view(np.uint32), r.answer.count[:64])
    assert same(rr.top.cpu().numpy()[:64 * 16].view(capi.pick_hit_dtype), r.answer.top[:64])
