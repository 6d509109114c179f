"""GPU: vgx_pick (csrc/vgx_pick.hip) against the numpy statement of the specification (tests/pick_model.py) on frames written by the
reference. Every comparison is exact: all four words of every hit. The frames, the query sets and the model's answers are those of
tests/test_pick_cpu.py; here the kernels answer. The shapes are the smallest at which the kernels can go wrong: the `walk` meshes
(8 008 vertices) cross several tiles, the 1-3-mesh Tiger ranges put many tiny meshes into one tile; nothing is full size."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import pick_model as P

pytestmark = pytest.mark.gpu
capi = P.capi
CM = P.CM
F = np.float32
NONE = P.NONE
PATTERN = 0x5A5A5A5A


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def to_dev(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(16, dtype=np.uint8)).to("cuda:0")


class DevFrame:
    """The four streams of a frame in device memory and the descriptor vgx_pick takes."""

    def __init__(self, pos, color, idx, meshes):
        self.host = (np.ascontiguousarray(pos, dtype=F), np.ascontiguousarray(color, dtype=np.uint32), np.ascontiguousarray(idx, dtype=np.uint16),
                     np.ascontiguousarray(meshes))
        self.t = [to_dev(a) for a in self.host]
        self.nm, self.nv, self.ni = meshes.shape[0], self.host[0].shape[0], self.host[2].shape[0]
        self.desc = capi.CacheDesc(self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(), self.nm, self.nv, self.ni)

    def unchanged(self):
        return all(np.array_equal(t.cpu().numpy()[:h.nbytes], h.view(np.uint8).reshape(-1)) for t, h in zip(self.t, self.host))


_frames = {}


def dev_frame(f):
    if f.key not in _frames:
        _frames[f.key] = DevFrame(f.pos, f.color, f.idx, f.meshes)
    return _frames[f.key]


def gpu_bounds(rt, ctx, df):
    import torch
    out = torch.empty((max(df.nm, 1), 4), dtype=torch.float32, device="cuda:0")
    assert rt.lib().vgx_mesh_bounds(ctx.handle, df.t[0].data_ptr(), df.t[3].data_ptr(), df.nm, out.data_ptr(), rt._stream_ptr()) == 0
    return out


def gpu_pick(rt, ctx, df, queries, bounds=None, guard=2):
    """vgx_pick in calls of at most 256 queries, each into a pattern-filled array: the records behind nqueries must stay as they were
    and the queries as they were."""
    import torch
    out = np.zeros(queries.shape[0], dtype=capi.pick_hit_dtype)
    for a, b in P.chunks(queries.shape[0]):
        q = to_dev(queries[a:b])
        h = torch.full(((b - a + guard) * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
        st = rt.lib().vgx_pick(ctx.handle, C.byref(df.desc), None if bounds is None else bounds.data_ptr(), q.data_ptr(), b - a, h.data_ptr(), rt._stream_ptr())
        torch.cuda.synchronize()
        assert st == capi.VGX_OK
        got = h.cpu().numpy().view(np.uint32)
        assert np.all(got[(b - a) * 4:] == PATTERN)
        assert np.array_equal(q.cpu().numpy()[:(b - a) * 16], np.ascontiguousarray(queries[a:b]).view(np.uint8).reshape(-1))
        out[a:b] = got[:(b - a) * 4].view(capi.pick_hit_dtype)
    return out


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def mismatches(a, b):
    return np.nonzero((a.view(np.uint32).reshape(-1, 4) != b.view(np.uint32).reshape(-1, 4)).any(axis=1))[0][:8]


@pytest.mark.parametrize("name,n", P.CASES)
def test_kernel_equals_model(rt, gpu_ctx, name, n):
    f = P.frame(name, n)
    P.check_query_conditions(f)
    df = dev_frame(f)
    mb = gpu_bounds(rt, gpu_ctx, df)
    with_boxes = gpu_pick(rt, gpu_ctx, df, f.queries, mb)
    assert same(with_boxes, f.hits), mismatches(with_boxes, f.hits)
    own_boxes = gpu_pick(rt, gpu_ctx, df, f.queries, None)
    assert same(own_boxes, with_boxes), mismatches(own_boxes, with_boxes)
    assert df.unchanged()
    assert np.array_equal(mb.cpu().numpy()[:df.nm], CM.mesh_boxes(f.pos, f.meshes))  # mesh_bounds as it was, too


@pytest.mark.parametrize("grid", [1, 3])
def test_many_tiles_per_workgroup(rt, grid):
    """VGX_PICK_GRID (read when the context is created): one and three workgroups stride over every tile of the 257-instance frame, the
    last tile partial."""
    f = P.frame(*P.BIG)
    df = dev_frame(f)
    os.environ["VGX_PICK_GRID"] = str(grid)
    try:
        ctx2 = rt.Context(0)
    finally:
        del os.environ["VGX_PICK_GRID"]
    try:
        q = f.queries[:512]
        got = gpu_pick(rt, ctx2, df, q, None)
    finally:
        ctx2.close()
    assert same(got, f.hits[:512]), mismatches(got, f.hits[:512])
    assert int((got["mesh"] != NONE).sum()) > 100


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 256])
def test_query_counts(rt, gpu_ctx, nq):
    f = P.frame("tiger", 65)
    df = dev_frame(f)
    got = gpu_pick(rt, gpu_ctx, df, f.queries[:nq], None)
    assert same(got, f.hits[:nq]), mismatches(got, f.hits[:nq])


def test_refused_and_empty_calls(rt, gpu_ctx):
    import torch
    f = P.frame("tiger", 65)
    df = dev_frame(f)
    q = to_dev(np.resize(f.queries, 257))
    h = torch.full((258 * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
    lib = rt.lib()
    # 257 queries: refused on the host, nothing enqueued, nothing written
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(df.desc), None, q.data_ptr(), 257, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_RANGE
    torch.cuda.synchronize()
    assert bool((h == PATTERN).all())
    # null and misaligned pointers
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(df.desc), None, None, 1, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(df.desc), None, q.data_ptr(), 1, None, rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(df.desc), None, q.data_ptr() + 4, 1, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(df.desc), df.t[0].data_ptr() + 8, q.data_ptr(), 1, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    assert lib.vgx_pick(gpu_ctx.handle, None, None, q.data_ptr(), 1, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_INVALID_ARG
    big = capi.CacheDesc(df.desc.pos, df.desc.color, df.desc.idx, df.desc.meshes, 0xFFFFFFFF, df.nv, df.ni)
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(big), None, q.data_ptr(), 1, h.data_ptr(), rt._stream_ptr()) == capi.VGX_E_RANGE
    torch.cuda.synchronize()
    assert bool((h == PATTERN).all())
    # no meshes: valid, every hit is "none"
    none = capi.CacheDesc(None, None, None, None, 0, 0, 0)
    assert lib.vgx_pick(gpu_ctx.handle, C.byref(none), None, q.data_ptr(), 5, h.data_ptr(), rt._stream_ptr()) == capi.VGX_OK
    torch.cuda.synchronize()
    got = h.cpu().numpy().view(np.uint32)
    assert np.all(got[:20] == NONE) and np.all(got[20:] == PATTERN)


@pytest.fixture(scope="module")
def stacked():
    """64 whole-Tiger instances under the SAME transform: every mesh box of a drawing contains what its 63 copies contain, and many
    lanes of a wave hit the same query."""
    c = CM.case("tiger")
    inst = np.zeros(64, dtype=capi.cache_instance_dtype)
    inst["num_meshes"], inst["color"] = c.nm, 0xFF336699
    inst["mtx"][:] = [1.5, 0.25, -0.25, 1.5, 300.0, 200.0]
    fr = P.oracle.cache_submit(c.cache, inst)
    T = P.triangles(fr.pos, fr.color, fr.idx, fr.meshes)
    pts = [CM.xform(inst["mtx"][0], x, y) for x, y in P.deep_local_points(c)]
    pts += [tuple(fr.pos[v]) for v in range(0, c.cache.pos.shape[0], 997)]
    q = np.zeros(len(pts) + 4, dtype=capi.pick_query_dtype)
    q["x"][:len(pts)], q["y"][:len(pts)] = [p[0] for p in pts], [p[1] for p in pts]
    q["mesh_end"] = NONE
    q["x"][len(pts):], q["y"][len(pts):] = pts[0][0], pts[0][1]
    q["mesh_end"][len(pts):] = [c.nm * 64, c.nm * 63, c.nm, 1]  # the same point under a falling mesh_end
    q["flags"][::5] = capi.PICK_SKIP_TRANSPARENT
    hits, depth = P.pick(T, fr.meshes, q)
    return fr, q, hits, depth


def test_stacked_frame_takes_the_maximum(rt, gpu_ctx, stacked):
    fr, q, hits, depth = stacked
    nm1 = fr.meshes.shape[0] // 64
    hit = hits["mesh"] != NONE
    assert int((depth >= 128).sum()) >= 8 and int(hit.sum()) >= 20  # at least two meshes of each of the 64 copies
    assert np.all(hits["mesh"][hit & (q["mesh_end"] == NONE)] >= 63 * nm1) and np.all(hits["draw"][hit & (q["mesh_end"] == NONE)] == 63)  # the topmost copy
    df = DevFrame(fr.pos, fr.color, fr.idx, fr.meshes)
    got = gpu_pick(rt, gpu_ctx, df, q, None)
    assert same(got, hits), mismatches(got, hits)
    assert same(gpu_pick(rt, gpu_ctx, df, q, gpu_bounds(rt, gpu_ctx, df)), got)


def test_consecutive_calls_keep_nothing(rt, gpu_ctx):
    """Two calls on one context with different query sets, nothing synchronised in between: each gives its own result. The first set
    hits almost everywhere, the second nowhere: a key table that the call did not reset would carry hits over."""
    import torch
    f = P.frame("tiger", 65)
    df = dev_frame(f)
    sel = np.nonzero(f.hits["mesh"] != NONE)[0][:200]
    qa = f.queries[sel]
    qb = qa.copy()
    qb["mesh_end"] = 0
    da, db = to_dev(qa), to_dev(qb)
    ha = rt.pick(gpu_ctx, df.desc, da, qa.shape[0])
    hb = rt.pick(gpu_ctx, df.desc, db, qb.shape[0])
    hc = rt.pick(gpu_ctx, df.desc, da, qa.shape[0], bounds_dev=gpu_bounds(rt, gpu_ctx, df))
    torch.cuda.synchronize()
    assert same(ha.cpu().numpy()[:sel.size * 16].view(capi.pick_hit_dtype), f.hits[sel])
    assert np.all(hb.cpu().numpy()[:sel.size * 16].view(np.uint32) == NONE)
    assert same(hc.cpu().numpy()[:sel.size * 16].view(capi.pick_hit_dtype), f.hits[sel])


def test_skip_transparent_and_click_through(rt, gpu_ctx):
    f = P.frame("tiger", 65)
    df = dev_frame(f)
    q = f.queries[:256].copy()
    q["flags"][::2] = capi.PICK_SKIP_TRANSPARENT  # both rules in one call: the colours are gathered, half the queries ignore them
    want, _ = P.pick(f.tris, f.meshes, q)
    got = gpu_pick(rt, gpu_ctx, df, q, None)
    assert same(got, want), mismatches(got, want)
    assert not same(want, f.hits[:256])
    # click-through: mesh_end = the previous hit's mesh, down to "none"
    g = P.frame(*P.BIG)
    dg = dev_frame(g)
    qi = int(np.nonzero((g.kind == "stacked") & (g.depth >= 2))[0][0])
    x, y = g.queries["x"][qi], g.queries["y"][qi]
    stack = np.unique(g.tris.mesh[P.containing(g.tris, x, y)])[::-1].tolist()
    walked, end = [], NONE
    for _ in range(len(stack) + 1):
        one = np.zeros(1, dtype=capi.pick_query_dtype)
        one["x"], one["y"], one["mesh_end"] = x, y, end
        h = gpu_pick(rt, gpu_ctx, dg, one, None)[0]
        if h["mesh"] == NONE:
            break
        walked.append(int(h["mesh"]))
        end = int(h["mesh"])
    assert walked == stack and len(stack) >= 2


def test_malformed_tables(rt, gpu_ctx):
    """An index >= num_vertices, num_indices % 3 != 0, a mesh of 0 indices: hand-made tables over the real streams."""
    import test_pick_cpu as cpu
    f = P.frame("tiger", 65)
    q = cpu.malformed_queries(f)
    for what, meshes in cpu.malformed(f):
        want, _ = P.pick(P.triangles(f.pos, f.color, f.idx, meshes), meshes, q)
        df = DevFrame(f.pos, f.color, f.idx, meshes)
        got = gpu_pick(rt, gpu_ctx, df, q, None)
        assert same(got, want), (what, mismatches(got, want))


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_pick -> vgx_tessellate_emit gives the meshes it gives without the pick (the oracle's)."""
    import torch
    f = P.frame("tiger", 65)
    df = dev_frame(f)
    ps, d = wl.tiger(3)
    ref = oracle.tessellate(ps, d)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, d.shape[0])
    hits = rt.pick(gpu_ctx, df.desc, to_dev(f.queries[:256]), 256)
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
    assert same(hits.cpu().numpy()[:256 * 16].view(capi.pick_hit_dtype), f.hits[:256])
    # and on what the product itself just wrote: the pick of its own frame == the model on the oracle's
    qv = np.zeros(64, dtype=capi.pick_query_dtype)
    qv["x"], qv["y"], qv["mesh_end"] = ref.pos[::max(1, nv // 64)][:64, 0], ref.pos[::max(1, nv // 64)][:64, 1], NONE
    want, _ = P.pick(P.triangles(ref.pos, ref.color, ref.idx, ref.meshes), ref.meshes, qv)
    own = capi.CacheDesc(bufs.pos.data_ptr(), bufs.color.data_ptr(), bufs.idx.data_ptr(), bufs.meshes.data_ptr(), nm, nv, ni)
    got = rt.pick(gpu_ctx, own, to_dev(qv), 64)
    torch.cuda.synchronize()
    assert same(got.cpu().numpy()[:64 * 16].view(capi.pick_hit_dtype), want)
