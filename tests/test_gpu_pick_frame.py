"""GPU: vgx_pick_frame (csrc/vgx_pick.hip: k_pickf_meshes, the candidate scan, k_pickf_tris, k_pickf_contours, k_pickf_resolve) against the
numpy statement of the specification (tests/pick_frame_model.py), against the lane code (vgxt_pick_frame), against the image the
KERNELS of vgx_raster_concave draw of the ID frame (relation (a) of include/vgx.h) and against vgx_pick where the two must agree (relation
(b)). Every comparison is exact: all four words of every hit. Frames, query sets and answers are those of tests/test_pick_frame_cpu.py.
The shapes are the smallest at which the kernels can go wrong: `stack_clip` puts more than 256 candidates on one tile under two regions (the
resolve stage carries a stamp across a chunk), `star300` has contour meshes of more edges than a wave, the `walk` meshes (8 008 vertices)
cross element tiles and wave windows."""
import ctypes as C

import numpy as np
import pytest

import pick_frame_model as PF
import raster_frame_model as M
import raster_harness as H
from raster_harness import first_difference, gpu_bounds, host, rt, same, to_dev  # noqa: F401 (host, rt: fixtures)

pytestmark = pytest.mark.gpu
capi = PF.capi
F = np.float32
NONE = PF.NONE
PATTERN = H.HITS_GUARD
ALL = H.OPEN


class Dev:
    """A frame and its draw table in device memory."""

    def __init__(self, f):
        self.f, self.frame, self.state = f, H.DevFrame(f), H.DevState(f)

    def unchanged(self):
        return self.frame.unchanged() and self.state.unchanged()


_devs = {}


def dev(key):
    if key not in _devs:
        _devs[key] = Dev(PF.frame(key))
    return _devs[key]


def gpu_pick_frame(rt, ctx, d, queries, bounds=None, begin=0, end=ALL, want=capi.VGX_OK, with_status=True, guard=2, chunk=capi.PICK_MAX_QUERIES):
    """vgx_pick_frame in calls of at most `chunk` queries, each into a pattern-filled array: the records behind nqueries and the words
    beside dev_status must stay as they were, and the queries as they were."""
    import torch
    out = np.zeros(queries.shape[0], dtype=capi.pick_hit_dtype)
    for a, b in PF.chunks(queries.shape[0], chunk) or [(0, 0)]:
        q = to_dev(queries[a:b])
        h = torch.full(((b - a + guard) * 4,), PATTERN, dtype=torch.int32, device="cuda:0")
        status = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
        st = rt.lib().vgx_pick_frame(ctx.handle, C.byref(d.frame.desc), None if bounds is None else bounds.data_ptr(), begin, end, C.byref(d.state.struct),
                                     q.data_ptr() if b > a else None, b - a, h.data_ptr(), status.data_ptr() if with_status else None, rt._stream_ptr())
        torch.cuda.synchronize()
        assert st == capi.VGX_OK
        assert status.cpu().tolist() == ([want, 77, 77] if with_status else [77, 77, 77])
        got = h.cpu().numpy().view(np.uint32)
        assert np.all(got[(b - a) * 4:] == PATTERN)
        assert b == a or np.array_equal(q.cpu().numpy()[:(b - a) * 16], np.ascontiguousarray(queries[a:b]).view(np.uint8).reshape(-1))
        out[a:b] = got[:(b - a) * 4].view(capi.pick_hit_dtype)
    return out


@pytest.mark.parametrize("key", PF.ALL, ids=lambda k: "-".join(str(v) for v in k))
def test_kernels_equal_model_and_lane_code(rt, gpu_ctx, host, key):
    f, qs = PF.frame(key), PF.query_set(key)
    PF.check_conditions(key)
    want = PF.expected(key)
    d = dev(key)
    mb = gpu_bounds(rt, gpu_ctx, d.frame)
    with_boxes = gpu_pick_frame(rt, gpu_ctx, d, qs.queries, mb)
    assert same(with_boxes, want.hits), first_difference(with_boxes, want.hits, qs.queries)
    own_boxes = gpu_pick_frame(rt, gpu_ctx, d, qs.queries, None, with_status=False)
    assert same(own_boxes, with_boxes), first_difference(own_boxes, with_boxes, qs.queries)
    if key in PF.IMAGES:  # the reference's streams are large for a sequential loop; tests/test_pick_frame_cpu.py holds the lane code to the same model
        assert same(H.host_pick_frame(host, f, qs.queries), with_boxes)
    assert d.unchanged()
    assert np.array_equal(mb.cpu().numpy()[:f.nm], PF.CM.mesh_boxes(f.pos, f.meshes))  # mesh_bounds as it was, too


@pytest.mark.parametrize("nq", [0, 1, 65, 256])
def test_query_counts(rt, gpu_ctx, nq):
    key = ("concave", "state")
    qs, want = PF.query_set(key), PF.expected(key)
    lo = qs.centres - nq // 2  # pixel centres and off-centre points in one call
    got = gpu_pick_frame(rt, gpu_ctx, dev(key), qs.queries[lo:lo + nq], chunk=max(nq, 1))
    assert same(got, want.hits[lo:lo + nq])


def device_ids(rt, ctx, f, begin=0):
    g, tgt = PF.id_frame(f)
    rt.raster_reserve(ctx, 8192, 1 << 17)  # the bin tables ahead, so that no call ends with VGX_E_GROWN
    return PF.decode_ids(H.gpu_level(rt, ctx, "concave", *H.dev_parts(g), tgt, begin=begin)[1], tgt)


@pytest.mark.parametrize("key", [("concave", "state"), ("frame", "stack_clip"), ("concave", "centres"), ("concave", "star300"), ("frame", "decoded")],
                         ids=lambda k: k[1])
def test_relation_a_the_image_is_the_oracle(rt, gpu_ctx, key):
    """vgx_pick_frame at every pixel centre against vgx_raster_concave of the ID frame, both run by the kernels."""
    f = M.frame("decoded", rt) if key[1] == "decoded" else PF.frame(key)
    ids = device_ids(rt, gpu_ctx, f)
    got = gpu_pick_frame(rt, gpu_ctx, Dev(f) if key[1] == "decoded" else dev(key), PF.centre_queries(f.target))
    mesh = np.where(got["mesh"] == NONE, -1, got["mesh"].astype(np.int64)).reshape(f.target.height, f.target.width)
    assert np.array_equal(mesh, ids), np.argwhere(mesh != ids)[:5]
    assert (ids >= 0).any() and np.unique(ids).size >= 3


def test_relation_b_equals_vgx_pick_away_from_edges(rt, gpu_ctx):
    f, q, want = H.relation_b_queries()
    d = dev(PF.TIGER)
    got = gpu_pick_frame(rt, gpu_ctx, d, q)
    old = H.gpu_pick(rt, gpu_ctx, d.frame, q)
    assert same(got, want)
    assert same(got, old), first_difference(got, old, q)
    assert int((got["mesh"] != NONE).sum()) > 100


def test_range_and_invalid_draw(rt, gpu_ctx):
    key = ("frame", "clips")
    f = PF.frame(key)
    q = PF.centre_queries(f.target)[:1024]
    want = PF.pick(f, q, mesh_begin=5, prep=PF._prepare_cached(key))
    assert same(gpu_pick_frame(rt, gpu_ctx, dev(key), q, begin=5), want.hits)
    assert same(gpu_pick_frame(rt, gpu_ctx, dev(key), q, end=4), PF.pick(f, q, mesh_end=4, prep=PF._prepare_cached(key)).hits)
    g = PF.R.make("clips_bad", f.pos, f.color, f.idx, f.meshes.copy(), f.target)
    g.draws, g.dstate = f.draws, f.dstate
    g.meshes["draw"][7] = f.draws.shape[0]
    bad = Dev(g)
    got = gpu_pick_frame(rt, gpu_ctx, bad, q[:300], want=capi.VGX_E_INVALID_ARG)
    assert (got.view(np.uint32) == NONE).all()
    assert same(gpu_pick_frame(rt, gpu_ctx, bad, q[:300], end=7), PF.pick(f, q[:300], mesh_end=7, prep=PF._prepare_cached(key)).hits)
    gpu_pick_frame(rt, gpu_ctx, bad, q[:0], want=capi.VGX_E_INVALID_ARG)
    gpu_pick_frame(rt, gpu_ctx, bad, q[:0], begin=9, end=9)  # an empty range: VGX_OK


def test_click_through_on_the_device(rt, gpu_ctx):
    key = ("frame", "stack_clip")
    qs, a = PF.query_set(key), PF.expected(key)
    qi = max(range(qs.centres), key=lambda q: len(a.stack[q]))
    assert len(a.stack[qi]) > 100
    got, end = [], NONE
    for _ in range(12):
        q = qs.queries[qi:qi + 1].copy()
        q["mesh_end"] = end
        h = gpu_pick_frame(rt, gpu_ctx, dev(key), q)[0]
        got.append(int(h["mesh"]))
        end = int(h["mesh"])
    assert got == a.stack[qi][:12]


def test_no_leak_between_calls(rt, gpu_ctx):
    """vgx_pick, vgx_pick_frame, vgx_pick on one context, then two vgx_pick_frame calls of 256 queries and of 1: each its own answers."""
    key = PF.TIGER
    f, qs, want = PF.frame(key), PF.query_set(key), PF.expected(key)
    d = dev(key)
    pq = f.pick.queries[:256]
    first = H.gpu_pick(rt, gpu_ctx, d.frame, pq)
    assert same(first, f.pick.hits[:256])
    assert same(gpu_pick_frame(rt, gpu_ctx, d, qs.queries[:256]), want.hits[:256])
    assert same(H.gpu_pick(rt, gpu_ctx, d.frame, pq), first)
    key = ("concave", "star300")
    qs, want = PF.query_set(key), PF.expected(key)
    hit = int(np.nonzero(want.hits["mesh"][:qs.centres] != NONE)[0][0])
    miss = int(np.nonzero(want.hits["mesh"][:qs.centres] == NONE)[0][0])
    for one in (miss, hit, miss):
        lo = min(hit, max(0, qs.centres - 256))
        assert same(gpu_pick_frame(rt, gpu_ctx, dev(key), qs.queries[lo:lo + 256]), want.hits[lo:lo + 256])
        assert same(gpu_pick_frame(rt, gpu_ctx, dev(key), qs.queries[one:one + 1]), want.hits[one:one + 1])


def test_scratch_bytes(rt):
    """The call keeps 84 bytes per mesh of the range, 16 more per mesh of the frame without mesh_bounds (and the head room of every scratch
    table); vgx_pick's tables are not touched."""
    key = PF.TIGER
    f, qs = PF.frame(key), PF.query_set(key)
    ctx = rt.Context(0)
    try:
        lib = rt.lib()
        lib.vgx_scratch_bytes.restype = C.c_uint64
        d = Dev(f)
        mb = gpu_bounds(rt, ctx, d.frame)
        b0 = lib.vgx_scratch_bytes(ctx.handle)
        gpu_pick_frame(rt, ctx, d, qs.queries[:256], mb)
        b1 = lib.vgx_scratch_bytes(ctx.handle)
        fixed = 512 * 32 + 4 * 8
        assert 84 * f.nm <= b1 - b0 <= int(84 * (f.nm + 1) * 1.25) + fixed + 9 * 4096, (b0, b1, f.nm)
        gpu_pick_frame(rt, ctx, d, qs.queries[:256], None)
        b2 = lib.vgx_scratch_bytes(ctx.handle)
        assert 16 * f.nm <= b2 - b1 <= int(16 * f.nm * 1.25) + 4096, (b1, b2)
        gpu_pick_frame(rt, ctx, d, qs.queries[:256], None)
        assert lib.vgx_scratch_bytes(ctx.handle) == b2
    finally:
        ctx.close()


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_pick_frame on another stream -> vgx_tessellate_emit gives the meshes count -> emit gives (the oracle's)."""
    import torch
    key = ("concave", "state")
    qs, want = PF.query_set(key), PF.expected(key)
    ps, dr = wl.tiger(3)
    ref = oracle.tessellate(ps, dr)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(dr)
    sizes = rt.tessellate_count(gpu_ctx, pset, dd, dr.shape[0])
    d = dev(key)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hits, status = rt.pick_frame(gpu_ctx, d.frame.desc, d.state.t[0], d.state.t[1], d.f.draws.shape[0], to_dev(qs.queries[:256]), 256)
    bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(gpu_ctx, pset, dd, dr.shape[0], bufs)
    torch.cuda.synchronize()
    pset.close()
    nv, ni = ref.sizes["num_vertices"], ref.sizes["num_indices"]
    assert np.array_equal(bufs.pos[:nv].cpu().numpy().view(np.uint32), ref.pos.view(np.uint32))
    assert np.array_equal(bufs.color[:nv].cpu().numpy().view(np.uint32), ref.color)
    assert np.array_equal(bufs.idx[:ni].cpu().numpy().view(np.uint16), ref.idx)
    assert int(status.item()) == capi.VGX_OK
    assert same(hits.cpu().numpy()[:256 * 16].view(capi.pick_hit_dtype), want.hits[:256])
