"""The generator and the models of tests/mesh_streams.py, without a GPU: invariants of the made-up streams, merge_model on a case
written out by hand and against the reference's own frames (a tessellated frame split in two and merged again is the frame), and the
oracle's verdict on every cached frame tests/test_gpu_mesh_streams.py submits."""
import numpy as np
import pytest

import mesh_streams as MS

capi = MS.capi


def fields_equal(a, b):
    assert a.shape == b.shape
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f


def assert_same_stream(got, want):
    assert np.array_equal(got.pos.view(np.uint32), want.pos.view(np.uint32))
    assert np.array_equal(got.color, want.color)
    assert np.array_equal(got.idx, want.idx)
    fields_equal(got.meshes, want.meshes)


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("n,maxv", [(0, 6), (1, 6), (300, 6), (5000, 40)])
def test_generator_invariants(n, maxv, holes):
    r = MS.make_stream(np.random.RandomState(n + maxv), n, maxv, 37, holes=holes)
    m = r.meshes
    assert m.dtype == capi.mesh_dtype and m.shape == (n,)
    assert r.pos.dtype == np.float32 and r.pos.shape == (r.sizes["num_vertices"], 2) and r.color.shape == (r.sizes["num_vertices"],)
    assert r.idx.dtype == np.uint16 and r.idx.shape == (r.sizes["num_indices"],)
    fv, fi, nv, ni = (m[f].astype(np.int64) for f in ("first_vertex", "first_index", "num_vertices", "num_indices"))
    end_v, end_i = np.append(fv[1:], r.sizes["num_vertices"]), np.append(fi[1:], r.sizes["num_indices"])
    gv, gi = end_v - fv - nv, end_i - fi - ni  # what lies between a mesh and its successor (or the end of the stream)
    if n and not holes:
        assert fv[0] == 0 and fi[0] == 0 and np.all(gv == 0) and np.all(gi == 0)
    elif n:
        assert np.all((gv >= 0) & (gv <= 5)) and np.all((gi >= 0) & (gi <= 5)) and fv[0] <= 5 and fi[0] <= 5
    if n >= 300:
        assert np.all(np.diff(m["draw"].astype(np.int64)) >= 0) and int(m["draw"].max()) < 37 and np.any(np.diff(m["draw"]) == 0)
        assert nv.max() <= maxv and np.any(nv == 0) and np.any(nv == maxv)
        assert np.all(ni % 3 == 0) and np.all(ni[nv < 3] == 0) and np.all(ni[nv >= 3] > 0)
        assert np.any(ni % 2 == 1) and np.any((ni % 2 == 0) & (ni > 0))
        assert set(int(k) for k in m["subpath_kind"] >> 28) == set(MS.ALL_KINDS) and np.any(m["subpath_kind"] & 0x0FFFFFFF)
        assert set(int(x) for x in fi % 4) == {0, 1, 2, 3} and set(int(x) for x in fi % 2) == {0, 1}
        assert np.all(np.abs(r.pos) <= 1000.0) and np.abs(r.pos).max() > 900.0
        if holes:
            assert np.any(gv > 0) and np.any(gi > 0) and np.any(gv == 0)
    owner = np.repeat(np.arange(n), ni)
    at = np.repeat(fi - (np.cumsum(ni) - ni), ni) + np.arange(int(ni.sum()))
    assert np.all(r.idx[at].astype(np.int64) < nv[owner])


def test_generator_takes_given_vertex_counts():
    nv = [0, 3] + [65536] * 10 + [65537] * 10
    r = MS.make_stream(np.random.RandomState(1), 22, 0, 2, num_vertices=nv)
    m = r.meshes
    assert m["num_vertices"].tolist() == nv and r.pos.shape[0] == sum(nv) and m["num_indices"][0] == 0 and m["num_indices"][1] == 9
    per = [r.idx[int(f):int(f) + int(c)].astype(np.int64) for f, c in zip(m["first_index"], m["num_indices"])]
    assert np.all(per[1] < 3)
    # a uint16 index reaches vertex 65 535 and no further: the indices of the large meshes spread over all of that range (the generator
    # draws below min(num_vertices, 65 536), so none of a 65 537-vertex mesh is wrapped from 65 536 to 0)
    for big in (np.concatenate(per[2:12]), np.concatenate(per[12:])):
        assert big.shape[0] > 200 and big.max() > 65000 and big.min() < 500 and np.unique(big // 8192).shape[0] == 8


def _hand_stream(nv, ni, draw, kind, pos0, idx):
    r = MS.pyoracle.MeshResult()
    m = np.zeros(len(nv), dtype=capi.mesh_dtype)
    m["num_vertices"], m["num_indices"], m["draw"], m["subpath_kind"] = nv, ni, draw, kind
    m["first_vertex"], m["first_index"] = np.cumsum(nv) - nv, np.cumsum(ni) - ni
    t = int(np.sum(nv))
    r.pos = np.stack([pos0 + np.arange(t), -(pos0 + np.arange(t))], axis=1).astype(np.float32)
    r.color = (np.uint32(pos0) + np.arange(t)).astype(np.uint32)
    r.idx = np.asarray(idx, dtype=np.uint16)
    r.meshes = m
    return r


def test_merge_model_by_hand():
    """A: draws 1, 4, 4 (3, 0 and 4 vertices); B: draws 0, 4, 9 (3, 3, 1 vertices). B's first mesh goes in front of all of A (a
    B-before-A draw), B's draw-4 mesh behind BOTH draw-4 meshes of A (the tie), the zero-vertex mesh keeps its place and moves nothing."""
    a = _hand_stream([3, 0, 4], [3, 0, 6], [1, 4, 4], [0x10000001, 0x20000002, 0x30000003], 100, [0, 1, 2, 0, 1, 2, 0, 2, 3])
    b = _hand_stream([3, 3, 1], [3, 6, 0], [0, 4, 9], [0x50000005, 0x60000006, 0x70000007], 200, [2, 1, 0, 0, 1, 2, 2, 1, 0])
    r = MS.merge_model(a, b)
    assert r.order.tolist() == [3, 0, 1, 2, 4, 5]
    m = r.meshes
    assert m["draw"].tolist() == [0, 1, 4, 4, 4, 9]
    assert m["num_vertices"].tolist() == [3, 3, 0, 4, 3, 1] and m["first_vertex"].tolist() == [0, 3, 6, 6, 10, 13]
    assert m["num_indices"].tolist() == [3, 3, 0, 6, 6, 0] and m["first_index"].tolist() == [0, 3, 6, 6, 12, 18]
    assert m["subpath_kind"].tolist() == [0x50000005, 0x10000001, 0x20000002, 0x30000003, 0x60000006, 0x70000007]
    assert r.pos[:, 0].tolist() == [200, 201, 202, 100, 101, 102, 103, 104, 105, 106, 203, 204, 205, 206]
    assert np.array_equal(r.pos[:, 1], -r.pos[:, 0]) and np.array_equal(r.color, r.pos[:, 0].astype(np.uint32))
    assert r.idx.tolist() == [2, 1, 0, 0, 1, 2, 0, 1, 2, 0, 2, 3, 0, 1, 2, 2, 1, 0]
    # b_draw overrides B's own draw field, for the order and for the records
    r2 = MS.merge_model(a, b, b_draw=[1, 1, 3])
    assert r2.order.tolist() == [0, 3, 4, 5, 1, 2] and r2.meshes["draw"].tolist() == [1, 1, 1, 3, 4, 4]
    # the UV stream: white everywhere, B's rows over the vertices of B's meshes
    b_uv = (np.uint32(0xB0000000) + np.arange(7, dtype=np.uint32)).reshape(7, 1)
    uv = MS.merge_uv_model(r.order, a, b, b_uv, (0xFFFF,), 4)
    W = 0xFFFF
    assert uv[:, 0].tolist() == [0xB0000000, 0xB0000001, 0xB0000002, W, W, W, W, W, W, W, 0xB0000003, 0xB0000004, 0xB0000005, 0xB0000006]


@pytest.mark.parametrize("split", ["even_odd", "thirds_b_draw"])
def test_merge_model_gives_back_a_split_reference_frame(wl, oracle, split):
    ps, d = wl.tiger(1)
    frame = oracle.tessellate(ps, d)
    draw = frame.meshes["draw"]
    in_b = (draw % 2 == 1) if split == "even_odd" else (draw % 3 == 0)
    a, b = MS.repack(frame, ~in_b), MS.repack(frame, in_b)
    assert a.meshes.shape[0] > 50 and b.meshes.shape[0] > 50
    b_draw = None
    if split == "thirds_b_draw":
        b_draw = b.meshes["draw"].copy()
        b.meshes["draw"] = np.random.RandomState(3).permutation(b.meshes.shape[0]).astype(np.uint32) + 5  # scrambled: must not be read
    assert_same_stream(MS.merge_model(a, b, b_draw), frame)


def test_oracle_accepts_every_cached_frame(oracle):
    """What the oracle leaves out, the GPU test leaves out: nothing. Every listed frame is accepted by vgo_cache_submit with the totals
    the records give, and by vgo_assemble at the vertex-buffer size the GPU test arms."""
    assert MS.left_out() == []
    for ninst, _ in MS.CACHE_FRAMES:
        cache, inst, ref = MS.cache_frame(ninst)
        nm, nv, ni = MS.instance_totals(cache, inst)
        assert (ref.sizes["num_meshes"], ref.sizes["num_vertices"], ref.sizes["num_indices"]) == (nm, nv, ni)
        assert len(oracle.assemble(ref.meshes, ref.idx, MS.CACHE_MAX_VB)[1]) > 1
        e = inst["num_meshes"] == 0
        assert e[:3].all() and e[-2:].all() and e[250:520].all() and np.any(e & (inst["first_mesh"] == MS.CACHE_MESHES))
        assert not np.any(np.all(inst["mtx"][:, :4] == 0, axis=1) & e) and np.any(np.all(inst["mtx"][:, :4] == 0, axis=1))
        assert int(inst["num_meshes"].max()) == 4 and np.array_equal(ref.meshes["draw"], np.repeat(np.arange(ninst), inst["num_meshes"]))
        # instance colour (non-AA kinds) and stored colours (AA kinds) alternate inside one instance range
        uniform = np.isin(ref.meshes["subpath_kind"] >> 28, (capi.MESH_FILL, capi.MESH_STROKE))
        same_inst = ref.meshes["draw"][1:] == ref.meshes["draw"][:-1]
        assert np.any(same_inst & (uniform[1:] != uniform[:-1]))


@pytest.mark.parametrize("n,max_vb,split", [(1025, 4096, False), (40000, 64, True), (131073, 700, True)])
def test_oracle_accepts_every_merged_frame(oracle, n, max_vb, split):
    a, b, b_draw, draws = MS.merge_case(n)
    merged = MS.merge_model(a, b, b_draw)
    keys = draws["state_key"][merged.meshes["draw"]] if split else None
    st, cmds, idx = oracle.assemble(merged.meshes, merged.idx, max_vb, mesh_keys=keys)
    assert st == 0 and len(cmds) >= (1 if not split else 1000)
    if split:
        assert len(set(cmds["state_key"].tolist())) == 4 and np.any(cmds["first_vertex_in_vb"] != 0)
