"""What the two sides of vgx_concave_triangulate_nested's tests share (tests/test_concave_nested_cpu.py: the lane code;
tests/test_gpu_concave_nested.py: the kernels): the host entry's prototype, the batches built from the fixtures of
tests/concave_nested_model.py and of the rings model, what the model expects of them (computed once, never changed), and the checks
both sides run through a `tri` callable (Flat, capacities) -> (status, sizes, routes, streams, guards intact)."""
import ctypes as C

import numpy as np

import concave_nested_model as NM
import concave_rings_harness as RH
import concave_rings_model as RM
import concave_triangulate_harness as TH
import concave_triangulate_model as TM
import raster_harness as H
import raster_model as R
import stream_order_nested  # noqa: F401 (puts the entry's row into the table of tests/stream_order.py)

capi = R.capi
F = np.float32
OK = capi.VGX_OK
TARGET = RH.TARGET
check_images = RH.check_images
RINGS_BATCHES = {"rings_fixtures": "fixtures", "rings_mixed": "mixed", "rings_single": "single"}


def load_host():
    """TH.load_host() with this entry's prototype; a library from before this entry is rebuilt here, once."""
    lib = RH.load_host()
    if not hasattr(lib, "vgxt_concave_triangulate_nested"):
        import __graft_entry__ as g
        g.build()
        lib = RH.load_host()
    assert hasattr(lib, "vgxt_concave_triangulate_nested"), "libvgx_hosttest.so lacks vgxt_concave_triangulate_nested after a build"
    lib.vgxt_concave_triangulate_nested.restype = C.c_int
    lib.vgxt_concave_triangulate_nested.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(capi.MeshOut), C.c_void_p, C.POINTER(capi.Sizes), C.c_void_p, C.c_void_p]
    return lib


def names_of(name):
    if name == "fixtures":
        return list(NM.DRAWS) + list(NM.WORDS)
    if name == "imaged":   # everything with finite coordinates inside the target
        return list(NM.DRAWS) + list(NM.WORDS) + ["max_rings"]
    return [name]


def batch(name):
    """(specs, the routes the fixtures are FOR, or None where the model decides) of a named batch."""
    if name == "mixed":
        return NM.mixed_specs(), list(NM.MIXED_ROUTES)
    if name == "random":
        return RM.random_specs(), None
    if name in RINGS_BATCHES:   # the rings model's own batches; what it refused as NESTING may be triangles now
        return RH.batch(RINGS_BATCHES[name])[0], None
    names = names_of(name)
    return RH.recolour([NM.draw_spec(n) for n in names]), [NM.fixture(n)[3] for n in names]


_want = {}


def want(host, name):
    """(Flat, routes, pos, color, idx, meshes, notes) the model expects of a batch, on vgx_concave_contours' output for it."""
    if name not in _want:
        specs, meant = batch(name)
        fl = H.Flat(specs)
        notes = {}
        routes, pos, col, idx, meshes = NM.expected(specs, *TH.contours_of(host, fl), notes=notes)
        assert meant is None or routes.tolist() == meant, (name, routes.tolist(), meant)   # no fixture passes by falling back
        for a in (routes, pos, col, idx, meshes):
            a.setflags(write=False)
        _want[name] = (fl, routes, pos, col, idx, meshes, notes)
    return _want[name]


def host_triangulate(host, fl, out, with_routes=True, entry="nested"):
    """-> status, sizes, routes, trips (per draw the most candidates one bridge search tried)."""
    sizes, status = capi.Sizes(), np.full(1, 77, dtype=np.uint32)
    n = len(fl.specs)
    routes = np.full(n + 2, 0xA5A5A5A5, dtype=np.uint32)
    trips = np.zeros(n + 1, dtype=np.uint32)
    fn = host.vgxt_concave_triangulate_nested if entry == "nested" else host.vgxt_concave_triangulate_rings
    rc = fn(fl.poly.ctypes.data, fl.subs.ctypes.data, fl.info.ctypes.data, fl.draws.ctypes.data, n, C.byref(out.struct),
            routes.ctypes.data if with_routes else None, C.byref(sizes), status.ctypes.data, trips.ctypes.data)
    assert rc == OK and (routes[n:] == 0xA5A5A5A5).all()
    return int(status[0]), (int(sizes.num_meshes), int(sizes.num_vertices), int(sizes.num_indices)), routes[:n], trips[:n]


def check_against_model(host, name, tri):
    fl, routes, pos, col, idx, meshes, _ = want(host, name)
    caps = (len(pos), len(idx), len(meshes))
    st, sizes, got_routes, streams, intact = tri(fl, caps)
    assert got_routes.tolist() == routes.tolist()
    assert st == OK and sizes == (caps[2], caps[0], caps[1]) and intact
    gpos, gcol, gidx, gmeshes = streams
    assert gmeshes.tobytes() == meshes.tobytes(), [(tuple(a), tuple(b)) for a, b in zip(gmeshes, meshes) if a != b][:3]
    assert np.array_equal(gpos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(gcol, col) and np.array_equal(gidx, idx)


def draw_bytes(streams, d):
    """What draw d holds, free of its place in the streams: per mesh (num_vertices, num_indices, kind, position bits, colours, indices)."""
    pos, col, idx, meshes = streams
    out = []
    for m in meshes[meshes["draw"] == d]:
        a, n, b, q = int(m["first_vertex"]), int(m["num_vertices"]), int(m["first_index"]), int(m["num_indices"])
        out.append((n, q, int(m["subpath_kind"]), pos[a:a + n].view(np.uint32).tobytes(), col[a:a + n].tobytes(), idx[b:b + q].tobytes()))
    return out


def check_one_group_draws_equal_the_rings_entry(host, name, nested_streams, rings_streams, nested_routes, rings_routes, least):
    """Every draw of a rings-model batch with G <= 1 -- triangulated as one group, refused, or making nothing -- has the rings entry's
    route and bytes. G is the model's."""
    fl, routes, _, _, _, _, notes = want(host, name)
    assert nested_routes.tolist() == routes.tolist()
    seen = more = 0
    for d in range(len(fl.specs)):
        if routes[d] == TM.TRIANGLES and len(notes[d]["groups"]) > 1:
            assert rings_routes[d] == RM.NESTING
            more += 1
            continue
        assert nested_routes[d] == rings_routes[d], d
        assert draw_bytes(nested_streams, d) == draw_bytes(rings_streams, d), d
        seen += routes[d] == TM.TRIANGLES
    assert seen >= least
    return more


def group_specs(name):
    """Per group of a triangulated fixture: (the draw made of that group's sub-paths alone, its draw-local vertex numbers). With AA
    the groups are those of the rings as given: the inset moves no ring of a fixture across another."""
    rings, flags, fringe = NM.fixture(name)[:3]
    depth, outer = NM.classify([np.ascontiguousarray(r, dtype=F) for r in rings], bool(flags & TM.EO))
    groups = [[r for r in range(len(rings)) if outer[r] == o] for o in range(len(rings)) if outer[o] == o]
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(int)
    return [(([rings[r] for r in g], TM.CONCAVE | flags, TM.COLOR, fringe), np.concatenate([np.arange(start[r], start[r + 1]) for r in g])) for g in groups]


def check_groups_equal_the_rings_entry(name, nested_streams_of, rings_streams_of):
    """Each group's triangles equal the rings entry's on that group alone, the indices translated. With AA a draw's triangles sit behind
    its 6 V fringe indices and count from its 2 V fringe vertices: V of the whole draw here, V_g of the group there.
    *_streams_of: specs -> streams."""
    groups = group_specs(name)
    aa = bool(NM.fixture(name)[1] & TM.AA)
    V = sum(len(local) for _, local in groups)
    _, _, idx, meshes = nested_streams_of([NM.draw_spec(name)])
    assert len(meshes) == 1 and int(meshes[0]["subpath_kind"]) == TM.FILL_KIND
    tris = idx.astype(np.int64)[6 * V:] - 2 * V if aa else idx.astype(np.int64)
    _, _, gidx, gmeshes = rings_streams_of([spec for spec, _ in groups])   # one batch: a draw per group
    assert len(gmeshes) == len(groups) and (gmeshes["subpath_kind"] == TM.FILL_KIND).all() and gmeshes["draw"].tolist() == list(range(len(groups))), name
    at = 0
    for (spec, local), m in zip(groups, gmeshes):
        t = gidx[int(m["first_index"]):int(m["first_index"]) + int(m["num_indices"])].astype(np.int64)
        if aa:
            t = t[6 * len(local):] - 2 * len(local)
        assert len(t) and t.min() >= 0 and np.array_equal(local[t], tris[at:at + len(t)]), name
        at += len(t)
    assert at == len(tris) == 3 * NM.fixture(name)[5] and len(groups) == NM.fixture(name)[4]
    return len(groups)


def check_exact_areas(fl, routes, pos, idx, meshes):
    """Exact rational arithmetic on the output alone (the rings' depths from their geometry): every triangle of group g has the
    orientation of its outer ring or area 0, and the areas sum to the even-depth rings' less the odd-depth rings'."""
    seen = 0
    for m in meshes:
        d = int(m["draw"])
        if routes[d] != TM.TRIANGLES or (int(m["subpath_kind"]) >> 28) == capi.MESH_CONTOURS:
            continue
        lens = [len(q) for q in fl.specs[d][0]]
        V, S = sum(lens), len(lens)
        aa = bool(fl.specs[d][1] & TM.AA)
        fv, fi = int(m["first_vertex"]) + (2 * V if aa else 0), int(m["first_index"]) + (6 * V if aa else 0)
        verts = pos[fv:fv + V]
        rings = np.split(verts, np.cumsum(lens)[:-1])
        depth, outer = NM.classify(rings, True) if S > 1 else (np.zeros(1, dtype=int), np.zeros(1, dtype=int))
        groups = [o for o in range(S) if outer[o] == o]
        nt = V + 2 * S - 4 * len(groups)
        assert int(m["num_indices"]) == (6 * V if aa else 0) + 3 * nt and int(m["num_vertices"]) == (3 * V if aa else V)
        t = idx[fi:fi + 3 * nt].astype(np.int64).reshape(-1, 3) - (2 * V if aa else 0)
        assert t.min() >= 0 and t.max() < V
        ring_areas = [TH.ring_area2(r) for r in rings]
        ring_of = np.repeat(np.arange(S), lens)
        at = total = 0
        for o in groups:   # the triangles come group after group
            members = [r for r in range(S) if outer[r] == o]
            n = sum(lens[r] for r in members) + 2 * (len(members) - 1) - 2
            s = 1 if ring_areas[o] > 0 else -1
            mine = t[at:at + n]
            assert set(outer[ring_of[mine.reshape(-1)]].tolist()) == {o}, d
            areas = [TH.ring_area2(verts[list(tri)]) for tri in mine]
            assert all(a * s >= 0 for a in areas), d
            want_area = abs(ring_areas[o]) - sum(abs(ring_areas[r]) for r in members if r != o)
            assert want_area > 0 and sum(areas) * s == want_area, d
            at, total = at + n, total + want_area
        assert at == nt
        assert total == sum(abs(a) * (-1 if depth[r] & 1 else 1) for r, a in enumerate(ring_areas)), d
        seen += 1
    return seen
