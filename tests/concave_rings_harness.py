"""What the two sides of vgx_concave_triangulate_rings' tests share (tests/test_concave_rings_cpu.py: the lane code;
tests/test_gpu_concave_rings.py: the kernels): the host entry's prototype, the batches built from the fixtures of
tests/concave_rings_model.py, what the model expects of them (computed once, never changed), and the checks both sides run through a
`tri` callable (Flat, capacities) -> (status, sizes, routes, streams, guards intact)."""
import ctypes as C
from fractions import Fraction

import numpy as np

import concave_rings_model as RM
import concave_triangulate_harness as TH
import concave_triangulate_model as TM
import raster_harness as H
import raster_model as R
import stream_order_rings  # noqa: F401 (puts the entry's row into the table of tests/stream_order.py)

capi = R.capi
F = np.float32
OK = capi.VGX_OK
TARGET = R.Target(104, 100, 104, -2, -2)


def load_host():
    """TH.load_host() with this entry's prototype; a library from before this entry is rebuilt here, once."""
    lib = TH.load_host()
    if not hasattr(lib, "vgxt_concave_triangulate_rings"):
        import __graft_entry__ as g
        g.build()
        lib = TH.load_host()
    assert hasattr(lib, "vgxt_concave_triangulate_rings"), "libvgx_hosttest.so lacks vgxt_concave_triangulate_rings after a build"
    lib.vgxt_concave_triangulate_rings.restype = C.c_int
    lib.vgxt_concave_triangulate_rings.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(capi.MeshOut), C.c_void_p, C.POINTER(capi.Sizes), C.c_void_p, C.c_void_p]
    return lib


def recolour(specs):
    return [(s[0], s[1], (s[2] & 0xFF000000) | ((s[2] ^ (0x00010307 * k)) & 0x00FFFFFF), s[3]) for k, s in enumerate(specs)]


def batch(name):
    """(specs, the routes the fixtures are FOR, or None where the model decides) of a named batch."""
    if name == "mixed":
        return RM.mixed_specs(), list(RM.MIXED_ROUTES)
    if name == "random":
        return RM.random_specs(), None
    if name == "single":   # draws of one ring: every ring of the single-ring model, and its mixed batch without the MULTI draws
        names = list(TM.RINGS)
        mixed = [(s, r) for s, r in zip(TM.mixed_specs(), TM.MIXED_ROUTES) if r != TM.MULTI]
        return [TM.ring_spec(n) for n in names] + [s for s, _ in mixed], [TM.RINGS[n][2] for n in names] + [r for _, r in mixed]
    if name == "fixtures":
        names = list(RM.DRAWS)
    elif name == "imaged":
        names = [n for n in RM.DRAWS if n not in RM.NOT_IMAGED]
    else:
        names = [name]
    return recolour([RM.draw_spec(n) for n in names]), [RM.fixture(n)[3] for n in names]


_want = {}


def want(host, name):
    """(Flat, routes, pos, color, idx, meshes, notes) the model expects of a batch, on vgx_concave_contours' output for it."""
    if name not in _want:
        specs, meant = batch(name)
        fl = H.Flat(specs)
        notes = {}
        routes, pos, col, idx, meshes = RM.expected(specs, *TH.contours_of(host, fl), notes=notes)
        assert meant is None or routes.tolist() == meant, (name, routes.tolist(), meant)   # no fixture passes by falling back
        for a in (routes, pos, col, idx, meshes):
            a.setflags(write=False)
        _want[name] = (fl, routes, pos, col, idx, meshes, notes)
    return _want[name]


def host_triangulate(host, fl, out, with_routes=True):
    """-> status, sizes, routes, trips (per draw the most candidates one bridge search tried)."""
    sizes, status = capi.Sizes(), np.full(1, 77, dtype=np.uint32)
    n = len(fl.specs)
    routes = np.full(n + 2, 0xA5A5A5A5, dtype=np.uint32)
    trips = np.zeros(n + 1, dtype=np.uint32)
    rc = host.vgxt_concave_triangulate_rings(fl.poly.ctypes.data, fl.subs.ctypes.data, fl.info.ctypes.data, fl.draws.ctypes.data, n, C.byref(out.struct),
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


def frame_of(name, pos, col, idx, meshes):
    m = meshes.copy()
    m["draw"] = 0   # one colour draw without a scissor
    import raster_concave_model as K
    return K.finish(R.make(name, pos, col, idx, m, TARGET))


def check_images(run, specs, tri, contours, least):
    """Alpha-128 colours: the image of the triangulated frame equals the image of the contour frame in every byte."""
    fl = H.Flat(specs)
    assert all((s[2] >> 24) == 0x80 for s in specs)
    a = frame_of("triangulated", *tri(fl))
    b = frame_of("contours", *contours(fl))
    kinds = a.meshes["subpath_kind"] >> 28
    made = sum(1 for s in specs if TM.makes(s))
    assert int(((b.meshes["subpath_kind"] >> 28) == capi.MESH_CONTOURS).sum()) == made
    assert made - int((kinds == capi.MESH_CONTOURS).sum()) >= least   # that many draws hold triangles
    want_img = run.concave(b, TARGET)
    got = run.concave(a, TARGET)
    assert int((want_img != TARGET.background()).sum()) > 4000
    assert np.array_equal(got, want_img), H.where(got, want_img)


def check_exact_areas(fl, routes, pos, idx, meshes):
    """Exact rational arithmetic on the output alone: every triangle of a triangulated draw has the outer ring's orientation or area 0,
    and the areas sum to |outer| - sum |holes|."""
    seen = 0
    for m in meshes:
        d = int(m["draw"])
        if routes[d] != TM.TRIANGLES or (int(m["subpath_kind"]) >> 28) == capi.MESH_CONTOURS:
            continue
        lens = [len(q) for q in fl.specs[d][0]]
        V, Hn = sum(lens), len(lens) - 1
        aa = bool(fl.specs[d][1] & TM.AA)
        fv, fi = int(m["first_vertex"]) + (2 * V if aa else 0), int(m["first_index"]) + (6 * V if aa else 0)
        verts = pos[fv:fv + V]
        nt = 3 * (V + 2 * Hn - 2)
        assert int(m["num_indices"]) == (6 * V if aa else 0) + nt and int(m["num_vertices"]) == (3 * V if aa else V)
        t = idx[fi:fi + nt].astype(np.int64).reshape(-1, 3) - (2 * V if aa else 0)
        assert t.min() >= 0 and t.max() < V
        ring_areas = [TH.ring_area2(r) for r in np.split(verts, np.cumsum(lens)[:-1])]
        outer = max(ring_areas, key=abs)
        total = abs(outer) - (sum(abs(a) for a in ring_areas) - abs(outer))
        s = 1 if outer > 0 else -1
        areas = [TH.ring_area2(verts[list(tri)]) for tri in t]
        assert total > 0 and all(a * s >= 0 for a in areas), d
        assert sum(areas) * s == total, d
        seen += 1
    return seen
