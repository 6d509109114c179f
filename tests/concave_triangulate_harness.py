"""What the two sides of vgx_concave_triangulate's tests share (tests/test_concave_triangulate_cpu.py: the lane code;
tests/test_gpu_concave_triangulate.py: the kernels): the host entry's prototype, the batches built from the fixtures of
tests/concave_triangulate_model.py, what the model expects of them (computed once, never changed), frames for the image checks, and the
checks both sides run through a `tri` callable (specs' Flat, Out-like capacities) -> (status, sizes, routes, streams)."""
import ctypes as C
from fractions import Fraction

import numpy as np

import concave_triangulate_model as TM
import raster_concave_model as K
import raster_harness as H
import raster_model as R
import stream_order_triangulate  # noqa: F401 (puts the entry's row into the table of tests/stream_order.py)

capi = R.capi
F = np.float32
OK = capi.VGX_OK
TARGET = R.Target(92, 90, 93, 0, 0)
NOT_IMAGED = ("nan", "stalled", "cap_plus_1")   # a NaN's box is unspecified; the other two are route fixtures far outside any image


def load_host():
    """H.load_host() with this entry's prototype. Its loader rebuilds for the symbols of its own table only: a library from before
    this entry is rebuilt here, once."""
    lib = H.load_host()
    if not hasattr(lib, "vgxt_concave_triangulate"):
        import __graft_entry__ as g
        g.build()
        lib = H.load_host()
    assert hasattr(lib, "vgxt_concave_triangulate"), "libvgx_hosttest.so lacks vgxt_concave_triangulate after a build"
    lib.vgxt_concave_triangulate.restype = C.c_int
    lib.vgxt_concave_triangulate.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(capi.MeshOut), C.c_void_p, C.POINTER(capi.Sizes), C.c_void_p]
    return lib


def batch(name):
    """(specs, the routes the fixtures are FOR) of a named batch."""
    if name == "mixed":
        return TM.mixed_specs(), list(TM.MIXED_ROUTES)
    if name == "rings":
        names = list(TM.RINGS)
    elif name == "imaged":
        names = [n for n in TM.RINGS if n not in NOT_IMAGED]
    else:
        names = [name]
    return [TM.ring_spec(n, color=TM.COLOR ^ (0x00010307 * k & 0x00FFFFFF)) for k, n in enumerate(names)], [TM.RINGS[n][2] for n in names]


_want = {}


def contours_of(host, fl):
    nm, nv, ni = fl.expected_sizes()
    out = H.Out(nv, ni, nm)
    st, sizes = H.host_contours(host, fl, out)
    assert st == OK and sizes == (nm, nv, ni)
    return out.streams(nm, nv, ni)


def want(host, name):
    """(Flat, routes, pos, color, idx, meshes) the model expects of a batch, on vgx_concave_contours' output for it."""
    if name not in _want:
        specs, meant = batch(name)
        fl = H.Flat(specs)
        routes, pos, col, idx, meshes = TM.expected(specs, *contours_of(host, fl))
        assert routes.tolist() == meant, (name, routes.tolist(), meant)   # no fixture passes by falling back
        for a in (routes, pos, col, idx, meshes):
            a.setflags(write=False)
        _want[name] = (fl, routes, pos, col, idx, meshes)
    return _want[name]


def host_triangulate(host, fl, out, with_routes=True):
    sizes, status = capi.Sizes(), np.full(1, 77, dtype=np.uint32)
    routes = np.full(len(fl.specs) + 2, 0xA5A5A5A5, dtype=np.uint32)
    rc = host.vgxt_concave_triangulate(fl.poly.ctypes.data, fl.subs.ctypes.data, fl.info.ctypes.data, fl.draws.ctypes.data, len(fl.specs), C.byref(out.struct),
                                       routes.ctypes.data if with_routes else None, C.byref(sizes), status.ctypes.data)
    assert rc == OK and (routes[len(fl.specs):] == 0xA5A5A5A5).all()
    return int(status[0]), (int(sizes.num_meshes), int(sizes.num_vertices), int(sizes.num_indices)), routes[:len(fl.specs)]


def check_against_model(host, name, tri):
    """tri(fl, caps) -> (status, sizes, routes, (pos, color, idx, meshes), guards intact): everything equals the model's word."""
    fl, routes, pos, col, idx, meshes = want(host, name)
    caps = (len(pos), len(idx), len(meshes))
    st, sizes, got_routes, streams, intact = tri(fl, caps)
    assert st == OK and sizes == (caps[2], caps[0], caps[1]) and intact
    assert got_routes.tolist() == routes.tolist()
    gpos, gcol, gidx, gmeshes = streams
    assert gmeshes.tobytes() == meshes.tobytes(), [(tuple(a), tuple(b)) for a, b in zip(gmeshes, meshes) if a != b][:3]
    assert np.array_equal(gpos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(gcol, col) and np.array_equal(gidx, idx)


def frame_of(name, pos, col, idx, meshes):
    m = meshes.copy()
    m["draw"] = 0   # one colour draw without a scissor
    return K.finish(R.make(name, pos, col, idx, m, TARGET))


def check_images(host, run, tri, contours):
    """Alpha-128 colours: the image of the triangulated frame equals the image of the contour frame in every byte. tri / contours:
    (fl) -> (pos, color, idx, meshes) of the side under test."""
    specs, meant = batch("imaged")
    fl = H.Flat(specs)
    assert all((s[2] >> 24) == 0x80 for s in specs) and meant.count(TM.TRIANGLES) >= 20
    a = frame_of("triangulated", *tri(fl))
    b = frame_of("contours", *contours(fl))
    kinds = a.meshes["subpath_kind"] >> 28
    assert int((kinds == capi.MESH_CONCAVE_FILL_AA).sum()) >= 20 and int(((b.meshes["subpath_kind"] >> 28) == capi.MESH_CONTOURS).sum()) == len(specs)
    want_img = run.concave(b, TARGET)
    got = run.concave(a, TARGET)
    assert int((want_img != TARGET.background()).sum()) > 4000
    assert np.array_equal(got, want_img), H.where(got, want_img)
    # the triangles are triangles to everyone: the level below, which skips contour meshes, draws them too
    tri_only = a.meshes.copy()
    keep = kinds == capi.MESH_CONCAVE_FILL_AA
    both = frame_of("kept", a.pos, a.color, a.idx, tri_only[keep])
    assert np.array_equal(run.painted(both, TARGET), run.concave(both, TARGET))


def ring_area2(ring):
    V = len(ring)
    return sum(Fraction(float(ring[i][0])) * Fraction(float(ring[(i + 1) % V][1])) - Fraction(float(ring[(i + 1) % V][0])) * Fraction(float(ring[i][1])) for i in range(V))


def check_exact_areas(fl, routes, pos, idx, meshes):
    """Exact rational arithmetic on the output alone: the triangles of a triangulated draw tile its ring."""
    seen = 0
    for m in meshes:
        d = int(m["draw"])
        if routes[d] != TM.TRIANGLES:
            continue
        V = sum(len(q) for q in fl.specs[d][0])
        aa = bool(fl.specs[d][1] & TM.AA)
        fv, fi = int(m["first_vertex"]) + (2 * V if aa else 0), int(m["first_index"]) + (6 * V if aa else 0)
        ring = pos[fv:fv + V]
        t = idx[fi:fi + 3 * (V - 2)].astype(np.int64).reshape(-1, 3) - (2 * V if aa else 0)
        assert int(m["num_indices"]) == (6 * V if aa else 0) + 3 * (V - 2) and t.min() >= 0 and t.max() < V
        total = ring_area2(ring)
        s = 1 if total > 0 else -1
        areas = [ring_area2(ring[list(tri)]) for tri in t]
        assert total != 0 and all(a * s >= 0 for a in areas), d          # the ring's orientation, or area 0
        assert sum(areas) == total, d                                       # ... so sum |area| = |area of the ring|
        seen += 1
    return seen
