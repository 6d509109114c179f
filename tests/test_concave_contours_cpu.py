"""CPU: the lane code of vgx_concave_contours (csrc/vgx_concave_lane.h through libvgx_hosttest.so: vgxt_concave_contours) on flatten
output built by hand: which draws make meshes, the records, the rings, the capacities with guard regions, VGX_E_MESH_TOO_LARGE, and --
with the reference's own strokerConcaveFillEndAA from oracle/_ref/libvgref.so -- the fringe bit for bit and the image of the AA pair.
tests/test_gpu_concave_contours.py runs the same inputs through the kernel and compares the fringe and the moved vertices with
vgx_concave_emit and vgx_concave_move on the device."""
import ctypes as C

import numpy as np
import pytest

import raster_concave_model as K
import raster_model as R
import test_gpu_concave as TC
import test_raster_concave_cpu as rcpu

capi = R.capi
F = np.float32
CONCAVE, AA, EO, ENABLE = capi.FILL_CONCAVE, 0x2, capi.FILL_EVEN_ODD, 0x1
GUARD = 0xA5


class Flat:
    """What vgx_flatten leaves for a list of draws: (contours, fill_flags, colour, fringe) each; contours = [n, 2] arrays, back to back."""

    def __init__(self, specs):
        polys, subs, infos = [], [], []
        self.draws = np.zeros(len(specs), dtype=capi.draw_dtype)
        nv = 0
        for d, (contours, flags, color, fringe) in enumerate(specs):
            infos.append((nv, len(subs), 0, sum(len(c) for c in contours), len(contours), 0, 0))
            for c in contours:
                c = np.asarray(c, dtype=F).reshape(-1, 2)
                subs.append((nv, len(c), 1))
                polys.append(c)
                nv += len(c)
            self.draws[d]["fill_flags"], self.draws[d]["fill_color"], self.draws[d]["fringe"] = flags, color, fringe
            self.draws[d]["scale"], self.draws[d]["tess_tol"] = 1.0, 0.25
        self.poly = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((1, 2), F), dtype=F)
        self.subs = np.array(subs if subs else [(0, 0, 0)], dtype=capi.subpath_dtype)
        self.info = np.array(infos, dtype=capi.draw_info_dtype)
        self.specs = specs

    def makes(self, d):
        contours, flags = self.specs[d][0], self.specs[d][1]
        return bool(flags & CONCAVE) and not (flags & ENABLE) and len(contours) > 0 and all(len(c) >= 3 for c in contours)

    def expected_sizes(self):
        nm = nv = ni = 0
        for d, (contours, flags, _, _) in enumerate(self.specs):
            if self.makes(d):
                V = sum(len(c) for c in contours)
                nm, nv, ni = nm + (2 if flags & AA else 1), nv + (3 * V if flags & AA else V), ni + (8 * V if flags & AA else 2 * V)
        return nm, nv, ni


def load_host():
    lib = rcpu.load_host()
    lib.vgxt_concave_contours.restype = C.c_int
    lib.vgxt_concave_contours.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.MeshOut), C.POINTER(capi.Sizes), C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


class Out:
    """Output streams of given capacities between guard regions of 64 elements."""

    def __init__(self, cap_v, cap_i, cap_m, pad=64):
        self.caps, self.pad = (cap_v, cap_i, cap_m), pad
        self.pos = np.full(((cap_v + 2 * pad), 2), np.nan, dtype=F)
        self.raw = [self.pos.view(np.uint8), np.zeros(4 * (cap_v + 2 * pad), np.uint8), np.zeros(2 * (cap_i + 2 * pad), np.uint8), np.zeros(32 * (cap_m + 2 * pad), np.uint8)]
        for r in self.raw:
            r[...] = GUARD
        self.color, self.idx, self.meshes = self.raw[1].view(np.uint32), self.raw[2].view(np.uint16), self.raw[3].view(capi.mesh_dtype)
        self.struct = capi.MeshOut(self.pos[pad:].ctypes.data, self.color[pad:].ctypes.data, self.idx[pad:].ctypes.data, self.meshes[pad:].ctypes.data, cap_v, cap_i, cap_m)

    def guards_intact(self):
        p = self.pad
        return all((r.reshape(n + 2 * p, -1)[:p] == GUARD).all() and (r.reshape(n + 2 * p, -1)[p + n:] == GUARD).all()
                   for r, n in zip(self.raw, (self.caps[0], self.caps[0], self.caps[1], self.caps[2])))

    def untouched(self):
        return all((r == GUARD).all() for r in self.raw[:3])

    def streams(self, nm, nv, ni):
        p = self.pad
        return self.pos[p:p + nv].copy(), self.color[p:p + nv].copy(), self.idx[p:p + ni].copy(), self.meshes[p:p + nm].copy()


def host_contours(host, fl, out):
    sizes, status = capi.Sizes(), np.full(1, 77, dtype=np.uint32)
    rc = host.vgxt_concave_contours(fl.poly.ctypes.data, fl.subs.ctypes.data, fl.info.ctypes.data, fl.draws.ctypes.data, len(fl.specs), C.byref(out.struct),
                                    C.byref(sizes), status.ctypes.data)
    assert rc == capi.VGX_OK
    return int(status[0]), (int(sizes.num_meshes), int(sizes.num_vertices), int(sizes.num_indices))


def specs():
    """Concave draws of both rules, AA and not, with one and several sub-paths, between draws that make nothing."""
    sq = np.array([[0, 0], [40, 0], [40, 40], [0, 40]], dtype=F)
    return [
        ([TC._star(100, 100, 80, 30, 5)], CONCAVE, 0xFF3366CC, 1.0),                                         # 0 one mesh, NonZero
        ([sq], ENABLE | AA, 0xFF112233, 1.0),                                                                  # 1 a convex fill: nothing
        ([TC._ring(300, 120, 90, 24), TC._ring(300, 120, 40, 16, cw=True)], CONCAVE | AA, 0x80FF8040, 1.5),   # 2 two meshes, two rings
        ([], CONCAVE | AA, 0xFFFFFFFF, 1.0),                                                                   # 3 no sub-path: nothing
        ([TC._ring(60, 300, 50, 12), sq[:2]], CONCAVE, 0xFF00AA55, 1.0),                                      # 4 a sub-path of 2 vertices: nothing at all
        ([TC._ring(60, 300, 50, 12), TC._ring(110, 300, 50, 7)], CONCAVE | EO, 0xFF00AA55, 1.0),              # 5 one mesh, EvenOdd
        ([sq + 7], CONCAVE | ENABLE, 0xFF445566, 1.0),                                                         # 6 VGX_FILL_ENABLE set: nothing
        ([TC._ring(600, 200, 70, 40, wobble=0.35, seed=3)], CONCAVE | AA | EO, 0xC0ABCDEF, 0.75),             # 7 two meshes, EvenOdd
    ]


def check_structure(fl, pos, color, idx, meshes):
    """Everything about the output that follows from the header without fringe arithmetic."""
    k = 0
    for d, (contours, flags, col, _) in enumerate(fl.specs):
        if not fl.makes(d):
            continue
        V = sum(len(c) for c in contours)
        allv = np.concatenate([np.asarray(c, dtype=F) for c in contours])
        rings = np.array(K.ring_indices([len(c) for c in contours]), dtype=np.uint16)
        if flags & AA:
            m = meshes[k]
            assert (int(m["num_vertices"]), int(m["num_indices"]), int(m["draw"]), int(m["subpath_kind"])) == (2 * V, 6 * V, d, capi.MESH_CONCAVE_FILL_AA << 28)
            fv = int(m["first_vertex"])
            assert (color[fv:fv + 2 * V:2] == col).all() and (color[fv + 1:fv + 2 * V:2] == (col & 0x00FFFFFF)).all()
            k += 1
        m = meshes[k]
        rule = capi.CONTOUR_EVEN_ODD if flags & EO else 0
        assert (int(m["num_vertices"]), int(m["num_indices"]), int(m["draw"]), int(m["subpath_kind"])) == (V, 2 * V, d, (capi.MESH_CONTOURS << 28) | rule)
        fv, fi = int(m["first_vertex"]), int(m["first_index"])
        if k and int(meshes[k - 1]["draw"]) == d:
            p = meshes[k - 1]
            assert fv == int(p["first_vertex"]) + 2 * V and fi == int(p["first_index"]) + 6 * V
            assert np.array_equal(pos[fv:fv + V].view(np.uint32), pos[int(p["first_vertex"]):fv:2].view(np.uint32))  # the moved vertex IS the inner fringe vertex
        else:
            assert np.array_equal(pos[fv:fv + V].view(np.uint32), allv.view(np.uint32))
        assert (color[fv:fv + V] == col).all() and np.array_equal(idx[fi:fi + 2 * V], rings)
        k += 1
    assert k == meshes.shape[0]
    ends = meshes["first_vertex"] + meshes["num_vertices"]
    assert (meshes["first_vertex"][1:] == ends[:-1]).all() and (np.diff(meshes["draw"].astype(np.int64)) >= 0).all()   # dense, ascending by draw


def test_which_draws_make_meshes_and_what_they_hold(host):
    fl = Flat(specs())
    nm, nv, ni = fl.expected_sizes()
    assert nm == 6 and [fl.makes(d) for d in range(8)] == [True, False, True, False, False, True, False, True]
    out = Out(nv, ni, nm)
    st, sizes = host_contours(host, fl, out)
    assert st == capi.VGX_OK and sizes == (nm, nv, ni) and out.guards_intact()
    check_structure(fl, *out.streams(nm, nv, ni))


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_writes_nothing_past_a_capacity(host, short):
    fl = Flat(specs())
    nm, nv, ni = fl.expected_sizes()
    out = Out(nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    st, sizes = host_contours(host, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni)  # the need
    assert out.guards_intact() and out.untouched()


def test_mesh_too_large_at_32769_contour_vertices_with_aa(host):
    for n, flags, want in ((32768, CONCAVE | AA, capi.VGX_OK), (32769, CONCAVE | AA, capi.VGX_E_MESH_TOO_LARGE), (65536, CONCAVE, capi.VGX_OK),
                           (65537, CONCAVE, capi.VGX_E_MESH_TOO_LARGE)):
        fl = Flat([([TC._ring(0, 0, 1000, n)], flags, 0xFFFFFFFF, 1.0)])
        nm, nv, ni = fl.expected_sizes()
        out = Out(nv, ni, nm)
        st, _ = host_contours(host, fl, out)
        assert st == want and out.guards_intact() and (want == capi.VGX_OK or out.untouched()), n


def test_subpaths_that_do_not_lie_back_to_back_are_refused(host):
    fl = Flat(specs())
    fl.subs["first_vertex"][2] += 1
    out = Out(*fl.expected_sizes()[1:], fl.expected_sizes()[0])
    st, _ = host_contours(host, fl, out)
    assert st == capi.VGX_E_INVALID_ARG and out.untouched()


def boundary_of(ref, contours, even_odd):
    """libtess2's boundary contours of a SIMPLE path: the input contours again, from whichever vertex libtess2 starts them."""
    t, verts, el = TC._tess_boundary(ref, contours, even_odd)
    ref.vgo_tess_delete(t)
    return [verts[int(a):int(a) + int(n)].copy() for a, n in el]


SIMPLE_AA = [([TC._star(100, 100, 80, 30, 5)], 0xFF3366CC, 1.0, 0), ([TC._ring(300, 120, 90, 24), TC._ring(300, 120, 40, 16, cw=True)], 0x80FF8040, 1.0, 0),
             ([TC._ring(600, 200, 70, 40, wobble=0.35, seed=3)], 0xFFABCDEF, 2.0, 1), ([TC._ring(700, 500, 60, 9, cw=True)], 0xFF123456, 0.5, 0)]


def test_fringe_equals_the_reference_bit_for_bit(host, ref):
    """strokerConcaveFillEndAA runs its fringe loop over libtess2's boundary contours; fed those contours as sub-paths the producer's
    fringe mesh is the first 2V vertices and 6V indices of the reference's mesh, bit for bit (the in-place quirk of the last vertex
    included)."""
    for contours, color, fringe, eo in SIMPLE_AA:
        b = boundary_of(ref, contours, eo)
        assert sorted(len(c) for c in b) == sorted(len(c) for c in contours)   # a simple path: nothing merged, nothing split
        fl = Flat([(b, CONCAVE | AA | (EO if eo else 0), color, fringe)])
        nm, nv, ni = fl.expected_sizes()
        out = Out(nv, ni, nm)
        st, _ = host_contours(host, fl, out)
        assert st == capi.VGX_OK
        pos, col, idx, meshes = out.streams(nm, nv, ni)
        check_structure(fl, pos, col, idx, meshes)
        rpos, rcol, ridx = TC._reference_mesh(ref, contours, color, fringe, eo)
        V = nv // 3
        assert np.array_equal(pos[:2 * V].view(np.uint32), rpos[:2 * V].view(np.uint32)) and np.array_equal(col[:2 * V], rcol[:2 * V])
        assert np.array_equal(idx[:6 * V], ridx[:6 * V])


def pair_frames(host, ref, contours, color, fringe, eo, tgt):
    """(the producer's AA pair as a frame, the reference's single mesh as a frame) for an integer-grid path."""
    b = boundary_of(ref, [np.asarray(c, dtype=F) for c in contours], eo)
    fl = Flat([(b, CONCAVE | AA | (EO if eo else 0), color, fringe)])
    nm, nv, ni = fl.expected_sizes()
    out = Out(nv, ni, nm)
    assert host_contours(host, fl, out)[0] == capi.VGX_OK
    pos, col, idx, meshes = out.streams(nm, nv, ni)
    meshes["draw"] = 0
    pair = K.finish(R.make("pair", pos, col, idx, meshes, tgt))
    rpos, rcol, ridx = TC._reference_mesh(ref, [np.asarray(c, dtype=F) for c in contours], color, fringe, eo)
    bld = K.Builder()
    bld.mesh([tuple(p) for p in rpos], [int(c) for c in rcol], [int(i) for i in ridx], kind=capi.MESH_CONCAVE_FILL_AA)
    return pair, K.finish(bld.frame("reference", tgt))


def check_aa_pair_image(run, host, ref):
    """Simple concave polygons on an integer grid, alpha 128: the AA pair through the new level equals the reference's single mesh
    (libtess2 supplying the interior of the moved contours) through vgx_raster_painted, at every pixel."""
    tgt = R.Target(42, 38, 43, -1, -1)
    for name, contours in rcpu.SIMPLE.items():
        pair, single = pair_frames(host, ref, contours, 0x8040C0F0, 1.0, 0, tgt)
        want = run.painted(single, tgt)
        got = run.concave(pair, tgt)
        assert int((want != tgt.background()).sum()) > 300
        assert np.array_equal(got, want), (name, rcpu.base.where(got, want))


def test_aa_pair_image_equals_the_reference_mesh(host, ref):
    check_aa_pair_image(rcpu.HostRunner(host), host, ref)
