"""CPU: the lane code of vgx_concave_contours (csrc/vgx_concave_lane.h through libvgx_hosttest.so: vgxt_concave_contours) on flatten
output built by hand: which draws make meshes, the records, the rings, the capacities with guard regions, VGX_E_MESH_TOO_LARGE, and --
with the reference's own strokerConcaveFillEndAA from oracle/_ref/libvgref.so -- the fringe bit for bit and the image of the AA pair.
tests/test_gpu_concave_contours.py runs the same inputs through the kernel and compares the fringe and the moved vertices with
vgx_concave_emit and vgx_concave_move on the device."""
import numpy as np
import pytest

import raster_harness as H
import raster_model as R
import test_gpu_concave as TC
from raster_harness import AA, CONCAVE, EO, Flat, Out, check_structure, host, host_contours  # noqa: F401 (host: fixture)

capi = R.capi
F = np.float32
specs = H.contour_specs


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


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


SIMPLE_AA = [([TC._star(100, 100, 80, 30, 5)], 0xFF3366CC, 1.0, 0), ([TC._ring(300, 120, 90, 24), TC._ring(300, 120, 40, 16, cw=True)], 0x80FF8040, 1.0, 0),
             ([TC._ring(600, 200, 70, 40, wobble=0.35, seed=3)], 0xFFABCDEF, 2.0, 1), ([TC._ring(700, 500, 60, 9, cw=True)], 0xFF123456, 0.5, 0)]


def test_fringe_equals_the_reference_bit_for_bit(host, ref):
    """strokerConcaveFillEndAA runs its fringe loop over libtess2's boundary contours; fed those contours as sub-paths the producer's
    fringe mesh is the first 2V vertices and 6V indices of the reference's mesh, bit for bit (the in-place quirk of the last vertex
    included)."""
    for contours, color, fringe, eo in SIMPLE_AA:
        b = H.boundary_of(ref, contours, eo)
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


def test_aa_pair_image_equals_the_reference_mesh(host, ref):
    H.check_aa_pair_image(H.HostRunner(host), host, ref)
