"""CPU: the lane code of vgx_concave_triangulate (csrc/vgx_triangulate_lane.h through libvgx_hosttest.so: vgxt_concave_triangulate) on
flatten output built by hand, against the rule as tests/concave_triangulate_model.py states it: routes, sizes, mesh records and every
vertex, colour and index; the capacities with guard regions; refused draws byte for byte vgx_concave_contours'; the image of the
triangulated frame against the contour frame's; exact rational areas; and -- with oracle/_ref/libvgref.so -- libtess2's triangulation and
strokerConcaveFillEndAA's fringe. tests/test_gpu_concave_triangulate.py runs the same batches through the kernels."""
import numpy as np
import pytest

import concave_triangulate_harness as TH
import concave_triangulate_model as TM
import raster_concave_model as K
import raster_harness as H
import raster_model as R
import test_gpu_concave as TC

capi = R.capi
F = np.float32
OK = capi.VGX_OK


@pytest.fixture(scope="module")
def host():
    return TH.load_host()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


def lane(host):
    def tri(fl, caps):
        out = H.Out(*caps)
        st, sizes, routes = TH.host_triangulate(host, fl, out)
        return st, sizes, routes, out.streams(sizes[0], sizes[1], sizes[2]) if st == OK else None, out.guards_intact()
    return tri


def lane_streams(host, fl, triangulate=True):
    if not triangulate:
        return TH.contours_of(host, fl)
    probe = H.Out(0, 0, 0)
    st, (nm, nv, ni), _ = TH.host_triangulate(host, fl, probe)
    assert st == capi.VGX_E_NOSPACE
    out = H.Out(nv, ni, nm)
    assert TH.host_triangulate(host, fl, out)[0] == OK
    return out.streams(nm, nv, ni)


def test_fixtures_are_what_they_are_for(host):
    """Decided on the model alone: every fixture meant to be triangulated is, every refusal reason occurs, the spike is accepted as it
    stands and refused after its inset."""
    seen = set()
    for name in ("rings", "mixed"):
        _, routes = TH.want(host, name)[:2]
        seen |= set(routes.tolist())
    assert seen == {0, TM.TRIANGLES, TM.MULTI, TM.TOO_LONG, TM.NONFINITE, TM.DEGENERATE, TM.NOT_SIMPLE, TM.STALLED}
    assert TM.RINGS["spike"][2] == TM.TRIANGLES and TM.RINGS["spike_aa"][2] == TM.NOT_SIMPLE and TM.RINGS["spike"][0] is TM.RINGS["spike_aa"][0]
    assert len(TM.RINGS["cap"][0]) == TM.CAP and len(TM.RINGS["cap_plus_1"][0]) == TM.CAP + 1
    assert [len(TM.RINGS[n][0]) for n in ("tri3", "dart", "spiral", "ring65", "ring257")] == [3, 4, 80, 65, 257]
    # the rings that touch themselves cross nowhere: the first clause of the edge-pair test passes them, the zero-in-box clause alone
    # refuses them, as they stand (no AA: with it the inset crosses properly and the first clause would do)
    for n in TM.ZERO_CLAUSE_ONLY:
        ring, flags, meant = TM.RINGS[n]
        assert flags == 0 and meant == TM.NOT_SIMPLE and TM.orientation(ring) != 0 and TM.meets(ring) and not TM.meets(ring, proper_only=True), n
    assert TM.MIXED_ROUTES[16:18] == [TM.NOT_SIMPLE] * 2 and TM.RINGS["touch_aa"][1] == TM.AA
    # the spiral is what it is for: most candidates are no ears
    ring = TM.RINGS["spiral"][0]
    assert TM.meets(ring) is False and TM.orientation(ring) != 0


def test_stream_order_table_holds_the_entry():
    """The row comes from tests/stream_order_triangulate.py: it is there once, and it rests on a line of the header."""
    import stream_order as SO
    rows = [r for r in SO.CASES if r.entry == "vgx_concave_triangulate"]
    assert len(rows) == 1 and rows[0].cls == SO.ASYNC and "vgx_concave_triangulate" in SO.stream_entries()
    assert any(rows[0].header in line for line in SO.header_text().splitlines())


@pytest.mark.parametrize("name", ["rings", "mixed"])
def test_lane_code_equals_model(host, name):
    TH.check_against_model(host, name, lane(host))


def test_route_word_is_optional(host):
    fl = TH.want(host, "mixed")[0]
    nm, nv, ni = (len(TH.want(host, "mixed")[k]) for k in (5, 2, 4))
    a, b = H.Out(nv, ni, nm), H.Out(nv, ni, nm)
    assert TH.host_triangulate(host, fl, a)[0] == OK and TH.host_triangulate(host, fl, b, with_routes=False)[0] == OK
    assert all(np.array_equal(x, y) for x, y in zip(a.raw, b.raw))


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_gives_the_need_and_writes_nothing(host, short):
    fl, routes, pos, _, idx, meshes = TH.want(host, "mixed")
    nv, ni, nm = len(pos), len(idx), len(meshes)
    out = H.Out(nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    st, sizes, got = TH.host_triangulate(host, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni) and got.tolist() == routes.tolist()
    assert out.guards_intact() and out.untouched()


def test_refused_draws_hold_the_contour_route_bytes(host):
    """Not through the model: the lane code's two outputs for the same batch, draw by draw."""
    fl, routes = TH.want(host, "mixed")[:2]
    tp, tc, ti, tm = lane_streams(host, fl)
    cp, cc, ci, cm = lane_streams(host, fl, triangulate=False)
    refused = [d for d in range(len(routes)) if routes[d] > TM.TRIANGLES]
    assert len(refused) >= 6
    for d in refused:
        a, b = tm[tm["draw"] == d], cm[cm["draw"] == d]
        assert len(a) == len(b) == (2 if fl.specs[d][1] & TM.AA else 1)
        for x, y in zip(a, b):
            assert (int(x["num_vertices"]), int(x["num_indices"]), int(x["subpath_kind"])) == (int(y["num_vertices"]), int(y["num_indices"]), int(y["subpath_kind"]))
            n, q = int(x["num_vertices"]), int(x["num_indices"])
            xa, ya, xb, yb = int(x["first_vertex"]), int(y["first_vertex"]), int(x["first_index"]), int(y["first_index"])
            assert np.array_equal(tp[xa:xa + n].view(np.uint32), cp[ya:ya + n].view(np.uint32)) and np.array_equal(tc[xa:xa + n], cc[ya:ya + n])
            assert np.array_equal(ti[xb:xb + q], ci[yb:yb + q])


def test_subpaths_that_do_not_lie_back_to_back_are_refused(host):
    specs, _ = TH.batch("mixed")
    fl = H.Flat(specs)
    fl.subs["first_vertex"][4] += 1   # the second sub-path of draw 3
    out = H.Out(4000, 12000, 40)
    st, _, _ = TH.host_triangulate(host, fl, out)
    assert st == capi.VGX_E_INVALID_ARG and out.untouched()


def test_image_of_the_triangles_equals_image_of_the_contours(host):
    TH.check_images(host, H.HostRunner(host), lambda fl: lane_streams(host, fl), lambda fl: lane_streams(host, fl, triangulate=False))


def test_triangles_tile_the_ring_in_exact_arithmetic(host):
    seen = 0
    for name in ("imaged", "mixed"):
        fl, routes = TH.want(host, name)[:2]
        pos, _, idx, meshes = lane_streams(host, fl)
        seen += TH.check_exact_areas(fl, routes, pos, idx, meshes)
    assert seen >= 25


def test_image_equals_libtess2_and_fringe_equals_the_reference(host, ref):
    """Simple polygons on an integer grid. Without AA: the triangles' image is the image of libtess2's TESS_POLYGONS triangulation. With AA,
    on libtess2's boundary contours: the first 2V vertices and 6V indices are strokerConcaveFillEndAA's bit for bit, and the whole mesh
    draws the image of the reference's mesh."""
    run = H.HostRunner(host)
    tgt = R.Target(42, 38, 43, -1, -1)
    for name in ("L", "comb"):
        contours = [np.array(c, dtype=F) for c in H.SIMPLE[name]]
        tf, _ = H.tess_frame(ref, name, contours, tgt, TM.COLOR, False)
        fl = H.Flat([(contours, TM.CONCAVE, TM.COLOR, 1.0)])
        pos, col, idx, meshes = lane_streams(host, fl)
        assert int(meshes[0]["subpath_kind"]) == TM.FILL_KIND
        m = meshes.copy()
        got = run.painted(K.finish(R.make(name, pos, col, idx, m, tgt)), tgt)
        want = run.painted(tf, tgt)
        assert int((want != tgt.background()).sum()) > 300 and np.array_equal(got, want), (name, H.where(got, want))
        b = H.boundary_of(ref, contours, 0)
        assert len(b) == 1 and len(b[0]) == len(contours[0])
        fl = H.Flat([(b, TM.CONCAVE | TM.AA, TM.COLOR, 1.0)])
        pos, col, idx, meshes = lane_streams(host, fl)
        V = len(b[0])
        assert len(meshes) == 1 and (int(meshes[0]["num_vertices"]), int(meshes[0]["num_indices"])) == (3 * V, 6 * V + 3 * (V - 2))
        rpos, rcol, ridx = TC._reference_mesh(ref, contours, TM.COLOR, 1.0, 0)
        assert np.array_equal(pos[:2 * V].view(np.uint32), rpos[:2 * V].view(np.uint32)) and np.array_equal(col[:2 * V], rcol[:2 * V])
        assert np.array_equal(idx[:6 * V], ridx[:6 * V])
        assert np.array_equal(pos[2 * V:].view(np.uint32), pos[0:2 * V:2].view(np.uint32))   # the interior: the moved vertices
        bld = K.Builder()
        bld.mesh([tuple(p) for p in rpos], [int(c) for c in rcol], [int(i) for i in ridx], kind=capi.MESH_CONCAVE_FILL_AA)
        want = run.painted(K.finish(bld.frame("reference", tgt)), tgt)
        got = run.painted(K.finish(R.make(name + "_aa", pos, col, idx, meshes.copy(), tgt)), tgt)
        assert np.array_equal(got, want), (name, H.where(got, want))
