"""CPU: the lane code of vgx_concave_triangulate_rings (csrc/vgx_triangulate_lane.h through libvgx_hosttest.so:
vgxt_concave_triangulate_rings) on flatten output built by hand, against the rule as tests/concave_rings_model.py states it: routes,
sizes, mesh records and every vertex, colour and index, between guard regions. Not resting on the model: exact rational areas, the image
of the triangulated frame against the contour frame's, single-ring draws against vgxt_concave_triangulate, and -- with
oracle/_ref/libvgref.so -- libtess2's triangulation and strokerConcaveFillEndAA's fringe. tests/test_gpu_concave_rings.py runs the same
batches through the kernels."""
import numpy as np
import pytest

import concave_rings_harness as RH
import concave_rings_model as RM
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
    return RH.load_host()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


def lane(host):
    def tri(fl, caps):
        out = H.Out(*caps)
        st, sizes, routes, _ = RH.host_triangulate(host, fl, out)
        return st, sizes, routes, out.streams(sizes[0], sizes[1], sizes[2]) if st == OK else None, out.guards_intact()
    return tri


def lane_streams(host, fl, triangulate=True):
    if not triangulate:
        return TH.contours_of(host, fl)
    probe = H.Out(0, 0, 0)
    st, (nm, nv, ni), _, _ = RH.host_triangulate(host, fl, probe)
    assert st == capi.VGX_E_NOSPACE
    out = H.Out(nv, ni, nm)
    assert RH.host_triangulate(host, fl, out)[0] == OK
    return out.streams(nm, nv, ni)


def test_fixtures_are_what_they_are_for(host):
    """Decided on the model: every listed route; the two trips of OCCLUDED; the slot SHARED's second bridge ends on; the spike."""
    routes = RH.want(host, "fixtures")[1].tolist()
    assert set(routes) == {RM.TRIANGLES, RM.NONFINITE, RM.DEGENERATE, RM.NOT_SIMPLE, RM.NESTING}
    for name in ("donut", "donut_hole_first", "donut_same_eo", "b", "row", "occluded", "shared", "comb"):
        assert RM.DRAWS[name][3] == RM.TRIANGLES
    assert [RM.DRAWS[n][3] for n in ("donut_same_nz", "island", "separate", "touching")] == [RM.NESTING, RM.NESTING, RM.NESTING, RM.NOT_SIMPLE]
    assert all(np.array_equal(r * 4, np.round(r * 4)) for n in RM.DRAWS if n != "nan_hole" for r in RM.DRAWS[n][0])   # multiples of 0.25
    # OCCLUDED: the nearest candidate in the cone of the last hole, (14.5, 10), is hidden behind the sliver; the second is taken
    _, _, notes = RM.rings_route(RM.OCCLUDED, False)
    assert notes["trips"] == [1, 2] and notes["bridges"][1][0] == 12 and tuple(RM.OCCLUDED[0][3]) == (14.5, 10.0) and notes["bridges"][1][1] != 3
    # SHARED: the second hole's bridge ends on the SECOND slot (V = 11, slot V + 0) of the first hole's bridge vertex; with every ring
    # reversed under even-odd on its first slot, the vertex itself
    _, _, notes = RM.rings_route(RM.SHARED, False)
    assert notes["bridges"] == [(5, 1), (8, 11)]
    _, _, notes = RM.rings_route([RM.rev(r) for r in RM.SHARED], True)
    assert notes["bridges"][0][0] == 7 and notes["bridges"][1] == (10, 7)
    # the comb: a search that needs more than one trip
    assert max(RM.rings_route(RM.COMB, False)[2]["trips"]) > 1
    # the hole next to the rim: apart as it stands, crossing after the inset
    assert RM.DRAWS["spike_hole"][3] == RM.TRIANGLES and RM.DRAWS["spike_hole_aa"][3] == RM.NOT_SIMPLE and RM.DRAWS["spike_hole"][0] is RM.DRAWS["spike_hole_aa"][0]


def test_random_sets_bridge_and_never_stall(host):
    """Every random set that passes NOT_SIMPLE and NESTING is triangulated: no STALLED and no NO_BRIDGE, under both rules."""
    routes = RH.want(host, "random")[1].tolist()
    assert len(routes) == 2 * len(RM.RANDOM_SEEDS) == 20
    assert set(routes) <= {RM.TRIANGLES, RM.NOT_SIMPLE, RM.NESTING} and routes.count(RM.TRIANGLES) >= 10, routes


def test_stream_order_table_holds_the_entry():
    import stream_order as SO
    rows = [r for r in SO.CASES if r.entry == "vgx_concave_triangulate_rings"]
    assert len(rows) == 1 and rows[0].cls == SO.ASYNC and "vgx_concave_triangulate_rings" in SO.stream_entries()
    assert any(rows[0].header in line for line in SO.header_text().splitlines())


@pytest.mark.parametrize("name", ["fixtures", "mixed", "random", "grid", "cap", "cap_plus_1"])
def test_lane_code_equals_model(host, name):
    RH.check_against_model(host, name, lane(host))


def test_search_trips_equal_the_model(host):
    fl, routes, _, _, _, _, notes = RH.want(host, "fixtures")
    _, _, got, trips = RH.host_triangulate(host, fl, H.Out(0, 0, 0))
    assert got.tolist() == routes.tolist()   # routes are written whatever the status
    for d in range(len(fl.specs)):
        assert int(trips[d]) == max(notes[d].get("trips", []) or [0]), d
    assert int(trips.max()) >= 2


def test_large_fixtures_have_the_listed_sizes():
    grid = RM.fixture("grid")[0]
    assert len(grid) == 145 and sum(len(r) for r in grid) == 1012 and all(len(r) == 7 for r in grid[1:])
    for extra, meant in ((0, RM.TRIANGLES), (1, RM.TOO_LONG)):
        rings = RM.cap_rings(extra)
        assert sum(len(r) for r in rings) + 2 * (len(rings) - 1) == RM.CAP + extra


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_gives_the_need_and_writes_nothing(host, short):
    fl, routes, pos, _, idx, meshes, _ = RH.want(host, "mixed")
    nv, ni, nm = len(pos), len(idx), len(meshes)
    out = H.Out(nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    st, sizes, got, _ = RH.host_triangulate(host, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni) and got.tolist() == routes.tolist()
    assert out.guards_intact() and out.untouched()


def test_single_ring_draws_get_the_single_ring_entry_s_words(host):
    """(c) Not through the model: the two host entries on the same draws of one ring each, every byte with the guard regions."""
    specs, meant = RH.batch("single")
    fl = H.Flat(specs)
    probe = H.Out(0, 0, 0)
    _, (nm, nv, ni), _ = TH.host_triangulate(host, fl, probe)
    a, b = H.Out(nv, ni, nm), H.Out(nv, ni, nm)
    sa, za, ra = TH.host_triangulate(host, fl, a)
    sb, zb, rb, _ = RH.host_triangulate(host, fl, b)
    assert sa == sb == OK and za == zb and ra.tolist() == rb.tolist() == meant
    assert all(np.array_equal(x, y) for x, y in zip(a.raw, b.raw))


def test_refused_draws_hold_the_contour_route_bytes(host):
    fl, routes = RH.want(host, "mixed")[:2]
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


@pytest.mark.parametrize("name", ["imaged", "random"])
def test_image_of_the_triangles_equals_image_of_the_contours(host, name):
    """(b) Both fill rules, with and without AA, in one frame at alpha 128."""
    specs, _ = RH.batch(name)
    if name == "imaged":
        flags = [s[1] & (TM.AA | TM.EO) for s, r in zip(specs, RH.want(host, "imaged")[1]) if r == TM.TRIANGLES]
        assert {0, TM.AA, TM.EO, TM.AA | TM.EO} <= set(flags)
    RH.check_images(H.HostRunner(host), specs, lambda fl: lane_streams(host, fl), lambda fl: lane_streams(host, fl, triangulate=False), least=10)


def test_triangles_tile_the_rings_in_exact_arithmetic(host):
    """(a)"""
    seen = 0
    for name in ("imaged", "random", "grid"):
        fl, routes = RH.want(host, name)[:2]
        pos, _, idx, meshes = lane_streams(host, fl)
        seen += RH.check_exact_areas(fl, routes, pos, idx, meshes)
    assert seen >= 25


def test_image_equals_libtess2_and_fringe_equals_the_reference(host, ref):
    """(d) Without AA the triangles' image is the image of libtess2's TESS_POLYGONS triangulation of the same rings. (e) With AA, on
    libtess2's boundary contours of DONUT and B: the first 2V vertices and 6V indices are strokerConcaveFillEndAA's bit for bit."""
    run = H.HostRunner(host)
    tgt = R.Target(42, 42, 43, -1, -1)
    for name in ("donut", "b"):
        contours = [np.array(c, dtype=F) for c in RM.DRAWS[name][0]]
        tf, _ = H.tess_frame(ref, name, contours, tgt, TM.COLOR, False)
        fl = H.Flat([(contours, TM.CONCAVE, TM.COLOR, 1.0)])
        pos, col, idx, meshes = lane_streams(host, fl)
        assert len(meshes) == 1 and int(meshes[0]["subpath_kind"]) == TM.FILL_KIND
        got = run.painted(K.finish(R.make(name, pos, col, idx, meshes.copy(), tgt)), tgt)
        want = run.painted(tf, tgt)
        assert int((want != tgt.background()).sum()) > 300 and np.array_equal(got, want), (name, H.where(got, want))
        b = H.boundary_of(ref, contours, 0)
        assert sorted(len(q) for q in b) == sorted(len(q) for q in contours)
        fl = H.Flat([(b, TM.CONCAVE | TM.AA, TM.COLOR, 1.0)])
        pos, col, idx, meshes = lane_streams(host, fl)
        V, Hn = sum(len(q) for q in b), len(b) - 1
        assert len(meshes) == 1 and (int(meshes[0]["num_vertices"]), int(meshes[0]["num_indices"])) == (3 * V, 6 * V + 3 * (V + 2 * Hn - 2))
        rpos, rcol, ridx = TC._reference_mesh(ref, contours, TM.COLOR, 1.0, 0)
        assert np.array_equal(pos[:2 * V].view(np.uint32), rpos[:2 * V].view(np.uint32)) and np.array_equal(col[:2 * V], rcol[:2 * V])
        assert np.array_equal(idx[:6 * V], ridx[:6 * V])
        assert np.array_equal(pos[2 * V:].view(np.uint32), pos[0:2 * V:2].view(np.uint32))   # the interior: the moved vertices
