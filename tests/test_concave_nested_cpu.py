"""CPU: the lane code of vgx_concave_triangulate_nested (csrc/vgx_triangulate_lane.h: tri_nested_route, through libvgx_hosttest.so:
vgxt_concave_triangulate_nested) on flatten output built by hand, against the rule as tests/concave_nested_model.py states it: routes,
sizes, mesh records and every vertex, colour and index, between guard regions. Not resting on the model: exact rational areas, the image
of the triangulated frame against the contour frame's, every group against vgxt_concave_triangulate_rings on that group alone, draws of
one group against that entry, and -- with oracle/_ref/libvgref.so -- libtess2's triangulation. tests/test_gpu_concave_nested.py runs the
same batches through the kernels."""
import numpy as np
import pytest

import concave_nested_harness as NH
import concave_nested_model as NM
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
TRIANGULATED = [n for n in list(NM.DRAWS) + list(NM.LARGE) if (NM.DRAWS.get(n) or NM.LARGE[n])[3] == TM.TRIANGLES]


@pytest.fixture(scope="module")
def host():
    return NH.load_host()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref/libvgref.so (the reference's sources + libtess2) is not built")
    return TC.load_ref(oracle)


def lane(host):
    def tri(fl, caps):
        out = H.Out(*caps)
        st, sizes, routes, _ = NH.host_triangulate(host, fl, out)
        return st, sizes, routes, out.streams(sizes[0], sizes[1], sizes[2]) if st == OK else None, out.guards_intact()
    return tri


def lane_streams(host, fl, entry="nested"):
    if entry == "contours":
        return TH.contours_of(host, fl)
    probe = H.Out(0, 0, 0)
    st, (nm, nv, ni), _, _ = NH.host_triangulate(host, fl, probe, entry=entry)
    assert st == capi.VGX_E_NOSPACE
    out = H.Out(nv, ni, nm)
    assert NH.host_triangulate(host, fl, out, entry=entry)[0] == OK
    return out.streams(nm, nv, ni)


def test_fixtures_are_what_they_are_for(host):
    """Decided on the model: every listed route, group count and triangle count; the fixtures the rings model pins as NESTING."""
    for name in list(NM.DRAWS) + list(NM.LARGE):
        if name.startswith("cap_nested"):
            continue   # its route is pinned by test_lane_code_equals_model; its sizes below
        rings, flags, _, meant, groups, triangles = NM.fixture(name)
        route, tris, notes = NM.draw_route([np.ascontiguousarray(r, dtype=F) for r in rings], bool(flags & TM.EO)) if not flags & TM.AA else (meant, None, None)
        assert route == meant, name
        if route == TM.TRIANGLES and tris is not None:
            assert (len(notes["groups"]), len(tris)) == (groups, triangles), name
        if name not in ("max_rings", "max_rings_plus_1"):
            assert all(np.array_equal(r * 4, np.round(r * 4)) for r in rings), name   # multiples of 0.25
    for name in ("separate", "island", "island_eo"):   # refused by the rings entry, the same rings here
        assert RM.DRAWS[name][3] == RM.NESTING and NM.DRAWS[name][3] == TM.TRIANGLES
        assert all(np.array_equal(a, b) for a, b in zip(RM.DRAWS[name][0], NM.DRAWS[name][0]))
    word = NM.fixture("word")[0]
    assert len(word) == 16 and sum(len(r) for r in word) == 64
    assert len(NM.draw_route(word, False)[2]["groups"]) == 9 > 4 and 9 % 4   # more groups than waves, and not a multiple of four
    grid = NM.fixture("grid_islands")[0]
    assert len(grid) == 289 and sum(len(r) for r in grid) == 1012 + 3 * 144
    for extra, meant in ((0, TM.TRIANGLES), (1, TM.TOO_LONG)):
        for rings in (NM.max_rings(extra), NM.cap_nested_rings(extra)):
            assert sum(len(r) for r in rings) + 2 * (len(rings) - 1) == NM.CAP + extra
    assert len(NM.max_rings(0)) == capi.TRIANGULATE_MAX_VERTICES // 5 == 819


def test_max_rings_is_819_groups_of_depth_0(host):
    """The model's vectorised inside() over all 670 000 ordered ring pairs finds no ring inside another, and the lane code makes one
    triangle per triangle and four of the hexagon: 3 (V + 2 S - 4 G) indices with G = S."""
    rings = NM.fixture("max_rings")[0]
    depth, outer = NM.classify(rings, False)
    assert not depth.any() and outer.tolist() == list(range(819))
    st, (nm, nv, ni), routes, _ = NH.host_triangulate(host, NH.want(host, "max_rings")[0], H.Out(0, 0, 0))
    assert routes.tolist() == [TM.TRIANGLES] and (nm, nv, ni) == (1, 2460, 3 * 822)


def test_random_sets_never_stall(host):
    """Every random set that passes NOT_SIMPLE and NESTING is triangulated; a hole that fell inside a hole is an island now."""
    fl, routes, _, _, _, _, notes = NH.want(host, "random")
    routes = routes.tolist()
    assert len(routes) == 20 and set(routes) <= {TM.TRIANGLES, TM.NOT_SIMPLE, RM.NESTING} and routes.count(TM.TRIANGLES) >= 10, routes
    rings_routes = NH.RH.want(host, "random")[1].tolist()
    assert all(a == b or (a == TM.TRIANGLES and b == RM.NESTING) for a, b in zip(routes, rings_routes))
    assert all(len(notes[d]["groups"]) > 1 for d in range(20) if routes[d] != rings_routes[d])


def test_stream_order_table_holds_the_entry():
    import stream_order as SO
    rows = [r for r in SO.CASES if r.entry == "vgx_concave_triangulate_nested"]
    assert len(rows) == 1 and rows[0].cls == SO.ASYNC and "vgx_concave_triangulate_nested" in SO.stream_entries()
    assert any(rows[0].header in line for line in SO.header_text().splitlines())


@pytest.mark.parametrize("name", ["fixtures", "mixed", "random", "rings_fixtures", "rings_mixed", "rings_single", "grid_islands", "max_rings", "max_rings_plus_1",
                                  "cap_nested", "cap_nested_plus_1"])
def test_lane_code_equals_model(host, name):
    NH.check_against_model(host, name, lane(host))


@pytest.mark.parametrize("short", ["vertices", "indices", "meshes"])
def test_nospace_gives_the_need_and_writes_nothing(host, short):
    fl, routes, pos, _, idx, meshes, _ = NH.want(host, "mixed")
    nv, ni, nm = len(pos), len(idx), len(meshes)
    out = H.Out(nv - (short == "vertices"), ni - (short == "indices"), nm - (short == "meshes"))
    st, sizes, got, _ = NH.host_triangulate(host, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (nm, nv, ni) and got.tolist() == routes.tolist()
    assert out.guards_intact() and out.untouched()


def test_no_room_at_all_still_gives_routes_and_need(host):
    fl, routes, pos, _, idx, meshes, _ = NH.want(host, "fixtures")
    out = H.Out(0, 0, 0)
    st, sizes, got, _ = NH.host_triangulate(host, fl, out)
    assert st == capi.VGX_E_NOSPACE and sizes == (len(meshes), len(pos), len(idx)) and got.tolist() == routes.tolist() and out.guards_intact()


@pytest.mark.parametrize("name,least", [("rings_fixtures", 14), ("rings_mixed", 5), ("rings_single", 5)])
def test_draws_of_one_group_get_the_rings_entry_s_words(host, name, least):
    """Not through the model: the two host entries on the rings model's own batches."""
    fl = NH.want(host, name)[0]
    a, b = lane_streams(host, fl), lane_streams(host, fl, entry="rings")
    ra, rb = NH.host_triangulate(host, fl, H.Out(0, 0, 0))[2], NH.host_triangulate(host, fl, H.Out(0, 0, 0), entry="rings")[2]
    more = NH.check_one_group_draws_equal_the_rings_entry(host, name, a, b, ra, rb, least)
    assert more == {"rings_fixtures": 3, "rings_mixed": 2, "rings_single": 0}[name]   # island, island_eo, separate


@pytest.mark.parametrize("name", TRIANGULATED)
def test_every_group_gets_the_rings_entry_s_triangles(host, name):
    n = NH.check_groups_equal_the_rings_entry(name, lambda specs: lane_streams(host, H.Flat(specs)), lambda specs: lane_streams(host, H.Flat(specs), entry="rings"))
    assert n == NM.fixture(name)[4]


@pytest.mark.parametrize("name,least", [("mixed", 5), ("fixtures", 3), ("rings_fixtures", 6)])
def test_refused_draws_hold_the_contour_route_bytes(host, name, least):
    fl, routes = NH.want(host, name)[:2]
    a, b = lane_streams(host, fl), lane_streams(host, fl, entry="contours")
    refused = [d for d in range(len(routes)) if routes[d] > TM.TRIANGLES]
    assert len(refused) >= least
    for d in refused:
        assert NH.draw_bytes(a, d) == NH.draw_bytes(b, d) and len(NH.draw_bytes(a, d)) == (2 if fl.specs[d][1] & TM.AA else 1)


@pytest.mark.parametrize("name,least", [("imaged", None), ("random", 10)])
def test_image_of_the_triangles_equals_image_of_the_contours(host, name, least):
    """Both fill rules, with and without AA, in one frame at alpha 128. least: the listed TRIANGLES routes (random: what the rings
    model's own test asks of the same sets)."""
    specs, meant = NH.batch(name)
    if name == "imaged":
        least = meant.count(TM.TRIANGLES)
        assert least >= 15
        flags = [s[1] & (TM.AA | TM.EO) for s, r in zip(specs, meant) if r == TM.TRIANGLES]
        assert {0, TM.AA, TM.EO, TM.AA | TM.EO} <= set(flags)
    NH.check_images(H.HostRunner(host), specs, lambda fl: lane_streams(host, fl), lambda fl: lane_streams(host, fl, entry="contours"), least=least)


def test_triangles_tile_the_groups_in_exact_arithmetic(host):
    seen = 0
    for name in ("fixtures", "random", "grid_islands", "max_rings"):
        fl, routes = NH.want(host, name)[:2]
        pos, _, idx, meshes = lane_streams(host, fl)
        seen += NH.check_exact_areas(fl, routes, pos, idx, meshes)
    assert seen >= 14 + 10 + 2


def test_image_equals_libtess2(host, ref):
    """Without AA the triangles' image is the image of libtess2's TESS_POLYGONS triangulation of the same rings."""
    run = H.HostRunner(host)
    tgt = R.Target(96, 84, 96, -2, -2)
    for name in ("island", "bullseye", "word", "two_donuts_interleaved"):
        contours = [np.array(c, dtype=F) for c in NM.fixture(name)[0]]
        tf, _ = H.tess_frame(ref, name, contours, tgt, TM.COLOR, False)
        fl = H.Flat([(contours, TM.CONCAVE, TM.COLOR, 1.0)])
        pos, col, idx, meshes = lane_streams(host, fl)
        assert len(meshes) == 1 and int(meshes[0]["subpath_kind"]) == TM.FILL_KIND
        got = run.painted(K.finish(R.make(name, pos, col, idx, meshes.copy(), tgt)), tgt)
        want = run.painted(tf, tgt)
        assert int((want != tgt.background()).sum()) > 300 and np.array_equal(got, want), (name, H.where(got, want))
