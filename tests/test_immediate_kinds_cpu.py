"""The premises of tests/test_gpu_immediate_sequences.py, from the reference alone (no GPU): every kind of immediate_kinds.py has the
property that steers the route of vgx_tessellate_immediate. When one of these fails, the GPU sequences no longer test what they say.

The three host rules the kinds are built around, written down here on purpose (nothing is imported from the product):
  * vgx_period_usable (vgx_route_plan.h): a period P is used when ndraws % P == 0 and ndraws / P >= 32 (VGX_INST_MIN_INSTANCES);
  * vgx_paths_reused (vgx_route_plan.h): grouped mode when ndraws / distinct paths >= 32;
  * the one-walk route of vgx_tessellate_immediate: polyline vertices >= 10 x command instances; its kernel shape, vgx_f1_shape
    (vgx_route_plan.h): 64 x vertices / command instances <= 800 -> the 1024-entry leaf list, > 1500 -> the 3072-entry one.
Batches of at most 2 048 draws (VGX_SMALL_DRAWS) take the frame-sized route whatever they hold."""
import numpy as np
import pytest

import immediate_kinds as K

MIN_INSTANCES = 32
ONE_WALK_VERTS_PER_CMD = 10
F1_LIGHT, F1_HEAVY = 800.0, 1500.0
SMALL_DRAWS = 2048
MAX_MESH_VERTICES = 65536

WITH_REFERENCE = K.SHARED + K.OWN


@pytest.fixture(scope="module")
def counted(oracle):
    return {k: oracle.tessellate(*K.make(k), count_only=True).sizes for k in WITH_REFERENCE}


def per_cmd(sz):
    return sz["num_poly_vertices"] / sz["num_cmd_instances"]


def test_every_kind_is_listed():
    assert sorted(K.PROPS) == sorted(WITH_REFERENCE)
    assert sorted(K.ALL) == sorted(WITH_REFERENCE + K.ERRORS) and len(set(K.ALL)) == len(K.ALL)


@pytest.mark.parametrize("kind", WITH_REFERENCE)
def test_period_distinct_and_curve_length(counted, kind):
    ps, d = K.make(kind)
    ndraws, period, distinct, long_curves = K.PROPS[kind]
    assert d.shape[0] == ndraws
    assert int(d["path"].max()) < ps.npaths
    assert K.period_of(d["path"]) == period
    assert np.unique(d["path"]).shape[0] == distinct
    sz = counted[kind]
    assert sz["num_cmd_instances"] > 0 and sz["num_poly_vertices"] > 0
    assert (per_cmd(sz) >= ONE_WALK_VERTS_PER_CMD) == long_curves, per_cmd(sz)


@pytest.mark.parametrize("kind", WITH_REFERENCE)
def test_learned_route_table_follows_the_host_rules(kind):
    assert (K.MIN_INSTANCES, K.SMALL_DRAWS) == (MIN_INSTANCES, SMALL_DRAWS)
    assert K.LEARNED[kind] == K.route_from_knowledge(*K.PROPS[kind])
    if kind == "thin":  # (a lineTo-only path set never takes the one-walk route: either side of the period rule ends in a periodic / build route)
        assert K.LEARNED[kind] != "route_one_walk"


def test_matrix_cells_and_stale_cells(counted):
    """225 ordered pairs of the shared kinds; in 132 the tags collide with another kind; in 126 of those the knowledge the first call
    runs on (period, distinct paths, vertices, command instances) is not the batch's own."""
    cells = [(a, b) for a in K.SHARED for b in K.SHARED]
    assert len(cells) == 225
    colliding = [(a, b) for a, b in cells if a != b and K.collide(a, b)]
    assert len(colliding) == 132

    def knowledge(k):
        return K.PROPS[k][1:3] + (counted[k]["num_poly_vertices"], counted[k]["num_cmd_instances"])
    stale = [(a, b) for a, b in colliding if knowledge(a) != knowledge(b)]
    assert len(stale) == 126
    # every colliding cell is observable through the stage names: a new tag would run route_build, no colliding kind learns that
    for a, b in colliding:
        assert K.first_call_route(a, b) == K.LEARNED[a] != "route_build"
    for a, b in cells:
        if not K.collide(a, b):
            assert K.first_call_route(a, b) == ("route_frame" if b == "frame2048" else "route_build")
    # the examples of the issue
    for b in ("broken_last", "periodic48", "shuffled64"):
        assert K.first_call_route("periodic64", b) == "route_periodic"
    assert K.first_call_route("shuffled64", "unique") == "route_grouped"
    assert K.first_call_route("unique", "periodic64_small") == "route_one_walk"


def test_shared_kinds_share_one_path_set():
    ps = K.shared_paths()
    assert ps.npaths == K.NPATHS == 3072
    for k in K.SHARED + K.ERRORS:
        assert K.make(k)[0] is ps, k


def test_colliding_kinds_have_equal_ndraws():
    colliding = [k for k in K.SHARED if k not in ("p96x31", "frame2048", "large2049")]
    assert len(colliding) == 12
    for k in colliding + ["nan_draw"]:
        assert K.make(k)[1].shape[0] == K.NDRAWS == 3072, k
    others = sorted(K.make(k)[1].shape[0] for k in ("p96x31", "frame2048", "large2049"))
    assert others == [2048, 2049, 2976]
    assert K.make("empty")[1].shape[0] == 0


def test_instance_counts_on_both_sides_of_the_minimum():
    for k, inst in (("periodic64", 48), ("periodic48", 64), ("fill_only64", 48), ("nothing", 48), ("periodic64_small", 48), ("periodic64_big", 48),
                    ("p96x32", 32), ("p96x31", 31), ("thin", 48), ("tiger10", 10)):
        n, P, distinct, _ = K.PROPS[k]
        assert n % P == 0 and n // P == inst, k
        assert (inst >= MIN_INSTANCES) == (k not in ("p96x31", "tiger10")), k
        assert (n // distinct >= MIN_INSTANCES) == (inst >= MIN_INSTANCES), k  # (no grouped mode either below the minimum)
    for k in ("shuffled64", "broken_last", "broken_first"):  # no period, paths reused: grouped mode
        n, P, distinct, _ = K.PROPS[k]
        assert P == 0 and n // distinct >= MIN_INSTANCES, k
    for k in ("unique", "unique_big", "large2049", "cubics_long", "cubics_short"):  # neither
        n, P, distinct, _ = K.PROPS[k]
        assert P == 0 and n // distinct < MIN_INSTANCES, k


def test_period_48_is_not_a_period_of_64_and_back():
    p48, p64 = K.make("periodic48")[1]["path"], K.make("periodic64")[1]["path"]
    assert not np.array_equal(p48, np.tile(p48[:64], 48))  # a stale period of 64 does not hold for periodic48
    assert not np.array_equal(p64, np.tile(p64[:48], 64))
    assert not np.array_equal(p64, np.tile(p64[:96], 32)) and not np.array_equal(K.make("p96x32")[1]["path"][:3072], np.tile(p64[:64], 48))


def test_broken_kinds_differ_from_periodic64_in_one_path():
    base = K.make("periodic64")[1]
    for k, i in (("broken_last", 3071), ("broken_first", 5)):
        d = K.make(k)[1]
        w = np.flatnonzero(d["path"] != base["path"])
        assert w.tolist() == [i], k
        assert int(d["path"][i]) not in set(base["path"].tolist())
    assert sorted(K.make("shuffled64")[1]["path"].tolist()) == sorted(base["path"].tolist())


def test_big_and_small_kinds_cross_the_shape_breakpoints(counted):
    for base, big in (("periodic64", "periodic64_big"), ("unique", "unique_big")):
        assert 64.0 * per_cmd(counted[base]) <= F1_LIGHT, base
        assert 64.0 * per_cmd(counted[big]) > F1_HEAVY, big
        assert counted[big]["num_cmd_instances"] == counted[base]["num_cmd_instances"]
        assert counted[big]["num_poly_vertices"] > 3 * counted[base]["num_poly_vertices"], big
    assert per_cmd(counted["periodic64_small"]) < ONE_WALK_VERTS_PER_CMD / 2
    assert counted["periodic64_small"]["num_cmd_instances"] == counted["periodic64"]["num_cmd_instances"]
    assert per_cmd(counted["cubics_long"]) > 50 and per_cmd(counted["cubics_short"]) < ONE_WALK_VERTS_PER_CMD
    assert per_cmd(counted["thin"]) < 1.0
    # thin holds the largest per-command scratch of the set, cubics_long more vertices than any same-size kind on the shared set
    assert counted["thin"]["num_cmd_instances"] == max(sz["num_cmd_instances"] for sz in counted.values())


def test_fill_only_and_nothing(counted):
    f, p, z = counted["fill_only64"], counted["periodic64"], counted["nothing"]
    assert 0 < f["num_meshes"] < p["num_meshes"] // 2
    assert z["num_meshes"] == 0 and z["num_vertices"] == 0 and z["num_indices"] == 0
    for k in ("num_poly_vertices", "num_subpaths", "num_cmd_instances"):
        assert z[k] == p[k] == f[k], k


def test_frame_and_large_sides_of_the_small_draws_limit():
    u = K.make("unique")[1]
    f, l = K.make("frame2048")[1], K.make("large2049")[1]
    assert f.shape[0] == SMALL_DRAWS and l.shape[0] == SMALL_DRAWS + 1
    assert f.tobytes() == u[:2048].tobytes() and l.tobytes() == u[:2049].tobytes()


def test_general_stroke_styles_and_path_content():
    capi = K._capi()
    ps, d = K.make("unique")
    assert set(np.unique(ps.cmd_type).tolist()) >= {capi.CMD_MOVE_TO, capi.CMD_LINE_TO, capi.CMD_CUBIC_TO, capi.CMD_CLOSE}
    assert len(set(np.unique(ps.cmd_type).tolist())) >= 8  # every command: quads, arcs, arcTo, polylines, shapes
    assert len(set(d["stroke_flags"].tolist())) >= 20  # caps x joins x AA / not / hairline
    assert (d["stroke_flags"] == 0).any() and (d["fill_flags"] == 0).any() and ((d["stroke_flags"] == 0) & (d["fill_flags"] == 0)).any()
    # the first 64 / 48 / 96 draws (the periods) hold strokes, fills and both
    for P in (48, 64, 96):
        assert (d["stroke_flags"][:P] != 0).sum() > P // 2 and (d["fill_flags"][:P] != 0).sum() > P // 4


def test_nan_draw_is_periodic64_with_one_nan():
    d, base = K.make("nan_draw")[1], K.make("periodic64")[1]
    bad = ~np.isfinite(d["mtx"])
    assert int(bad.sum()) == 1
    m = d["mtx"].copy()
    m[bad] = base["mtx"][bad]
    d2 = d.copy()
    d2["mtx"] = m
    assert d2.tobytes() == base.tobytes()


@pytest.mark.parametrize("kind", [k for k in WITH_REFERENCE if k != "nothing"])
def test_no_mesh_too_large(oracle, kind):
    """A mesh of more than 65 536 vertices would make the kind a test of VGX_E_MESH_TOO_LARGE, not of a route."""
    ref = K.reference(oracle, kind)
    assert 0 < int(ref.meshes["num_vertices"].max()) <= MAX_MESH_VERTICES
