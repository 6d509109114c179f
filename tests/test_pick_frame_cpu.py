"""CPU: the lane code of vgx_pick_frame (csrc/vgx_pick.h through libvgx_hosttest.so: vgxt_pick_frame, a plain loop over queries, meshes
and triangles or edges) against the numpy statement of the specification (tests/pick_frame_model.py), against the IMAGE vgxt_raster_concave
draws of the ID frame (relation (a) of include/vgx.h: a check that does not rest on the model), against vgxt_pick where the two calls must
agree (relation (b)), and the coverage decision against exact rational arithmetic. Exact everywhere, in all four words of every hit; the
GPU suite (tests/test_gpu_pick_frame.py) makes the same comparisons on the kernels."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import pick_frame_model as PF
import raster_harness as H
import raster_model as R
from raster_harness import draws_struct, first_difference, host, host_pick_frame, relation_b_queries, same  # noqa: F401 (host: fixture)

capi = PF.capi
F = np.float32
D = np.float64
NONE = PF.NONE
ALL = H.OPEN


@pytest.mark.parametrize("key", PF.ALL, ids=lambda k: "-".join(str(v) for v in k))
def test_lane_code_equals_model(host, key):
    f, qs = PF.frame(key), PF.query_set(key)
    PF.check_conditions(key)
    want = PF.expected(key)
    got = host_pick_frame(host, f, qs.queries)
    assert same(got, want.hits), first_difference(got, want.hits, qs.queries)
    # with the boxes handed in instead of computed by the call: the same words
    assert same(host_pick_frame(host, f, qs.queries, with_bounds=True), got)


def test_cover_many_is_raster_models_cover():
    """The model's many-triangles form of the coverage rule against raster_model.cover, triangle by triangle: half-integer lattices (ties
    and zero edge values everywhere), degenerate triangles and random ones."""
    rs = np.random.RandomState(4)
    tri = np.concatenate([rs.randint(0, 8, size=(600, 3, 2)).astype(F) + F(0.5), rs.uniform(0, 8, size=(300, 3, 2)).astype(F)])
    tri[::37, 1] = tri[::37, 0]  # two equal corners
    pts = [(x + 0.5, y + 0.5) for x in range(8) for y in range(8)] + [tuple(p) for p in rs.uniform(0, 8, size=(40, 2)).astype(F).astype(D)]
    zeros = 0
    for px, py in pts:
        cov, zero = PF.cover_many(tri[:, 0], tri[:, 1], tri[:, 2], D(px), D(py))
        zeros += int(zero.sum())
        for k in range(0, tri.shape[0], 7):
            got = R.cover(tri[k, 0], tri[k, 1], tri[k, 2], np.array([px], dtype=D), np.array([py], dtype=D))
            assert bool(cov[k]) == (got is not None and bool(got[0][0])), (k, px, py)
            assert bool(zero[k]) == (got is not None and bool(got[5][0])), (k, px, py)
    assert zeros > 1000


def raster_ids(host, f, skip_transparent=False):
    g, tgt = PF.id_frame(f, skip_transparent)
    return PF.decode_ids(H.host_level(host, "concave", g, tgt), tgt)


@pytest.mark.parametrize("flags", [0, PF.SKIP])
@pytest.mark.parametrize("key", PF.IMAGES, ids=lambda k: "-".join(k))
def test_relation_a_the_image_is_the_oracle(host, key, flags):
    """At every pixel centre the picked mesh is the mesh vgxt_raster_concave leaves in the pixel of the ID frame."""
    f = PF.frame(key)
    ids = raster_ids(host, f, skip_transparent=bool(flags))
    got = host_pick_frame(host, f, PF.centre_queries(f.target, flags))
    mesh = np.where(got["mesh"] == NONE, -1, got["mesh"].astype(np.int64)).reshape(f.target.height, f.target.width)
    assert np.array_equal(mesh, ids), np.argwhere(mesh != ids)[:5]
    assert (ids >= 0).any()
    if flags and key == ("concave", "aa_seam"):  # the flag does drop something: a fringe's outer ring was on top somewhere
        assert not np.array_equal(raster_ids(host, f), ids)


def test_relation_b_equals_vgx_pick_away_from_edges(host):
    f, q, want = relation_b_queries()
    got = host_pick_frame(host, f, q)
    old = H.host_pick(host, f, q)
    assert same(got, want)
    assert same(got, old), first_difference(got, old, q)
    assert int((got["mesh"] != NONE).sum()) > 100 and int((got["mesh"] == NONE).sum()) > 100


@pytest.mark.parametrize("key", [("concave", "state"), ("frame", "stack_clip")], ids=lambda k: k[1])
def test_click_through_walks_the_visible_stack(host, key):
    """mesh_end = the previous hit's mesh, until "none": the model's descending list of all hit meshes at the point."""
    f, qs, a = PF.frame(key), PF.query_set(key), PF.expected(key)
    deep = [q for q in range(qs.centres) if len(a.stack[q]) >= 2]
    assert len(deep) >= 6
    longest = max(deep, key=lambda q: len(a.stack[q]))
    for qi in deep[::max(1, len(deep) // 6)][:6] + [longest]:
        got, end = [], NONE
        for _ in range(len(a.stack[qi]) + 1):
            q = qs.queries[qi:qi + 1].copy()
            q["mesh_end"] = end
            h = host_pick_frame(host, f, q)[0]
            if h["mesh"] == NONE:
                assert tuple(h) == (NONE, NONE, NONE, NONE)
                break
            got.append(int(h["mesh"]))
            end = int(h["mesh"])
        assert got == a.stack[qi]
        if len(got) > 12:
            break  # one long walk is enough


def test_range_that_begins_behind_a_regions_clip_meshes(host):
    """S is NONE at the start of the range, as in vgx_raster_frame: In fails everywhere, Out passes."""
    key = ("frame", "clips")
    f = PF.frame(key)
    q = PF.centre_queries(f.target)
    begin = 5  # behind the clip meshes 1, 2 (region 1) and 4 (region 2)
    want = PF.pick(f, q, mesh_begin=begin, prep=PF._prepare_cached(key))
    got = host_pick_frame(host, f, q, begin=begin)
    assert same(got, want.hits)
    assert not want.passed_in.any() and want.refused_in.any() and want.passed_out.any()
    whole = PF.pick(f, q, prep=PF._prepare_cached(key))
    assert not same(whole.hits, want.hits)
    # the image of the same range says the same
    g, tgt = PF.id_frame(f)
    ids = PF.decode_ids(H.host_level(host, "concave", g, tgt, begin=begin), tgt)
    assert np.array_equal(np.where(got["mesh"] == NONE, -1, got["mesh"].astype(np.int64)).reshape(ids.shape), ids)
    # a mesh_end inside the table ends the range
    assert same(host_pick_frame(host, f, q, begin=0, end=4), PF.pick(f, q, mesh_end=4, prep=PF._prepare_cached(key)).hits)


def test_mesh_with_a_draw_beyond_the_table(host):
    key = ("frame", "clips")
    f = PF.frame(key)
    q = PF.centre_queries(f.target)[:300]
    meshes = f.meshes.copy()
    meshes["draw"][7] = f.draws.shape[0]
    got = host_pick_frame(host, f, q, meshes=meshes, want=capi.VGX_E_INVALID_ARG)
    assert (got.view(np.uint32) == NONE).all()
    # outside the range the record is not looked at
    want = PF.pick(f, q, mesh_end=7, prep=PF._prepare_cached(key))
    assert same(host_pick_frame(host, f, q, meshes=meshes, end=7), want.hits)
    # nqueries == 0: the status is decided all the same
    host_pick_frame(host, f, q[:0], meshes=meshes, want=capi.VGX_E_INVALID_ARG)


def test_host_return_values(host):
    f = PF.frame(("frame", "clips"))
    d, s = f.desc(), draws_struct(f)
    q = np.zeros(257, dtype=capi.pick_query_dtype)
    h = np.zeros(257, dtype=capi.pick_hit_dtype)
    st = np.zeros(2, dtype=np.uint32)

    def call(desc=d, mb=None, state=s, queries=q.ctypes.data, n=1, hits=h.ctypes.data, status=st.ctypes.data, begin=0, end=ALL):
        return host.vgxt_pick_frame(C.byref(desc) if desc is not None else None, mb, begin, end, C.byref(state) if state is not None else None, queries, n,
                                    hits, status)

    assert call() == capi.VGX_OK
    assert call(n=257) == capi.VGX_E_RANGE
    assert call(n=256) == capi.VGX_OK
    assert call(desc=None) == capi.VGX_E_INVALID_ARG
    assert call(state=None) == capi.VGX_E_INVALID_ARG
    assert call(queries=None) == capi.VGX_E_INVALID_ARG
    assert call(hits=None) == capi.VGX_E_INVALID_ARG
    assert call(queries=None, hits=None, n=0) == capi.VGX_OK
    assert call(status=None) == capi.VGX_OK
    assert call(queries=q.ctypes.data + 8) == capi.VGX_E_INVALID_ARG
    assert call(hits=h.ctypes.data + 4) == capi.VGX_E_INVALID_ARG
    assert call(status=st.ctypes.data + 2) == capi.VGX_E_INVALID_ARG
    assert call(mb=q.ctypes.data + 8) == capi.VGX_E_INVALID_ARG
    nd = f.draws.shape[0]
    assert call(state=capi.RasterDraws(f.draws.ctypes.data, f.dstate.ctypes.data, nd, 1)) == capi.VGX_E_INVALID_ARG          # reserved != 0
    assert call(state=capi.RasterDraws(None, f.dstate.ctypes.data, nd, 0)) == capi.VGX_E_INVALID_ARG
    assert call(state=capi.RasterDraws(f.draws.ctypes.data, None, nd, 0)) == capi.VGX_E_INVALID_ARG
    assert call(state=capi.RasterDraws(f.draws.ctypes.data + 2, f.dstate.ctypes.data, nd, 0)) == capi.VGX_E_INVALID_ARG
    assert call(state=capi.RasterDraws(None, None, 0, 0)) == capi.VGX_OK and st[0] == capi.VGX_E_INVALID_ARG   # every mesh names a draw >= 0 draws
    assert call(state=capi.RasterDraws(None, None, 0, 0), begin=3, end=3) == capi.VGX_OK and st[0] == capi.VGX_OK  # an empty range
    p = [a.ctypes.data for a in (f.pos, f.color, f.idx, f.meshes)]
    assert call(desc=capi.CacheDesc(p[0], p[1], p[2], p[3], 0xFFFFFFFF, f.nv, f.ni)) == capi.VGX_E_RANGE
    assert call(desc=capi.CacheDesc(None, p[1], p[2], p[3], f.nm, f.nv, f.ni)) == capi.VGX_E_INVALID_ARG
    assert call(desc=capi.CacheDesc(p[0] + 4, p[1], p[2], p[3], f.nm, f.nv, f.ni)) == capi.VGX_E_INVALID_ARG
    assert call(desc=capi.CacheDesc(p[0], p[1], p[2] + 1, p[3], f.nm, f.nv, f.ni)) == capi.VGX_E_INVALID_ARG
    h[:] = (1, 2, 3, 4)
    assert call(desc=capi.CacheDesc(None, None, None, None, 0, 0, 0), n=3) == capi.VGX_OK
    assert np.all(h[:3].view(np.uint32) == NONE) and tuple(h[3]) == (1, 2, 3, 4)


def exact_cover(a, b, c, p):
    """The coverage rule of vgx_raster over the rationals: box, sign of every edge value against the orientation, the tie rule."""
    (ax, ay), (bx, by), (cx, cy), (px, py) = [tuple(Fraction(float(v)) for v in pt) for pt in (a, b, c, p)]
    if not (min(ax, bx, cx) <= px <= max(ax, bx, cx) and min(ay, by, cy) <= py <= max(ay, by, cy)):
        return False
    A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    if A == 0:
        return False
    s = 1 if A > 0 else -1
    for (ux, uy), (vx, vy) in (((ax, ay), (bx, by)), ((bx, by), (cx, cy)), ((cx, cy), (ax, ay))):
        E = s * ((vx - ux) * (py - uy) - (vy - uy) * (px - ux))
        dx, dy = s * (vx - ux), s * (vy - uy)
        if not (E > 0 or (E == 0 and (dy > 0 or (dy == 0 and dx < 0)))):
            return False
    return True


def test_coverage_has_the_exact_sign():
    """Where the header says the binary64 expressions carry the exact geometric sign -- vertices and query points of one binade, as on
    these frames -- the model's coverage decision is the decision of exact rational arithmetic: on `lattice_clip` (edges and vertices
    through pixel centres: the tie rule in every form) at every pixel centre, and on the Tiger frame's own triangles at vertices,
    representable edge midpoints and random points of the triangle's box."""
    f = PF.frame(("frame", "lattice_clip"))
    Tr = PF._prepare_cached(("frame", "lattice_clip")).tris
    q = PF.centre_queries(f.target)
    ties = 0
    for k in range(0, q.shape[0], 3):
        px, py = D(q["x"][k]), D(q["y"][k])
        cov, zero = PF.cover_many(Tr.a, Tr.b, Tr.c, px, py)
        ties += int(zero.sum())
        for g in np.nonzero(zero | cov)[0]:
            assert bool(cov[g]) == exact_cover(Tr.a[g], Tr.b[g], Tr.c[g], (px, py)), (k, int(g))
    assert ties > 100
    # `centres`: contour meshes whose every vertex is a pixel centre -- at every pixel centre the winding number, and with it the
    # coverage decision, is the one of rational arithmetic, and the lane code reports a contour mesh exactly where it says so
    key = ("concave", "centres")
    f, prep = PF.frame(key), PF._prepare_cached(key)
    q = PF.centre_queries(f.target)
    a = PF.pick(f, q, prep=prep)
    inside = np.zeros(q.shape[0], dtype=bool)
    on_edge = 0
    for m, (u, v) in prep.edges.items():
        even_odd = int(f.meshes["subpath_kind"][m]) & capi.CONTOUR_EVEN_ODD
        W = PF.K.winding(u, v, q["x"].astype(D), q["y"].astype(D))
        for k in range(q.shape[0]):
            exact = H.exact_winding(u, v, float(q["x"][k]), float(q["y"][k]))
            assert int(W[k]) == exact, (m, k)
            inside[k] |= bool(exact & 1) if even_odd else exact != 0
        on_edge += sum(1 for p in u if (np.abs(q["x"] - p[0]) + np.abs(q["y"] - p[1]) == 0).any())
    assert on_edge >= 6
    top_is_contour = a.contour & (a.hits["mesh"] != NONE)
    assert top_is_contour.any() and inside[top_is_contour].all()
    f = PF.frame(PF.TIGER)
    Tr = PF._prepare_cached(PF.TIGER).tris
    rs = np.random.RandomState(3)
    wrong, n, covered = [], 0, 0
    for g in rs.choice(np.nonzero(Tr.valid)[0], size=1200, replace=False):
        a, b, c = Tr.a[g], Tr.b[g], Tr.c[g]
        u, v = ((a, b), (b, c), (c, a))[g % 3]
        mid = (u.astype(D) + v.astype(D)) / 2.0
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        pts = [(a, b, c)[g % 3], (lo + (hi - lo) * rs.uniform(0, 1, 2).astype(F)).astype(F)]
        if np.array_equal(mid.astype(F).astype(D), mid):
            pts.append(mid.astype(F))
        for p in pts:
            cov, _ = PF.cover_many(a[None], b[None], c[None], D(p[0]), D(p[1]))
            exact = exact_cover(a, b, c, p)
            n += 1
            covered += exact
            if bool(cov[0]) != exact:
                wrong.append((int(g), tuple(p)))
    assert not wrong, (len(wrong), wrong[:5])
    assert n >= 2400 and 100 < covered < n
