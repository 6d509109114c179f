"""CPU: dashed strokes, pinned without a GPU.
  1. the specification's worked cases and hand-checked corner cases, through the sequential model (tests/dash_model.py) AND the host
     build of the lane code (vgxt_dash of libvgx_hosttest.so: csrc/vgx_dash.h, the functions the kernels run per lane);
  2. vgx_dash_validate, rule by rule;
  3. the lane code against the model, bit for bit, on random walks, circles and the oracle's flatten output;
  4. the condition under which tests/test_gpu_dash.py may hand pieces to the reference's stroker;
  5. examples/vgx_dash_example.cpp compiles and links against libvgx.so.
tests/test_gpu_dash.py runs the kernels on the same families."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dash_model as M
import dash_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def both(lists, closed, entries, sub_draw=None):
    """The model's pieces for the lists (draw l for list l unless sub_draw says otherwise), after checking that the lane code gives
    the same bytes."""
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes(entries)
    sd = np.arange(len(lists), dtype=np.uint32) if sub_draw is None else np.asarray(sub_draw, dtype=np.uint32)
    st, mp, ms, md, msrc = M.dash(poly, subs, sd, dashes, pattern)
    hst, _, hp, hs, hd, hsrc = U.host_dash(poly, subs, sd, dashes, pattern)
    assert st == hst == 0, (st, hst)
    U.assert_same((hp, hs, hd, hsrc), (mp, ms, md, msrc))
    return U.pieces_of(mp, ms), ms, md, msrc


def check(pieces, expected):
    assert len(pieces) == len(expected), (len(pieces), len(expected), [p.tolist() for p in pieces])
    for p, e in zip(pieces, expected):
        e = np.asarray(e, dtype=np.float64).reshape(-1, 2)
        assert p.shape == e.shape, (p.tolist(), e.tolist())
        assert np.all(np.abs(p.astype(np.float64) - e) <= 1e-5 * np.maximum(1.0, np.abs(e))), (p.tolist(), e.tolist())


def line(*xs):
    return np.array([(x, 0.0) for x in xs], dtype=f32)


def test_worked_square():
    sq = np.array([(0, 0), (10, 0), (10, 10), (0, 10)], dtype=f32)
    pieces, subs, draw, src = both([sq], [1], [([4, 2], 1.0)])
    check(pieces, [[(0, 0), (3, 0)], [(5, 0), (9, 0)], [(10, 1), (10, 5)], [(10, 7), (10, 10), (9, 10)], [(7, 10), (3, 10)],
                   [(1, 10), (0, 10), (0, 7)], [(0, 5), (0, 1)]])
    assert np.all(subs["flags"] == 0) and np.all(draw == 0) and np.all(src == 0)
    # vertices that are source vertices are the source's bits
    assert pieces[0][0].tobytes() == sq[0].tobytes() and pieces[3][1].tobytes() == sq[2].tobytes() and pieces[5][1].tobytes() == sq[3].tobytes()


def test_worked_triangle():
    tri = np.array([(0, 0), (3, 0), (3, 4)], dtype=f32)
    pieces, _, _, _ = both([tri], [1], [([5, 1], 0.0)])
    check(pieces, [[(0, 0), (3, 0), (3, 2)], [(3, 3), (3, 4), (0.6, 0.8)]])
    t = f32(4.0 / 5.0)  # the cut lies 4 of the hypotenuse's 5 units behind (3, 4)
    assert pieces[1][2][0] == f32(f32(3) + f32(f32(0 - 3) * t)) and pieces[1][2][1] == f32(f32(4) + f32(f32(0 - 4) * t))
    assert abs(float(pieces[1][2][0]) - 0.59999990) < 1e-7 and abs(float(pieces[1][2][1]) - 0.79999995) < 1e-7


def test_phase_beyond_the_period():
    pieces, _, _, _ = both([line(0, 20)], [0], [([4, 2], 13.0)])  # 13 mod 6 = 1
    check(pieces, [[(0, 0), (3, 0)], [(5, 0), (9, 0)], [(11, 0), (15, 0)], [(17, 0), (20, 0)]])
    same, _, _, _ = both([line(0, 20)], [0], [([4, 2], 1.0)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pieces, same))
    # a phase inside the last gap: the first piece belongs to the next period
    pieces, _, _, _ = both([line(0, 20)], [0], [([4, 2], 5.0)])
    check(pieces, [[(1, 0), (5, 0)], [(7, 0), (11, 0)], [(13, 0), (17, 0)], [(19, 0), (20, 0)]])


def test_zero_on_and_zero_off_entries():
    pieces, _, _, _ = both([line(0, 12)], [0], [([0, 2, 3, 1], 0.0)])
    check(pieces, [[(2, 0), (5, 0)], [(8, 0), (11, 0)]])
    pieces, _, _, _ = both([line(0, 12)], [0], [([3, 0, 2, 1], 0.0)])  # neighbouring "on" intervals stay two pieces
    check(pieces, [[(0, 0), (3, 0)], [(3, 0), (5, 0)], [(6, 0), (9, 0)], [(9, 0), (11, 0)]])


def test_pattern_longer_than_the_list():
    bend = np.array([(0, 0), (2, 0), (2, 2)], dtype=f32)
    pieces, _, _, _ = both([line(0, 5), bend], [0, 0], [([10, 10], 0.0), ([10, 10], 0.0)])
    check(pieces, [[(0, 0), (5, 0)], [(0, 0), (2, 0), (2, 2)]])
    pieces, _, _, _ = both([bend], [1], [([100, 1], 0.0)])  # closed: the closing segment is part of it, the piece stays open
    check(pieces, [[(0, 0), (2, 0), (2, 2), (0, 0)]])


def test_lists_of_fewer_than_two_vertices():
    one = np.array([(7, 7)], dtype=f32)
    none = np.zeros((0, 2), f32)
    pieces, subs, draw, src = both([one, none, line(0, 3), one, none], [0, 0, 0, 1, 0], [([1, 1], 0.0), None], sub_draw=[0, 0, 0, 1, 1])
    # dashed lists with n < 2: nothing; undashed ones: copied whatever n, with their flags
    check(pieces, [[(0, 0), (1, 0)], [(2, 0), (3, 0)], [(7, 7)], np.zeros((0, 2))])
    assert src.tolist() == [2, 2, 3, 4] and draw.tolist() == [0, 0, 1, 1] and subs["flags"].tolist() == [0, 0, 1, 0]


def test_zero_length_segment_inside_a_piece():
    v = np.array([(0, 0), (2, 0), (2, 0), (4, 0)], dtype=f32)
    pieces, _, _, _ = both([v], [0], [([10, 10], 0.0)])
    check(pieces, [[(0, 0), (2, 0), (2, 0), (4, 0)]])
    # an end on the doubled vertex takes the smallest j, a start the largest: neither piece holds the zero-length segment
    pieces, _, _, _ = both([v], [0], [([2, 0], 0.0)])
    check(pieces, [[(0, 0), (2, 0)], [(2, 0), (4, 0)]])
    pieces, _, _, _ = both([v], [0], [([1, 1], 0.0)])
    check(pieces, [[(0, 0), (1, 0)], [(2, 0), (3, 0)]])


def test_cuts_snap_onto_a_vertex_from_either_side():
    v = line(0, 10, 20)
    for first in (10.002, 9.998):  # 2^-8 = 0.0039: the end lands on the vertex, as the vertex
        pieces, _, _, _ = both([v], [0], [([first, 30.0], 0.0)])
        assert len(pieces) == 1 and pieces[0].tobytes() == v[:2].tobytes()
    for gap in (6.001, 5.999):     # the second start at 10 +- 0.001: the piece starts with the vertex
        pieces, _, _, _ = both([v], [0], [([4.0, gap], 0.0)])
        assert pieces[1][0].tobytes() == v[1].tobytes() and len(pieces[1]) == 2
        assert abs(float(pieces[1][1][0]) - (4.0 + gap + 4.0)) < 1e-5
    # beyond the snapping distance the cut stays a cut
    pieces, _, _, _ = both([v], [0], [([10.01, 30.0], 0.0)])
    assert len(pieces) == 1 and len(pieces[0]) == 3 and abs(float(pieces[0][2][0]) - 10.01) < 1e-5
    # an interval that shrinks to nothing: [9.999, 10.001) snaps to [10, 10]
    pieces, _, _, _ = both([v], [0], [([0.002, 30.0], 20.003)])
    assert len(pieces) == 0


def test_validate_rule_by_rule(rt, vgr):
    capi = vgr.capi

    def status(records, pattern):
        d = np.zeros(len(records), capi.dash_dtype)
        for i, r in enumerate(records):
            d[i] = r
        pattern = np.asarray(pattern, dtype=f32)
        st = rt.dash_validate(d, pattern)
        assert M.validate(d, pattern) == st
        poly, subs = U.lists_to_arrays([line(0, 5)], [0])
        hst = U.host_dash(poly, subs, np.zeros(1, np.uint32), d, pattern)[0]
        assert hst == st, (hst, st)
        return st

    ok, bad = capi.VGX_OK, capi.VGX_E_INVALID_ARG
    assert status([(0, 2, 0.0, 0)], [4, 2]) == ok
    assert status([(0, 0, 0.0, 0)], []) == ok                      # not dashed
    assert status([(0, 2, 0.0, 0), (2, 4, 7.5, 0)], [4, 2, 1, 0, 0, 3]) == ok
    assert status([(0, 32, 0.0, 0)], [1] * 32) == ok
    assert status([(0, 2, 0.0, 0)], [4, float("nan")]) == bad      # entries are finite
    assert status([(0, 2, 0.0, 0)], [float("inf"), 2]) == bad
    assert status([(0, 2, 0.0, 0)], [4, -1]) == bad                # ... and >= 0
    assert status([(0, 2, 0.0, 0)], [0, 0]) == bad                 # P > 0
    assert status([(0, 3, 0.0, 0)], [1, 1, 1]) == bad              # count is even
    assert status([(0, 34, 0.0, 0)], [1] * 34) == bad              # ... and <= VGX_DASH_MAX
    assert status([(1, 2, 0.0, 0)], [4, 2]) == bad                 # first + count <= npattern
    assert status([(0xFFFFFFFF, 2, 0.0, 0)], [4, 2]) == bad
    assert status([(0, 2, float("nan"), 0)], [4, 2]) == bad        # phase is finite
    assert status([(0, 2, -1.0, 0)], [4, 2]) == bad                # ... and >= 0
    assert status([(0, 2, 0.0, 1)], [4, 2]) == bad                 # reserved == 0
    assert status([(0, 2, 0.0, 0)], [4, 2, float("nan")]) == bad   # every entry of pattern[], referenced or not
    assert status([(0, 2, 0.0, 0)], [2.0 ** 40, 2]) == bad         # below 2^40


def test_range():
    poly, subs = U.lists_to_arrays([np.array([(0, 0), (float("inf"), 0)], dtype=f32), line(0, 5)], [0, 0])
    d, p = U.make_dashes([([4, 2], 0.0)])
    sd = np.zeros(2, np.uint32)
    assert M.dash(poly, subs, sd, d, p)[0] == M.E_RANGE and U.host_dash(poly, subs, sd, d, p)[0] == M.E_RANGE
    poly, subs = U.lists_to_arrays([np.array([(0, 0), (3e38, 0), (0, 3e38)], dtype=f32)], [1])  # dx * dx overflows
    assert M.dash(poly, subs, sd[:1], d, p)[0] == M.E_RANGE and U.host_dash(poly, subs, sd[:1], d, p)[0] == M.E_RANGE
    # an undashed draw does not look at lengths
    d0, p0 = U.make_dashes([None])
    assert M.dash(poly, subs, sd[:1], d0, p0)[0] == 0 and U.host_dash(poly, subs, sd[:1], d0, p0)[0] == 0


def test_interval_count_and_its_limit():
    """The closed-form interval range of the lane code against the model's entry-by-entry count, around period boundaries and at the
    2^32 - 1 limit; one list just over the limit is VGX_E_RANGE in both (neither walks four billion intervals to find out)."""
    import ctypes as C
    lib = U.hosttest()
    lib.vgxt_dash_intervals.restype = C.c_uint64
    lib.vgxt_dash_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    rng = np.random.default_rng(5)
    cases = [([1.0 / 64, 1.0 / 64], 0.0, (1 << 43) - 2048), ([1.0 / 64, 1.0 / 64], 0.0, 1 << 43), ([1.0 / 64, 1.0 / 64], 0.0, (1 << 43) + 1)]
    for _ in range(400):
        k = 2 * int(rng.integers(1, 5))
        p = [float(f32(x)) for x in rng.uniform(0.0, 4.0, k)]
        if rng.random() < 0.3:
            p[int(rng.integers(0, k))] = 0.0
        if sum(M.q(x) for x in p) == 0:
            continue
        P = sum(M.q(x) for x in p)
        T = int(rng.integers(0, 40)) * P + int(rng.integers(-3, 4)) + int(rng.choice([0, 1, M.q(p[0]), M.q(p[0]) + M.q(p[1])]))
        cases.append((p, float(f32(rng.uniform(0, 3) * sum(p))), max(T, 0)))
    for p, phase, T in cases:
        d, pat = U.make_dashes([(p, phase)])
        A, P, f = M.pattern_of(d[0], pat)
        jlo = C.c_uint64()
        n = lib.vgxt_dash_intervals(d.ctypes.data, pat.ctypes.data, pat.shape[0], T, C.byref(jlo))
        m = M.interval_count(A, P, f, T)
        assert n == m or (n > M.MAX_INTERVALS and m > M.MAX_INTERVALS), (p, phase, T, n, m)  # (beyond the limit the lane code saturates)
    assert M.interval_count([0, 1024, 2048], 2048, 0, (1 << 43) - 2048) == M.MAX_INTERVALS
    assert M.interval_count([0, 1024, 2048], 2048, 0, 1 << 43) == M.MAX_INTERVALS + 1
    # a list of exactly 2^43 fixed units: 0 -> 2^26 -> 2^25 -> ... -> 2^-5 -> 2^-4 (every coordinate and every length a power of two)
    xs = [0.0] + [2.0 ** e for e in range(26, -6, -1)] + [2.0 ** -4]
    poly, subs = U.lists_to_arrays([line(*xs)], [0])
    assert M.prefix_lengths(poly, False)[-1] == 1 << 43
    d, pat = U.make_dashes([([1.0 / 64, 1.0 / 64], 0.0)])
    sd = np.zeros(1, np.uint32)
    assert M.dash(poly, subs, sd, d, pat)[0] == M.E_RANGE and U.host_dash(poly, subs, sd, d, pat)[0] == M.E_RANGE
    # the limit is the call's: two lists of half that each, plus one undashed list
    half = line(*([0.0] + [2.0 ** e for e in range(25, -6, -1)] + [2.0 ** -4]))
    assert M.prefix_lengths(half, False)[-1] == 1 << 42
    poly, subs = U.lists_to_arrays([half, half, line(0, 1)], [0, 0, 0])
    d, pat = U.make_dashes([([1.0 / 64, 1.0 / 64], 0.0), None])
    sd = np.array([0, 0, 1], np.uint32)
    assert M.dash(poly, subs, sd, d, pat)[0] == M.E_RANGE and U.host_dash(poly, subs, sd, d, pat)[0] == M.E_RANGE


def test_nospace_on_the_host_build():
    poly, subs = U.lists_to_arrays([line(0, 20)], [0])
    d, p = U.make_dashes([([4, 2], 0.0)])
    st, z, *_ = U.host_dash(poly, subs, np.zeros(1, np.uint32), d, p, caps=(7, 4))
    assert st == M.E_NOSPACE and z["num_poly_vertices"] == 8 and z["num_subpaths"] == 4


def compare_family(lists, closed, rng, what, ndraws=6):
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes(U.random_dash_entries(rng, ndraws))
    sd = rng.integers(0, ndraws, len(lists)).astype(np.uint32)
    st, mp, ms, md, msrc = M.dash(poly, subs, sd, dashes, pattern)
    hst, z, hp, hs, hd, hsrc = U.host_dash(poly, subs, sd, dashes, pattern)
    assert st == hst == 0, (what, st, hst)
    assert z["num_poly_vertices"] == mp.shape[0] and z["num_subpaths"] == ms.shape[0]
    U.assert_same((hp, hs, hd, hsrc), (mp, ms, md, msrc), what)
    return ms.shape[0]


def test_lane_code_equals_model_random_walks(wl):
    rng = np.random.default_rng(11)
    lists, closed = U.walks(wl, 60, 120)
    assert compare_family(lists, closed, rng, "walks") > 300


def test_lane_code_equals_model_circles():
    rng = np.random.default_rng(12)
    lists, closed = U.circles(rng, 80)
    assert compare_family(lists, closed, rng, "circles") > 300


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_lane_code_equals_model_oracle_flatten(wl, oracle, seed):
    ps = wl.fuzz_paths(seed, npaths=48)
    d = wl.fuzz_draws(ps, seed)
    flat = oracle.flatten(ps, d, apply_transform=True)
    lists = U.pieces_of(flat.poly, flat.subpaths)
    rng = np.random.default_rng(seed)
    n = compare_family(lists, flat.subpaths["flags"], rng, "fuzz %d" % seed, ndraws=d.shape[0])
    assert n > len(lists)


def test_fixture_condition_for_the_gpu_end_to_end_test(wl):
    """Every piece of the end-to-end fixtures keeps its first two and last two vertices at least VG_EPSILON apart as pathPolyline
    measures it (path.cpp:693-696): the reference drops no vertex when a piece is fed to it. Zero violations."""
    total, smallest = 0, np.inf
    for name, lists, closed, pattern, phase in U.gpu_fixture_families(wl):
        poly, subs = U.lists_to_arrays(lists, closed)
        assert not np.any(np.signbit(poly) & (poly == 0)), name  # the reference's identity transformPath turns -0 into +0
        dashes, pat = U.make_dashes([(pattern, phase)])
        st, mp, ms, _, _ = M.dash(poly, subs, np.zeros(len(lists), np.uint32), dashes, pat)
        assert st == 0
        bad, n, least = U.epsilon_violations(mp, ms)
        print("%s: %d pieces, smallest end-segment distSqr %.3g, %d violations" % (name, n, least, bad))
        assert bad == 0, (name, bad, least)
        total += n
        smallest = min(smallest, least)
    print("total %d pieces, smallest %.3g" % (total, smallest))
    assert total > 100000


def test_dash_example_compiles_and_links(rt, tmp_path):
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_dash_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", str(tmp_path / "vgx_dash_example")])
