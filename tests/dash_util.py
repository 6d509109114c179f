"""Shared by tests/test_dash_cpu.py and tests/test_gpu_dash.py: fixtures, the host build of the lane code (vgxt_dash of
libvgx_hosttest.so) and the comparison against tests/dash_model.py."""
import ctypes as C
import importlib
import os

import numpy as np

import dash_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
capi = importlib.import_module("vg-renderer_amd.capi")


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def lists_to_arrays(lists, closed):
    """[float32 [n, 2]] + closed flags -> (poly, subpaths)."""
    subs = np.zeros(len(lists), capi.subpath_dtype)
    n = np.array([len(v) for v in lists], dtype=np.uint64)
    subs["num_vertices"] = n
    subs["first_vertex"] = np.cumsum(n) - n
    subs["flags"] = np.asarray(closed, dtype=np.uint32)
    poly = np.concatenate([np.asarray(v, dtype=f32).reshape(-1, 2) for v in lists]) if len(lists) else np.zeros((0, 2), f32)
    return poly, subs


def walks(wl, n, nseg, seed=5678):
    """workloads.random_walk_polylines as open vertex lists (its path arguments ARE the transformed polylines: identity draws)."""
    ps, _ = wl.random_walk_polylines(n=n, nseg=nseg, seed=seed)
    pts = np.asarray(ps.args, dtype=f32).reshape(n, nseg + 1, 2)
    return [pts[i] for i in range(n)], [0] * n


def circles(rng, count):
    """Closed sampled circles: radius 5-300, 8-200 vertices, centres in [0, 2000)^2. No negative zeros."""
    out = []
    for _ in range(count):
        r, k = rng.uniform(5.0, 300.0), int(rng.integers(8, 201))
        c = rng.uniform(0.0, 2000.0, 2)
        a = np.arange(k) * (2.0 * np.pi / k) + rng.uniform(0, 2 * np.pi)
        v = (np.stack([np.cos(a), np.sin(a)], axis=1) * r + c).astype(f32) + f32(0.0)
        out.append(v)
    return out, [1] * count


def gpu_fixture_families(wl):
    """The fixtures of the GPU end-to-end test (tests/test_gpu_dash.py): (name, lists, closed, pattern, phase)."""
    w, wc = walks(wl, 200, 200)
    c, cc = circles(np.random.default_rng(2024), 200)
    return [("walks [12,6]", w, wc, [12.0, 6.0], 0.0), ("walks [5,3,1,3] phase 2.5", w, wc, [5.0, 3.0, 1.0, 3.0], 2.5), ("walks [0.75,0.5]", w, wc, [0.75, 0.5], 0.0),
            ("circles [4,2] phase 1", c, cc, [4.0, 2.0], 1.0), ("circles [10,10]", c, cc, [10.0, 10.0], 0.0)]


def make_dashes(entries):
    """entries: per draw None (undashed) or (pattern list, phase) -> (dash records, pattern array)."""
    d = np.zeros(len(entries), capi.dash_dtype)
    pat = []
    for i, e in enumerate(entries):
        if e is None:
            continue
        d["first"][i], d["count"][i], d["phase"][i] = len(pat), len(e[0]), e[1]
        pat += list(e[0])
    return d, np.array(pat, dtype=f32)


def random_dash_entries(rng, ndraws, undashed=0.25):
    out = []
    for _ in range(ndraws):
        if rng.random() < undashed:
            out.append(None)
            continue
        k = 2 * int(rng.integers(1, 5))
        p = rng.uniform(0.3, 40.0, k)
        if rng.random() < 0.2:
            p[int(rng.integers(0, k))] = 0.0
        out.append((list(p), float(rng.uniform(0, 100.0)) if rng.random() < 0.7 else 0.0))
    return out


# ---- the lane code on the host ------------------------------------------------------------------------------------------
class DashOut(C.Structure):
    _fields_ = [("poly", C.c_void_p), ("subpaths", C.c_void_p), ("subpath_draw", C.c_void_p), ("subpath_src", C.c_void_p),
                ("cap_poly_vertices", C.c_uint64), ("cap_subpaths", C.c_uint64)]


_host = None


def hosttest():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(ROOT, "vg-renderer_amd", "libvgx_hosttest.so"))
        _host.vgxt_dash.restype = C.c_int
        _host.vgxt_dash.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return _host


def _ptr(a):
    return a.ctypes.data if a.size else None


def host_dash(poly, subs, sub_draw, dashes, pattern, caps=None):
    """vgxt_dash: (status, sizes dict, poly, subpaths, subpath_draw, subpath_src). caps: (vertices, sub-paths) instead of the
    counted sizes."""
    lib = hosttest()
    poly = np.ascontiguousarray(poly, dtype=f32)
    subs = np.ascontiguousarray(subs)
    sub_draw = np.ascontiguousarray(sub_draw, dtype=np.uint32)
    dashes = np.ascontiguousarray(dashes)
    pattern = np.ascontiguousarray(pattern, dtype=f32)
    sizes = capi.Sizes()
    args = (_ptr(poly), _ptr(subs), _ptr(sub_draw), subs.shape[0], _ptr(dashes), dashes.shape[0], _ptr(pattern), pattern.shape[0])
    st = lib.vgxt_dash(*args, None, C.byref(sizes))
    z = sizes.as_dict()
    if st != 0:
        return st, z, None, None, None, None
    nv, ns = caps if caps is not None else (z["num_poly_vertices"], z["num_subpaths"])
    op = np.zeros((max(nv, 1), 2), f32)
    os_ = np.zeros(max(ns, 1), capi.subpath_dtype)
    od, osrc = np.zeros(max(ns, 1), np.uint32), np.zeros(max(ns, 1), np.uint32)
    out = DashOut(op.ctypes.data, os_.ctypes.data, od.ctypes.data, osrc.ctypes.data, nv, ns)
    st = lib.vgxt_dash(*args, C.byref(out), C.byref(sizes))
    z = sizes.as_dict()
    if st != 0:
        return st, z, None, None, None, None
    return st, z, op[:z["num_poly_vertices"]], os_[:z["num_subpaths"]], od[:z["num_subpaths"]], osrc[:z["num_subpaths"]]


def assert_same(got, want, what=""):
    """(poly, subpaths, subpath_draw, subpath_src) twice: positions as bit patterns, everything else as integers."""
    gp, gs, gd, gsrc = got
    wp, ws, wd, wsrc = want
    assert gs.shape[0] == ws.shape[0], (what, "pieces", gs.shape[0], ws.shape[0])
    for k in ("first_vertex", "num_vertices", "flags"):
        assert np.array_equal(gs[k], ws[k]), (what, k)
    assert np.array_equal(np.asarray(gd).view(np.uint32), wd), (what, "subpath_draw")
    assert np.array_equal(np.asarray(gsrc).view(np.uint32), wsrc), (what, "subpath_src")
    assert gp.shape == wp.shape, (what, "vertices", gp.shape, wp.shape)
    assert np.array_equal(np.ascontiguousarray(gp).view(np.uint32), np.ascontiguousarray(wp).view(np.uint32)), (what, "positions")


def pieces_of(poly, subs):
    return [poly[int(s["first_vertex"]):int(s["first_vertex"]) + int(s["num_vertices"])] for s in subs]


def epsilon_violations(poly, subs):
    """Pieces whose first two or last two vertices are closer than VG_EPSILON the way pathPolyline measures it (reference
    src/path.cpp:693-696): the reference would drop a vertex of such a piece. Returns (violations, pieces, smallest distSqr)."""
    bad, smallest = 0, np.inf
    for v in pieces_of(poly, subs):
        if len(v) < 2:
            continue
        worst = np.inf
        for a, b in ((v[0], v[1]), (v[-2], v[-1])):
            dx, dy = f32(a[0] - b[0]), f32(a[1] - b[1])
            worst = min(worst, float(f32(f32(dx * dx) + f32(dy * dy))))
        smallest = min(smallest, worst)
        bad += worst < float(f32(1e-5))  # VG_EPSILON
    return bad, subs.shape[0], smallest
