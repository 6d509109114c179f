"""GPU: vgx_dash / vgx_dash_count / vgx_subpath_draws (csrc/vgx_dash.hip).
  1. device output == the sequential model (tests/dash_model.py), bit for bit, on the device's own vgx_flatten + vgx_subpath_draws
     output for fuzz path sets, on random walks and circles, on the skewed case (one 60 000-unit segment under [1,1]) and on a list of
     65 000 vertices under a pattern longer than the list;
  2. sizes: vgx_dash_count == the dev_sizes of vgx_dash; vgx_subpath_draws == np.repeat(arange(ndraws), num_subpaths);
  3. error paths: halved capacities (VGX_E_NOSPACE, exact sizes, nothing written), invalid records / entries
     (VGX_E_INVALID_ARG, nothing written), a scratch that is too small (VGX_E_GROWN, then VGX_OK);
  4. end to end: vgx_flatten -> vgx_dash -> vgx_stroke_* against the reference's strokerPolylineStroke* run on the same pieces;
  5. full size: 10 000 x 1 000 segments under [12,6] against the host build of the lane code (pinned to the model by
     tests/test_dash_cpu.py), by digests per source list and exact totals."""
import importlib

import numpy as np
import pytest

import dash_model as M
import dash_util as U
import hashutil as H

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def to_dev(poly, subs, sub_draw, dashes, pattern):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(poly, dtype=f32).reshape(-1, 2).copy()).cuda() if len(poly) else torch.zeros((1, 2), dtype=torch.float32, device="cuda"),
            torch.from_numpy(np.ascontiguousarray(subs).view(np.uint8).copy()).cuda() if len(subs) else torch.zeros(16, dtype=torch.uint8, device="cuda"),
            torch.from_numpy(np.ascontiguousarray(sub_draw).astype(np.int32)).cuda() if len(sub_draw) else torch.zeros(1, dtype=torch.int32, device="cuda"),
            torch.from_numpy(np.ascontiguousarray(dashes).view(np.uint8).copy()).cuda(),
            torch.from_numpy(np.ascontiguousarray(pattern, dtype=f32).copy()).cuda() if len(pattern) else torch.zeros(1, dtype=torch.float32, device="cuda"))


def run_dash(rt, ctx, poly, subs, sub_draw, dashes, pattern):
    dev = to_dev(poly, subs, sub_draw, dashes, pattern)
    return rt.dash(ctx, dev[0], dev[1], dev[2], len(subs), dev[3], len(dashes), dev[4], len(pattern))


def against_model(rt, ctx, poly, subs, sub_draw, dashes, pattern, what):
    st, mp, ms, md, msrc = M.dash(poly, subs, sub_draw, dashes, pattern)
    assert st == 0, (what, st)
    got = run_dash(rt, ctx, poly, subs, sub_draw, dashes, pattern)
    assert got.sizes["num_poly_vertices"] == mp.shape[0] and got.sizes["num_subpaths"] == ms.shape[0], (what, got.sizes)
    U.assert_same((got.poly, got.subpaths, got.sub_draw, got.sub_src), (mp, ms, md, msrc), what)
    return got


@pytest.mark.parametrize("seed", [100, 101, 102, 103])
def test_device_flatten_then_dash_equals_model(rt, gpu_ctx, wl, seed):
    """The chain on the device: vgx_flatten(apply_transform = 1) -> vgx_subpath_draws -> vgx_dash, every stage's output read back
    only to be compared: sub-path draws against np.repeat, pieces against the model run on the device's own polylines."""
    import torch
    ps = wl.fuzz_paths(seed, npaths=48)
    d = wl.fuzz_draws(ps, seed)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    flat = rt.flatten(gpu_ctx, pset, dd, d.shape[0], apply_transform=True)
    nsub = flat.sizes["num_subpaths"]
    sd = rt.subpath_draws(gpu_ctx, flat.dinfo_dev, d.shape[0], nsub)
    torch.cuda.synchronize()
    sub_draw = sd[:nsub].cpu().numpy().view(np.uint32)
    assert np.array_equal(sub_draw, np.repeat(np.arange(d.shape[0], dtype=np.uint32), flat.draw_info["num_subpaths"]))
    rng = np.random.default_rng(seed)
    dashes, pattern = U.make_dashes(U.random_dash_entries(rng, d.shape[0]))
    st, mp, ms, md, msrc = M.dash(flat.poly, flat.subpaths, sub_draw, dashes, pattern)
    assert st == 0
    got = rt.dash(gpu_ctx, flat.poly_dev, flat.subs_dev, sd, nsub, torch.from_numpy(dashes.view(np.uint8).copy()).cuda(), d.shape[0],
                  torch.from_numpy(pattern).cuda(), pattern.shape[0])
    U.assert_same((got.poly, got.subpaths, got.sub_draw, got.sub_src), (mp, ms, md, msrc), "fuzz %d" % seed)
    assert ms.shape[0] > nsub
    pset.close()


def test_walks_and_circles_equal_model(rt, gpu_ctx, wl):
    rng = np.random.default_rng(21)
    w, wc = U.walks(wl, 60, 120)
    c, cc = U.circles(rng, 80)
    lists, closed = w + c, wc + cc
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes(U.random_dash_entries(rng, 9))
    sub_draw = rng.integers(0, 9, len(lists)).astype(np.uint32)
    against_model(rt, gpu_ctx, poly, subs, sub_draw, dashes, pattern, "walks + circles")


def test_skewed_segment(rt, gpu_ctx):
    """One segment, 30 000 pieces: the work is one lane per "on" interval, not one lane per segment."""
    poly, subs = U.lists_to_arrays([np.array([(5, 7), (60005, 7)], dtype=f32)], [0])
    dashes, pattern = U.make_dashes([([1.0, 1.0], 0.0)])
    got = against_model(rt, gpu_ctx, poly, subs, np.zeros(1, np.uint32), dashes, pattern, "skewed")
    assert got.sizes["num_subpaths"] == 30000 and got.sizes["num_poly_vertices"] == 60000


def test_long_list_under_a_longer_pattern(rt, gpu_ctx):
    """65 000 vertices, one piece: the whole list."""
    t = np.arange(65000) * 0.01
    v = np.stack([t * 3.0, np.sin(t) * 50.0 + 100.0], axis=1).astype(f32)
    poly, subs = U.lists_to_arrays([v], [0])
    dashes, pattern = U.make_dashes([([1.0e6, 5.0], 0.0)])
    got = against_model(rt, gpu_ctx, poly, subs, np.zeros(1, np.uint32), dashes, pattern, "long list")
    assert got.sizes["num_subpaths"] == 1 and got.sizes["num_poly_vertices"] == 65000
    assert got.poly.tobytes() == v.tobytes()


def sizes_of(bufs):
    z = bufs.dev_sizes.cpu().numpy()
    return {k: int(z[i]) for i, (k, _) in enumerate(U.capi.Sizes._fields_)}


def test_count_equals_dev_sizes_and_grown_then_ok(rt, wl):
    """vgx_dash on a context that never counted: its first guess of the segment tables (from the output capacity) is too small for
    this batch -> VGX_E_GROWN, nothing written; the second call has grown them -> VGX_OK with the sizes vgx_dash_count reports."""
    import torch
    ctx = rt.Context(0)
    lists, closed = U.walks(wl, 400, 400)  # 160 000 segments
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes([([3000.0, 200.0], 0.0)])
    dev = to_dev(poly, subs, np.zeros(len(lists), np.uint32), dashes, pattern)
    bufs = rt.DashBuffers("cuda", 70000, 70000)
    bufs.poly.fill_(-77.0)
    rt.dash_async(ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == U.capi.VGX_E_GROWN
    assert bool((bufs.poly == -77.0).all())
    rt.dash_async(ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == U.capi.VGX_E_NOSPACE  # a walk's 401 vertices nearly all lie in its first piece: far more than 70 000, and the sizes are exact
    need = sizes_of(bufs)
    counted = rt.dash_count(ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2)
    assert counted["num_poly_vertices"] == need["num_poly_vertices"] and counted["num_subpaths"] == need["num_subpaths"]
    hst, z, *_ = U.host_dash(poly, subs, np.zeros(len(lists), np.uint32), dashes, pattern)
    assert hst == 0 and z["num_poly_vertices"] == need["num_poly_vertices"] and z["num_subpaths"] == need["num_subpaths"]
    bufs = rt.DashBuffers("cuda", need["num_poly_vertices"], need["num_subpaths"])
    rt.dash_async(ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == 0 and sizes_of(bufs) == need
    ctx.close()


def test_halved_capacities(rt, gpu_ctx, wl):
    import torch
    lists, closed = U.walks(wl, 40, 100)
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes([([12.0, 6.0], 0.0)])
    dev = to_dev(poly, subs, np.zeros(len(lists), np.uint32), dashes, pattern)
    counted = rt.dash_count(gpu_ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2)
    nv, ns = counted["num_poly_vertices"], counted["num_subpaths"]
    for cv, cs in ((nv // 2, ns), (nv, ns // 2), (nv // 2, ns // 2), (nv - 1, ns), (nv, ns - 1)):
        bufs = rt.DashBuffers("cuda", nv + 64, ns + 64)  # the words behind the stated capacity are the guard
        for t_, val in ((bufs.poly, -77.0), (bufs.subs, 0x5A), (bufs.sub_draw, 0x5A5A5A5A), (bufs.sub_src, 0x5A5A5A5A)):
            t_.fill_(val)
        bufs.cap = (cv, cs)
        rt.dash_async(gpu_ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 1, dev[4], 2, bufs)
        torch.cuda.synchronize()
        assert int(bufs.dev_status.item()) == U.capi.VGX_E_NOSPACE, (cv, cs)
        z = sizes_of(bufs)
        assert z["num_poly_vertices"] == nv and z["num_subpaths"] == ns
        # nothing at all is written: the buffers below the stated capacities and the guard words behind them
        assert bool((bufs.poly == -77.0).all()) and bool((bufs.subs == 0x5A).all())
        assert bool((bufs.sub_draw == 0x5A5A5A5A).all()) and bool((bufs.sub_src == 0x5A5A5A5A).all())


@pytest.mark.parametrize("what", ["odd count", "nan entry", "all-zero pattern", "negative phase", "reserved", "subpath_draw out of range"])
def test_invalid_arguments_write_nothing(rt, gpu_ctx, wl, what):
    import torch
    lists, closed = U.walks(wl, 10, 50)
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes, pattern = U.make_dashes([([12.0, 6.0], 0.0), ([5.0, 5.0, 1.0, 1.0], 2.0)])
    sub_draw = (np.arange(len(lists)) % 2).astype(np.uint32)
    if what == "odd count":
        dashes["count"][1] = 3
    elif what == "nan entry":
        pattern[3] = np.nan
    elif what == "all-zero pattern":
        pattern[:2] = 0.0
    elif what == "negative phase":
        dashes["phase"][0] = -0.5
    elif what == "reserved":
        dashes["reserved"][1] = 1
    else:
        sub_draw[7] = 2
    if what != "subpath_draw out of range":
        assert rt.dash_validate(dashes, pattern) == U.capi.VGX_E_INVALID_ARG
    dev = to_dev(poly, subs, sub_draw, dashes, pattern)
    bufs = rt.DashBuffers("cuda", 4096, 4096)
    for t_, val in ((bufs.poly, -77.0), (bufs.subs, 0x5A), (bufs.sub_draw, 0x5A5A5A5A), (bufs.sub_src, 0x5A5A5A5A)):
        t_.fill_(val)
    rt.dash_async(gpu_ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 2, dev[4], pattern.shape[0], bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == U.capi.VGX_E_INVALID_ARG
    assert bool((bufs.poly == -77.0).all()) and bool((bufs.subs == 0x5A).all())
    assert bool((bufs.sub_draw == 0x5A5A5A5A).all()) and bool((bufs.sub_src == 0x5A5A5A5A).all())
    with pytest.raises(rt.VgxError):
        rt.dash_count(gpu_ctx, dev[0], dev[1], dev[2], len(subs), dev[3], 2, dev[4], pattern.shape[0])


def test_nonfinite_length_is_out_of_range(rt, gpu_ctx):
    import torch
    poly, subs = U.lists_to_arrays([np.array([(0, 0), (4, 0), (np.inf, 3)], dtype=f32), np.array([(0, 0), (9, 9)], dtype=f32)], [0, 0])
    dashes, pattern = U.make_dashes([([1.0, 1.0], 0.0)])
    dev = to_dev(poly, subs, np.zeros(2, np.uint32), dashes, pattern)
    bufs = rt.DashBuffers("cuda", 256, 256)
    bufs.poly.fill_(-77.0)
    rt.dash_async(gpu_ctx, dev[0], dev[1], dev[2], 2, dev[3], 1, dev[4], 2, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == U.capi.VGX_E_RANGE and bool((bufs.poly == -77.0).all())


STYLES = [(cap, join, True, False) for cap in (0, 1, 2) for join in (0, 1, 2)] + [(0, 0, False, False), (1, 2, False, False), (0, 0, True, True)]


def source_pathset(vgr, lists, closed):
    b = vgr.PathSetBuilder()
    for v, c in zip(lists, closed):
        b.begin_path()
        b.move_to(float(v[0][0]), float(v[0][1]))
        for p in v[1:]:
            b.line_to(float(p[0]), float(p[1]))
        if c:
            b.close()
        b.end_path()
    return b.arrays()


def piece_pathset(vgr, poly, subs):
    """One path per piece: MOVE_TO + POLYLINE of the piece."""
    n = subs.shape[0]
    first = subs["first_vertex"].astype(np.int64)
    cmd_type = np.tile(np.array([U.capi.CMD_MOVE_TO, U.capi.CMD_POLYLINE], dtype=np.uint8), n)
    arg_off = np.zeros(2 * n + 1, dtype=np.uint32)
    arg_off[0:2 * n:2] = 2 * first
    arg_off[1:2 * n:2] = 2 * first + 2
    arg_off[2 * n] = 2 * poly.shape[0]
    return vgr.pathset.PathSetArrays(cmd_type, arg_off, np.ascontiguousarray(poly, dtype=f32).reshape(-1), np.arange(n + 1, dtype=np.uint32) * 2)


@pytest.mark.parametrize("family", [0, 1, 2, 3, 4])
def test_end_to_end_against_the_reference_stroker(rt, gpu_ctx, wl, vgr, oracle, family):
    """vgx_flatten -> vgx_subpath_draws -> vgx_dash -> vgx_stroke_* with every cap x join in AA, non-AA and Thin spread over the
    draws, against the oracle tessellating one path per piece (MOVE_TO + POLYLINE, identity transform, the same stroke fields):
    indices and colours equal, positions equal as bit patterns."""
    import torch
    name, lists, closed, pat, phase = U.gpu_fixture_families(wl)[family]
    n = len(lists)
    ps = source_pathset(vgr, lists, closed)
    d = wl.make_draws(n)
    d["path"] = np.arange(n, dtype=np.uint32)
    for i in range(n):
        cap, join, aa, thin = STYLES[i % len(STYLES)]
        wl.set_stroke(d, i, 0xFF2080FF + i, 0.8 if thin else 3.0 + (i % 4), cap, join, aa=aa)
    assert np.all(d["fill_flags"] == 0)
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    flat = rt.flatten(gpu_ctx, pset, dd, n, apply_transform=True)
    nsub = flat.sizes["num_subpaths"]
    assert nsub == n
    sd = rt.subpath_draws(gpu_ctx, flat.dinfo_dev, n, nsub)
    dashes = np.zeros(n, U.capi.dash_dtype)
    dashes["count"], dashes["phase"] = len(pat), phase
    pattern = np.array(pat, dtype=f32)
    got = rt.dash(gpu_ctx, flat.poly_dev, flat.subs_dev, sd, nsub, torch.from_numpy(dashes.view(np.uint8).copy()).cuda(), n, torch.from_numpy(pattern).cuda(), len(pat))
    npieces = got.sizes["num_subpaths"]
    # the fixture condition (tests/test_dash_cpu.py checks it with the model): no piece the reference would drop a vertex of
    f0 = got.subpaths["first_vertex"].astype(np.int64)
    last = f0 + got.subpaths["num_vertices"].astype(np.int64) - 1
    assert np.all(got.subpaths["num_vertices"] >= 2)
    for a, b in ((got.poly[f0], got.poly[f0 + 1]), (got.poly[last - 1], got.poly[last])):
        dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
        dist = dx * dx + dy * dy
        print("%s: %d pieces, smallest end-segment distSqr %.3g" % (name, npieces, float(dist.min())))
        assert int((dist < f32(1e-5)).sum()) == 0
    mesh = rt.stroke(gpu_ctx, got.poly_dev, got.subs_dev, got.sub_draw_dev, npieces, dd, n)
    # the reference on the same pieces
    rd = d[got.sub_draw].copy()
    rd["path"] = np.arange(npieces, dtype=np.uint32)
    ref = oracle.tessellate(piece_pathset(vgr, got.poly, got.subpaths), rd)
    for k in ("num_meshes", "num_vertices", "num_indices"):
        assert mesh.sizes[k] == ref.sizes[k], (name, k, mesh.sizes[k], ref.sizes[k])
    assert mesh.sizes["num_meshes"] == npieces
    assert np.array_equal(mesh.meshes["num_vertices"], ref.meshes["num_vertices"]) and np.array_equal(mesh.meshes["num_indices"], ref.meshes["num_indices"])
    assert np.array_equal(mesh.meshes["first_vertex"], ref.meshes["first_vertex"]) and np.array_equal(mesh.meshes["first_index"], ref.meshes["first_index"])
    assert np.array_equal(mesh.idx, ref.idx), name
    assert np.array_equal(mesh.color, ref.color), name
    assert np.array_equal(mesh.pos.view(np.uint32), ref.pos.view(np.uint32)), name
    pset.close()


def test_full_size_random_walks(rt, gpu_ctx, wl):
    """random_walk_polylines() at its default size under [12,6]: totals exact, every source list's pieces by digest, against the host
    build of the lane code."""
    import torch
    n, nseg = 10000, 1000
    lists, closed = U.walks(wl, n, nseg)
    poly, subs = U.lists_to_arrays(lists, closed)
    del lists
    dashes, pattern = U.make_dashes([([12.0, 6.0], 0.0)])
    sub_draw = np.zeros(n, np.uint32)
    hst, z, hp, hs, hd, hsrc = U.host_dash(poly, subs, sub_draw, dashes, pattern)
    assert hst == 0
    got = run_dash(rt, gpu_ctx, poly, subs, sub_draw, dashes, pattern)
    nv, ns = z["num_poly_vertices"], z["num_subpaths"]
    assert got.sizes["num_poly_vertices"] == nv and got.sizes["num_subpaths"] == ns
    assert got.subpaths.tobytes() == hs.tobytes()
    assert np.array_equal(got.sub_src, hsrc) and np.array_equal(got.sub_draw, hd)
    # per source list: its pieces are one contiguous range of the output polyline
    counts = np.bincount(hsrc, weights=hs["num_vertices"].astype(np.float64), minlength=n).astype(np.int64)
    starts = np.cumsum(counts) - counts
    dg = H.digest_ragged_torch(got.poly_dev[:nv].view(torch.int32).reshape(-1), torch.from_numpy(2 * starts).cuda(), torch.from_numpy(2 * counts).cuda())
    dh = H.digest_ragged_np(hp.view(np.uint32).reshape(-1), 2 * starts, 2 * counts)
    assert np.array_equal(dg, dh), np.nonzero((dg != dh).any(axis=1))[0][:10]
