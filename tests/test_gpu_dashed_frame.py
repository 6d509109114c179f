"""GPU: vgx_tessellate_dashed / vgx_reserve_dashed / vgx_stroke (csrc/vgx_dashframe.hip, csrc/vgx_api.hip). Everything is compared exactly:
every field of every vgx_mesh, idx, color, pos as bit patterns, dev_sizes and dev_dash_sizes.
  1. frames against the reference model (tests/dashed_frame_model.py): fuzz seeds 100-103;
  2. fills with dashes: the 200 closed circles, against the model;
  3. zero and many pieces in one batch, against the model;
  4. route independence: 2 048 / 2 049 / 2 100 draws against the composition of the older entries, twice on one context;
  5. no dashes: dashes = None and all-zero records equal tessellate_immediate byte for byte;
  6. the status protocol: convergence within four calls, sentinels, exact NOSPACE totals, reserve_dashed, bad records, counted state;
  7. draw-command assembly against vgx_merge of the composition under the same armed assembly;
  8. vgx_stroke against vgx_stroke_count + vgx_stroke_emit."""
import importlib

import numpy as np
import pytest

import dash_util as U
import dashed_frame_fixtures as F
import dashed_frame_gpu as G
import dashed_frame_model as DM
import hashutil as H

pytestmark = pytest.mark.gpu
capi = U.capi
f32 = np.float32


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def check_sizes(got, want_sizes, want_dash, what):
    for k in DM.TOTALS:
        assert got.sizes[k] == want_sizes[k], (what, k, got.sizes, want_sizes)
    assert got.dash_sizes == want_dash, (what, got.dash_sizes, want_dash)


def against_model(rt, ctx, oracle, fixture):
    name, ps, d, dashes, pattern = fixture
    want = DM.frame(oracle, ps, d, dashes, pattern)
    pset = rt.PathSet(ctx, ps)
    got = G.dashed(rt, ctx, pset, rt.upload_draws(d), d.shape[0], dashes, pattern)
    check_sizes(got, want.sizes, want.dash_sizes, name)
    DM.assert_frame_equal(got, want, name)
    pset.close()
    return got, want


@pytest.mark.parametrize("seed", F.FUZZ_SEEDS)
def test_frame_equals_the_reference_model(rt, gpu_ctx, oracle, wl, seed):
    got, want = against_model(rt, gpu_ctx, oracle, F.fuzz(wl, seed))
    assert want.dash_sizes["num_subpaths"] > 500 and got.sizes["num_serial_draws"] > 0  # (the exact builder's draws are in the frame)


def test_fills_with_dashes(rt, gpu_ctx, oracle, wl, vgr):
    got, want = against_model(rt, gpu_ctx, oracle, F.circles(wl, vgr))
    kinds = got.meshes["subpath_kind"] >> 28
    assert int((kinds == capi.MESH_FILL_AA).sum()) == 200 and int((kinds >= capi.MESH_STROKE).sum()) == want.dash_sizes["num_subpaths"]


def test_zero_and_many(rt, gpu_ctx, oracle, wl, vgr):
    got, want = against_model(rt, gpu_ctx, oracle, F.zero_and_many(wl, vgr))
    per_draw = np.bincount(got.meshes["draw"][(got.meshes["subpath_kind"] >> 28) >= capi.MESH_STROKE], minlength=len(F.ZERO_AND_MANY))
    k = {name: i for i, name in enumerate(F.ZERO_AND_MANY)}
    assert per_draw[k["no on length"]] == 0 and per_draw[k["one-vertex sub-paths"]] == 0 and per_draw[k["stroke off"]] == 0 and per_draw[k["neither op"]] == 0
    assert per_draw[k["many pieces"]] > 4096


@pytest.mark.parametrize("ndraws", [2048, 2049, 2100])
def test_route_independence(rt, wl, ndraws):
    """Against the composition, whose immediate call takes the frame-sized route at 2 048 draws and k_flatten_build beyond (and another
    route on a second call); the frame call twice on one context: the bytes are equal."""
    ps = wl.fuzz_paths(100, npaths=48)
    d = wl.fuzz_draws(ps, 100, ndraws=ndraws)
    dashes, pattern = U.make_dashes(U.random_dash_entries(np.random.default_rng(100), ndraws))
    ctx, ctx2 = rt.Context(0), rt.Context(0)
    pset, pset2 = rt.PathSet(ctx, ps), rt.PathSet(ctx2, ps)
    want = G.compose(rt, ctx2, pset2, d, dashes, pattern)
    dd = rt.upload_draws(d)
    first = G.dashed(rt, ctx, pset, dd, ndraws, dashes, pattern)
    assert first.dash_sizes["num_subpaths"] == want.dash_sizes[0] and first.dash_sizes["num_poly_vertices"] == want.dash_sizes[1]
    for k in ("num_poly_vertices", "num_subpaths", "num_cmd_instances"):
        assert first.sizes[k] == want.flat_sizes[k], k
    DM.assert_frame_equal(first, want, "%d draws" % ndraws)
    second = G.dashed(rt, ctx, pset, dd, ndraws, dashes, pattern, bufs=first.bufs)
    assert second.statuses == [0] and second.sizes == first.sizes and second.dash_sizes == first.dash_sizes
    DM.assert_frame_equal(second, want, "%d draws, second call" % ndraws)
    # by digests per draw as well: the streams of every draw, whole
    nv = np.bincount(want.meshes["draw"], weights=want.meshes["num_vertices"].astype(np.float64), minlength=ndraws).astype(np.int64)
    v0 = np.cumsum(nv) - nv
    assert np.array_equal(H.digest_ragged_np(second.pos.view(np.uint32).reshape(-1), 2 * v0, 2 * nv), H.digest_ragged_np(want.pos.view(np.uint32).reshape(-1), 2 * v0, 2 * nv))
    pset.close(); pset2.close(); ctx.close(); ctx2.close()


@pytest.mark.parametrize("ndraws", [48, 2100])
def test_no_dashes_equals_immediate(rt, wl, ndraws):
    import torch
    ps = wl.fuzz_paths(101, npaths=48)
    d = wl.fuzz_draws(ps, 101, ndraws=ndraws)
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    res, bufs = rt.tessellate_grow(ctx, pset, dd, ndraws, max_calls=4)
    want = G.read(bufs, res.sizes)
    for dashes in (None, DM.no_dashes(ndraws)):
        ctx2 = rt.Context(0)
        pset2 = rt.PathSet(ctx2, ps)
        got = G.dashed(rt, ctx2, pset2, dd, ndraws, dashes, np.array([4.0, 2.0], f32))
        for k in DM.TOTALS:
            assert got.sizes[k] == res.sizes[k], (k, got.sizes, res.sizes)
        assert all(v == 0 for v in got.dash_sizes.values())
        assert got.meshes.tobytes() == want.meshes.tobytes() and got.idx.tobytes() == want.idx.tobytes()
        assert got.color.tobytes() == want.color.tobytes() and got.pos.tobytes() == want.pos.tobytes()
        pset2.close(); ctx2.close()
    pset.close(); ctx.close()


SENT_F, SENT_I, SENT_B = -77.0, 0x5A5A, 0x5A


def fill_sentinel(bufs):
    bufs.pos.fill_(SENT_F); bufs.color.fill_(0x5A5A5A5A); bufs.idx.fill_(SENT_I); bufs.meshes.fill_(SENT_B)


def sentinel_intact(bufs, nv=0, ni=0, nm=0):
    return (bool((bufs.pos[nv:] == SENT_F).all()) and bool((bufs.color[nv:] == 0x5A5A5A5A).all()) and bool((bufs.idx[ni:] == SENT_I).all())
            and bool((bufs.meshes[nm * 32:] == SENT_B).all()))


def guarded(rt, cap, guard=256):
    """Buffers with `guard` more elements than the stated capacity: the words behind it are the guard."""
    b = rt.MeshBuffers("cuda", cap[0] + guard, cap[1] + guard, cap[2] + guard)
    b.cap = tuple(int(c) for c in cap)
    fill_sentinel(b)
    return b


def test_protocol(rt, wl):
    import torch
    _, ps, d, dashes, pattern = F.fuzz(wl, 102)
    n = d.shape[0]
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd, ddash, dpat = rt.upload_draws(d), G.upload(dashes), G.upload(pattern)
    dds = torch.zeros(10, dtype=torch.int64, device="cuda")
    bufs = guarded(rt, (1024, 1024, 64))
    trail, nospace = [], None
    for _ in range(4):
        rt.tessellate_dashed_async(ctx, pset, dd, n, ddash, dpat, len(pattern), bufs, dds)
        st = int(bufs.dev_status.item())
        trail.append(st)
        z = G.sizes_of(bufs.dev_sizes)
        if st == capi.VGX_E_GROWN:
            assert sentinel_intact(bufs), trail  # nothing anywhere in the caller's buffers
            assert z["num_vertices"] == 0 and z["num_indices"] == 0
        elif st == capi.VGX_E_NOSPACE:
            assert sentinel_intact(bufs, *bufs.cap), trail  # nothing past a capacity
            nospace = z
            bufs = guarded(rt, (z["num_vertices"], z["num_indices"], z["num_meshes"]))
        else:
            break
    print("fresh context:", trail)
    assert trail[-1] == capi.VGX_OK and capi.VGX_E_NOSPACE in trail and capi.VGX_E_GROWN in trail, trail
    final, final_dash = G.sizes_of(bufs.dev_sizes), G.sizes_of(dds)
    for k in ("num_vertices", "num_indices", "num_meshes"):
        assert nospace[k] == final[k], (k, nospace, final)
    assert sentinel_intact(bufs, *bufs.cap)
    want = G.read(bufs, final)
    # after the call the counted state is gone: emit without a new count is refused
    with pytest.raises(rt.VgxError):
        rt.tessellate_emit(ctx, pset, dd, n, bufs)
    # halved capacities, one at a time and all together: VGX_E_NOSPACE, exact totals, nothing past a capacity
    nv, ni, nm = final["num_vertices"], final["num_indices"], final["num_meshes"]
    for cap in ((nv // 2, ni, nm), (nv, ni // 2, nm), (nv, ni, nm // 2), (nv // 2, ni // 2, nm // 2), (nv - 1, ni, nm)):
        b = guarded(rt, cap)
        rt.tessellate_dashed_async(ctx, pset, dd, n, ddash, dpat, len(pattern), b, dds)
        assert int(b.dev_status.item()) == capi.VGX_E_NOSPACE, cap
        z = G.sizes_of(b.dev_sizes)
        assert (z["num_vertices"], z["num_indices"], z["num_meshes"]) == (nv, ni, nm), (cap, z)
        assert sentinel_intact(b, *b.cap), cap
    # a fresh context after reserve_dashed with the final totals: one call, the same bytes
    ctx2 = rt.Context(0)
    pset2 = rt.PathSet(ctx2, ps)
    ctx2.reserve_dashed(n, final, final_dash)
    b = guarded(rt, (nv, ni, nm))
    rt.tessellate_dashed_async(ctx2, pset2, dd, n, ddash, dpat, len(pattern), b, dds)
    assert int(b.dev_status.item()) == capi.VGX_OK
    assert G.sizes_of(b.dev_sizes) == final and G.sizes_of(dds) == final_dash
    DM.assert_frame_equal(G.read(b, final), want, "after reserve_dashed")
    pset2.close(); ctx2.close(); pset.close(); ctx.close()


@pytest.mark.parametrize("what", ["odd count", "nan entry", "first + count > npattern", "cap code 3"])
def test_bad_records_write_nothing(rt, gpu_ctx, wl, what):
    _, ps, d, dashes, pattern = F.fuzz(wl, 103)
    d, dashes, pattern = d.copy(), dashes.copy(), pattern.copy()
    k = int(np.flatnonzero(dashes["count"] > 0)[3])
    if what == "odd count":
        dashes["count"][k] = 3
    elif what == "nan entry":
        pattern[int(dashes["first"][k])] = np.nan
    elif what == "first + count > npattern":
        dashes["first"][k] = len(pattern) - 1
    else:
        s = int(np.flatnonzero(d["stroke_flags"] & 1)[2])
        d["stroke_flags"][s] |= 3 << 4
    if what != "cap code 3":
        assert rt.dash_validate(dashes, pattern) == capi.VGX_E_INVALID_ARG
    pset = rt.PathSet(gpu_ctx, ps)
    dd = rt.upload_draws(d)
    bufs = guarded(rt, (1 << 20, 1 << 21, 1 << 15))
    for _ in range(3):  # (a VGX_E_GROWN of the scratch may come first; the verdict must not be VGX_OK and nothing may be written)
        rt.tessellate_dashed_async(gpu_ctx, pset, dd, d.shape[0], G.upload(dashes), G.upload(pattern), len(pattern), bufs)
        st = int(bufs.dev_status.item())
        assert sentinel_intact(bufs), (what, st)
        if st != capi.VGX_E_GROWN:
            break
    assert st == capi.VGX_E_INVALID_ARG, (what, st)
    pset.close()


@pytest.mark.parametrize("max_vb", [512, 2048])
def test_assembly(rt, wl, max_vb):
    """Seed 100 with max_vb_vertices 512, VGX_ASM_SPLIT_STATE and a UV stream against vgx_merge of the composition under the same armed
    assembly. The frame of seed 100 holds four meshes of more than 512 vertices (the largest: 1 222), so at 512 the merge of the
    composition ends with VGX_E_MESH_TOO_LARGE and so must the frame call: the verdicts are compared. At 2 048 both fit: the
    draw-command table, the rebased indices and the UVs are compared."""
    import torch
    _, ps, d, dashes, pattern = F.fuzz(wl, 100)
    d = d.copy()
    d["state_key"] = (np.arange(d.shape[0]) // 5).astype(np.uint32)
    n = d.shape[0]
    white = (0x12345678, 0)

    def run(ctx, fn):
        cmds = torch.zeros(8192 * 48, dtype=torch.uint8, device="cuda")
        num = torch.zeros(1, dtype=torch.int64, device="cuda")
        uv = torch.full((1 << 20, 2), -3, dtype=torch.int16, device="cuda")

        def arm(on):
            if on:
                ctx.set_assembly(cmds, max_vb_vertices=max_vb, dev_num=num, split_state=True, uv=uv, uv_value=white)
            else:
                ctx.set_assembly(None)
        g = fn(arm)
        torch.cuda.synchronize()
        if g.status != 0:
            return g, None, None
        k = int(num.item())
        return g, cmds[:k * 48].cpu().numpy().view(capi.drawcmd_dtype), uv[:g.pos.shape[0]].cpu().numpy()

    ctx, ctx2 = rt.Context(0), rt.Context(0)
    pset, pset2 = rt.PathSet(ctx, ps), rt.PathSet(ctx2, ps)
    want, wcmds, wuv = run(ctx2, lambda arm: G.compose(rt, ctx2, pset2, d, dashes, pattern, assembly=arm))

    def frame(arm):
        arm(True)
        try:
            g = G.dashed(rt, ctx, pset, rt.upload_draws(d), n, dashes, pattern, max_calls=5)
            g.status = 0
        except rt.VgxError as e:
            g = G.Got()
            g.status = e.status
        arm(False)
        return g
    got, gcmds, guv = run(ctx, frame)
    print("max_vb %d: merge of the composition -> %d, frame call -> %d" % (max_vb, want.status, got.status))
    assert got.status == want.status
    assert want.status == (capi.VGX_E_MESH_TOO_LARGE if max_vb == 512 else capi.VGX_OK)
    if want.status == 0:
        assert gcmds.shape[0] == wcmds.shape[0] and gcmds.shape[0] > 8 and got.sizes["num_drawcmds"] == gcmds.shape[0]
        assert gcmds.tobytes() == wcmds.tobytes()
        DM.assert_frame_equal(got, want, "assembly")  # (idx: rebased by the vertices in front of each mesh inside its vertex buffer)
        assert guv.tobytes() == wuv.tobytes()
    pset.close(); pset2.close(); ctx.close(); ctx2.close()


def test_stroke_single_call(rt, gpu_ctx, wl):
    """The "walks [5,3,1,3]" pieces with the style sweep: bytes and mesh table equal stroke_count + stroke_emit; halved capacities give
    VGX_E_NOSPACE with exact totals and nothing past a capacity."""
    import torch
    name, lists, closed, pat, phase = U.gpu_fixture_families(wl)[1]
    n = len(lists)
    d = F.styled_draws(wl, n, False)
    poly, subs = U.lists_to_arrays(lists, closed)
    dashes = np.zeros(n, capi.dash_dtype)
    dashes["count"], dashes["phase"] = len(pat), phase
    dd = rt.upload_draws(d)
    pcs = rt.dash(gpu_ctx, torch.from_numpy(poly).cuda(), G.upload(subs), torch.arange(n, dtype=torch.int32, device="cuda"), n, G.upload(dashes), n,
                  torch.tensor(pat, dtype=torch.float32, device="cuda"), len(pat))
    npieces = pcs.sizes["num_subpaths"]
    want = rt.stroke(gpu_ctx, pcs.poly_dev, pcs.subs_dev, pcs.sub_draw_dev, npieces, dd, n)
    nv, ni, nm = want.sizes["num_vertices"], want.sizes["num_indices"], want.sizes["num_meshes"]
    assert nm == npieces and npieces > 2000
    b = guarded(rt, (nv, ni, nm))
    rt.stroke_async(gpu_ctx, pcs.poly_dev, pcs.subs_dev, pcs.sub_draw_dev, npieces, dd, n, b)
    assert int(b.dev_status.item()) == capi.VGX_OK
    z = G.sizes_of(b.dev_sizes)
    for k in ("num_vertices", "num_indices", "num_meshes", "num_poly_vertices", "num_subpaths"):
        assert z[k] == want.sizes[k], (k, z, want.sizes)
    got = G.read(b, z)
    assert got.meshes.tobytes() == want.meshes.tobytes() and got.idx.tobytes() == want.idx.tobytes()
    assert got.color.tobytes() == want.color.tobytes() and got.pos.tobytes() == want.pos.tobytes()
    assert sentinel_intact(b, nv, ni, nm)
    for cap in ((nv // 2, ni, nm), (nv, ni // 2, nm), (nv, ni, nm // 2), (nv // 2, ni // 2, nm // 2)):
        b = guarded(rt, cap)
        rt.stroke_async(gpu_ctx, pcs.poly_dev, pcs.subs_dev, pcs.sub_draw_dev, npieces, dd, n, b)
        assert int(b.dev_status.item()) == capi.VGX_E_NOSPACE, cap
        z = G.sizes_of(b.dev_sizes)
        assert (z["num_vertices"], z["num_indices"], z["num_meshes"]) == (nv, ni, nm), (cap, z)
        assert sentinel_intact(b, *b.cap), cap
    with pytest.raises(rt.VgxError):  # the single call ends the counted state
        out = b.out_struct()
        rt._check(rt.lib().vgx_stroke_emit(gpu_ctx.handle, pcs.poly_dev.data_ptr(), pcs.subs_dev.data_ptr(), pcs.sub_draw_dev.data_ptr(), npieces, dd.data_ptr(), n,
                                           rt.C.byref(out), None), "vgx_stroke_emit")
