"""GPU: the chunk step the three command-parallel flatten kernels share (csrc/vgx_chunk.h: decode, segmented bookkeeping, carries)
at the borders of its 64-command chunks. test_gpu_parity.py, test_gpu_flatten_onewalk.py and test_gpu_count_routes.py reach these
branches through random batches; the cases here are the smallest shapes that reach each one on purpose, every batch under 400
command instances, and each runs through all three kernels on the same batch, bit-exact against the CPU oracle:
  vgx_flatten_count + vgx_flatten_emit           k_flatten<EMIT, XFORM>   (stages flatten_count / flatten_emit)
  vgx_tessellate, frame-sized launches off       k_flatten_build          (stage flatten_build, flatten mode 0: not k_flatten_thin / _inst)
  vgx_flatten on a fresh context                 k_flat1                  (stage flatten_one_walk)
The cases pin behaviour: they pass on the library as it was before the chunk step moved into the header as well."""
import importlib

import numpy as np
import pytest

from util import assert_flat_equal, assert_mesh_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def _pm():
    return importlib.import_module("vg-renderer_amd.pathset")


def _cubic_path(b, k):
    """An ordinary path: a closed sub-path with a cubic (no path set here is lineTo-only: k_flatten_build, not k_flatten_thin)."""
    b.begin_path(); b.move_to(10.0 + k, 20.0); b.line_to(60.0 + k, 25.0); b.cubic_to(70.0 + k, 60.0, 30.0 + k, 80.0, 15.0 + k, 50.0); b.close(); b.end_path()


def _styled(d, wl, rt):
    wl.set_fill(d, slice(None), 0xFF336699, aa=True)
    wl.set_stroke(d, slice(None), 0xFF112233, 3.0, cap=rt.capi.CAP_BUTT, join=rt.capi.JOIN_MITER)
    d["mtx"][:, 4] = (np.arange(d.shape[0]) % 7).astype(np.float32) * 3.0
    d["mtx"][:, 5] = 1.5
    return d


def case_owner_search(wl, rt):
    """(a) 130 draws of one-command (MOVE_TO only) and empty paths in a row between two ordinary draws: more than 63 draws begin
    inside one chunk, the draw window cannot cover it, the lanes take the find_owner_u64 branch."""
    pm = _pm()
    b = pm.PathSetBuilder()
    _cubic_path(b, 0)
    b.begin_path(); b.move_to(3.0, 4.0); b.end_path()
    b.begin_path(); b.end_path()
    _cubic_path(b, 5)
    ps = b.arrays()
    d = pm.make_draws(132)
    d["path"] = [0] + [1 if i % 3 else 2 for i in range(130)] + [3]
    return ps, _styled(d, wl, rt)


def case_close_at_lane0(wl, rt):
    """(b) MOVE_TO + 127 LINE_TOs + CLOSE, the last LINE_TO back on the first point: the CLOSE is lane 0 of the third chunk, its
    sub-path's 128 vertices arrive as a carry, it pops the vertex of lane 63 of the chunk before (NEXT_IS_CLOSE there). A second
    sub-path behind it starts from zero."""
    pm = _pm()
    b = pm.PathSetBuilder()
    b.begin_path()
    b.move_to(100.0, 100.0)
    for i in range(126):
        a = 2.0 * np.pi * (i + 1) / 127.0
        b.line_to(100.0 + 80.0 * np.sin(a), 180.0 - 80.0 * np.cos(a))
    b.line_to(100.0, 100.0)
    b.close()
    b.move_to(5.0, 5.0); b.line_to(9.0, 5.0); b.line_to(9.0, 9.0)
    b.end_path()
    _cubic_path(b, 0)
    ps = b.arrays()
    d = pm.make_draws(2)
    d["path"] = [0, 1]
    return ps, _styled(d, wl, rt)


def case_draw_ends_at_lane63(wl, rt):
    """(c) a draw whose last command is lane 63 (10 + 54 commands in front of the border), the next draw begins at lane 0: nothing
    of the draw that ended reaches the next one."""
    pm = _pm()
    b = pm.PathSetBuilder()
    for n in (10, 54, 12):
        b.begin_path()
        b.move_to(1.0, 2.0)
        for i in range(n - 3):
            b.line_to(4.0 + 3.0 * i, 2.0 + (i % 5) * 7.0)
        b.quadratic_to(40.0, 90.0, 2.0, 60.0)
        b.close()
        b.end_path()
    ps = b.arrays()
    d = pm.make_draws(4)
    d["path"] = [0, 1, 2, 0]
    return ps, _styled(d, wl, rt)


def case_thin_beside_full(wl, rt):
    """(d) one cubic path, thin paths (MOVE_TO / LINE_TO / CLOSE only) and one empty path in one set: no static layout, so
    k_flatten_build reads 16-byte thin records beside 64-byte ones, in one chunk and across a border."""
    pm = _pm()
    b = pm.PathSetBuilder()
    _cubic_path(b, 0)
    b.begin_path(); b.move_to(0.0, 0.0); b.line_to(30.0, 0.0); b.line_to(30.0, 30.0); b.line_to(0.0, 0.0); b.close(); b.end_path()  # pops
    b.begin_path(); b.end_path()
    b.begin_path()
    b.move_to(50.0, 50.0)
    for i in range(70):
        b.line_to(52.0 + 2.0 * i, 50.0 + (i % 3) * 11.0)
    b.close()
    b.move_to(7.0, 7.0); b.line_to(8.0, 9.0)
    b.end_path()
    b.begin_path(); b.move_to(2.0, 2.0); b.line_to(20.0, 2.0); b.line_to(20.0, 12.0); b.end_path()
    ps = b.arrays()
    d = pm.make_draws(12)
    d["path"] = [1, 0, 4, 2, 3, 1, 0, 2, 4, 3, 1, 0]
    return ps, _styled(d, wl, rt)


def case_degenerate_across_border(wl, rt):
    """(e) one degenerate draw (a LINE_TO onto the current point, in the first chunk) that ends in the second chunk: the flag
    travels as a carry to the draw's last command, the draw goes to the serial list and the exact builder."""
    pm = _pm()
    b = pm.PathSetBuilder()
    _cubic_path(b, 0)
    b.begin_path()
    b.move_to(0.0, 0.0)
    for i in range(80):
        b.line_to(3.0 * (i + 1), (i % 4) * 5.0)
        if i == 20:
            b.line_to(3.0 * (i + 1), (i % 4) * 5.0)
    b.close()
    b.end_path()
    ps = b.arrays()
    d = pm.make_draws(3)
    d["path"] = [0, 1, 0]
    return ps, _styled(d, wl, rt)


def case_mesh_count_edges(wl, rt):
    """(f) a fill + stroke draw with a 2-vertex and a 3-vertex sub-path (and a lone MOVE_TO): a stroke mesh from 2 vertices, a
    fill mesh from 3."""
    pm = _pm()
    b = pm.PathSetBuilder()
    b.begin_path()
    b.move_to(0.0, 0.0); b.line_to(40.0, 0.0)
    b.move_to(0.0, 10.0); b.line_to(40.0, 10.0); b.line_to(40.0, 50.0)
    b.move_to(90.0, 90.0)
    b.end_path()
    _cubic_path(b, 0)
    ps = b.arrays()
    d = pm.make_draws(3)
    d["path"] = [0, 1, 0]
    return ps, _styled(d, wl, rt)


CASES = {"owner_search": case_owner_search, "close_at_lane0": case_close_at_lane0, "draw_ends_at_lane63": case_draw_ends_at_lane63,
         "thin_beside_full": case_thin_beside_full, "degenerate_across_border": case_degenerate_across_border, "mesh_count_edges": case_mesh_count_edges}
_made = {}


def batch(wl, rt, name):
    """(PathSetArrays, draws, flatten reference, tessellate reference) of a case. Made once, shared by the three routes."""
    if name not in _made:
        _made[name] = CASES[name](wl, rt)
    return _made[name]


_refs = {}


def reference(oracle, wl, rt, name, what):
    if (name, what) not in _refs:
        ps, d = batch(wl, rt, name)
        _refs[(name, what)] = oracle.tessellate(ps, d) if what == "mesh" else oracle.flatten(ps, d, apply_transform=what == "flat_xform")
    return _refs[(name, what)]


def _stages(ctx):
    return [n for n, _ in ctx.stage_times()]


@pytest.mark.parametrize("name", list(CASES))
def test_shapes_are_what_they_claim(wl, rt, name):
    """The batches against their own description (no GPU work): sizes, and where the border commands sit."""
    ps, d = batch(wl, rt, name)
    ncmd = np.diff(ps.path_cmd_begin)[d["path"]]
    prefix = np.concatenate([[0], np.cumsum(ncmd)])
    assert prefix[-1] < 400
    C = rt.capi
    if name == "owner_search":
        assert np.sum((prefix[:-1] >= 0) & (prefix[:-1] < 64)) > 63  # draws that begin inside the first chunk
    if name == "close_at_lane0":
        assert ps.cmd_type[128] == C.CMD_CLOSE and prefix[0] == 0 and ncmd[0] > 128
    if name == "draw_ends_at_lane63":
        assert prefix[2] == 64
    if name == "degenerate_across_border":
        assert prefix[1] < 64 < prefix[2]


@pytest.mark.parametrize("xform", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_two_pass_flatten(rt, wl, oracle, name, xform):
    ps, d = batch(wl, rt, name)
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    ctx.set_profiling(True)
    got = rt.flatten(ctx, pset, dd, d.shape[0], apply_transform=xform, entry="two_phase")
    stages = _stages(ctx)  # of vgx_flatten_emit, the last call
    ctx.set_profiling(False)
    pset.close(); ctx.close()
    assert "flatten_emit" in stages and "flatten_one_walk" not in stages
    assert_flat_equal(got, reference(oracle, wl, rt, name, "flat_xform" if xform else "flat"), "%s two-pass xform=%s" % (name, xform))


@pytest.mark.parametrize("xform", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_one_walk_flatten(rt, wl, oracle, name, xform):
    ps, d = batch(wl, rt, name)
    ref = reference(oracle, wl, rt, name, "flat_xform" if xform else "flat")
    ctx = rt.Context(0)  # fresh: the first vgx_flatten on a batch takes the one-walk kernel
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    ctx.set_profiling(True)
    got = rt.flatten_one_walk(ctx, pset, dd, d.shape[0], apply_transform=xform, cap_poly=ref.sizes["num_poly_vertices"], cap_subs=ref.sizes["num_subpaths"])
    stages = _stages(ctx)
    ctx.set_profiling(False)
    pset.close(); ctx.close()
    assert "flatten_one_walk" in stages and "flatten_emit" not in stages
    assert_flat_equal(got, ref, "%s one-walk xform=%s" % (name, xform))


@pytest.mark.parametrize("name", list(CASES))
def test_tessellate_build(rt, wl, oracle, monkeypatch, name):
    import torch
    monkeypatch.setenv("VGX_NO_SMALL", "1")  # read at vgx_create: the large-batch launch sequence, k_flatten_build on the ordinary route
    ps, d = batch(wl, rt, name)
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(ctx, pset, dd, d.shape[0])
    mode = ctx.failure_info()["segment_items"]
    bufs = rt.MeshBuffers(dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    bufs.pos.fill_(float("nan")); bufs.idx.fill_(-1)
    ctx.set_profiling(True)
    rt.tessellate_async(ctx, pset, dd, d.shape[0], bufs)
    torch.cuda.synchronize()
    stages = _stages(ctx)
    ctx.set_profiling(False)

    class G:
        pass
    got = G()
    nv, ni, nm = sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]
    got.sizes = sizes
    got.pos = bufs.pos[:nv].cpu().numpy()
    got.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
    got.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
    got.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(rt.capi.mesh_dtype)
    status = int(bufs.dev_status.item())
    pset.close(); ctx.close()
    assert status == 0
    assert mode == 0 and "flatten_build" in stages and "small_front" not in stages and "flatten_one_walk" not in stages
    assert_mesh_equal(got, reference(oracle, wl, rt, name, "mesh"), "%s vgx_tessellate" % name)
