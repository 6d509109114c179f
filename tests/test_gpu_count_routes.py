"""GPU: which stages an ordinary (non-template) batch launches through vgx_tessellate_count and the vgx_tessellate that follows --
the route rules of csrc/vgx_route_plan.h and the route state vgx_api.hip keeps between the two calls -- through public calls only.
One small batch per route: the recorded stage names and flatten mode, and the output against the reference oracle. One more case
for route state across calls: a one-walk route belongs to the path set it was sized for. And one for a vgx_tessellate that follows
immediate calls without a count: the one-walk choice of an immediate call is that call's own.

The recorded lists are what the library did BEFORE the route rules moved into vgx_route_plan.h (commit d26a47b), taken by running
`collect` / `collect_two_sets` / `collect_after_immediate` of this file on that build; they are not derived from the code under test."""
import numpy as np
import pytest

from util import assert_mesh_equal

pytestmark = pytest.mark.gpu

COUNT = ["scan_cmd_prefix", "flatten_count", "scan_draws", "flatten_emit", "mesh_prepare", "scan_meshes"]
TAIL = ["mesh_prepare", "scan_meshes", "fill_emit", "stroke_emit"]
BUILD = ["scan_cmd_prefix", "flatten_build", "scan_draws", "flatten_gather"] + TAIL  # (k_flatten_inst / k_flatten_thin run under the same name)
SORTED = ["scan_cmd_prefix", "inst_group", "flatten_build", "scan_draws", "flatten_gather"] + TAIL
ONE_WALK = ["scan_cmd_prefix", "flatten_one_walk", "flatten_gather"] + TAIL
# route -> (flatten mode of vgx_get_failure_info after the count, stages of vgx_tessellate_count, stages of vgx_tessellate)
PARENT = {
    "frame": (0, COUNT, ["small_front", "flatten_build", "small_middle", "fill_emit", "stroke_emit"]),
    "periodic": (1, COUNT, BUILD), "periodic_perm": (4, COUNT, SORTED),
    "grouped": (2, COUNT, SORTED), "grouped_classes": (3, COUNT, SORTED),
    "one_walk": (0, COUNT, ONE_WALK), "build": (0, COUNT, BUILD), "thin": (6, COUNT, BUILD),
}
PARENT_TWO_SETS = (BUILD, ONE_WALK)  # the second path set, the first one again
# the last immediate call (on its learned route), the vgx_tessellate that follows it without a count
PARENT_AFTER_IMMEDIATE = (["route_one_walk", "scan_cmd_prefix", "flatten_one_walk", "flatten_gather", "imm_size"] + TAIL, BUILD)
ROUTES = ["frame", "periodic", "periodic_perm", "grouped", "grouped_classes", "one_walk", "build", "thin"]
# knobs a route's context is made under (read at vgx_create): no template where one would take the batch
KNOBS = {"periodic": {"VGX_TMPL": "0"}, "periodic_perm": {"VGX_TMPL": "0"}, "grouped_classes": {"VGX_INST_PERM": "0"}}


@pytest.fixture(scope="module")
def rt():
    import importlib
    return importlib.import_module("vg-renderer_amd.runtime")


def _instances(wl, spread):
    """33 instances of a 64-path fuzz drawing (2112 draws) at ONE scale and tolerance, each under its own translation; `spread`: each
    instance at a scale of its own, over two decades."""
    ps = wl.fuzz_paths(4301, npaths=64, with_shapes=True)
    one = wl.fuzz_draws(ps, 4301)
    one["mtx"][:, :4] /= one["scale"][:, None]
    one["scale"] = 1.0
    one["tess_tol"] = 0.25
    d = np.tile(one, 33)
    inst = np.arange(d.shape[0]) // 64
    d["mtx"][:, 4] += (37.0 * (inst % 10)).astype(np.float32)
    d["mtx"][:, 5] += (41.0 * (inst // 10)).astype(np.float32)
    if spread:
        f = np.repeat((10.0 ** np.random.RandomState(4302).uniform(-1.0, 1.0, size=33)).astype(np.float32), 64)
        d["mtx"][:, :4] *= f[:, None]
        d["scale"] *= f
    return ps, d


def _cubics(wl, capi, f):
    """2049 draws of distinct one-cubic paths in a box of 1000 x f, stroked."""
    ps, d = wl.random_cubics(2049, seed=4303, box=1000.0)
    d = d.copy()
    d["fill_flags"] = 0
    d["stroke_flags"] = capi.stroke_flags(capi.CAP_BUTT, capi.JOIN_MITER)
    d["stroke_width"] = 2.0
    d["mtx"][:, :4] *= np.float32(f)
    d["scale"] *= np.float32(f)
    return ps, d


_batches = {}


def batch(rt, wl, route):
    """(PathSetArrays, draws) of a route: the smallest shape that still takes it. Made once."""
    if route in _batches:
        return _batches[route]
    if route == "frame":
        ps = wl.fuzz_paths(4300, npaths=64, with_shapes=True)
        r = ps, wl.fuzz_draws(ps, 4300, ndraws=2048)
    elif route in ("periodic", "periodic_perm"):
        r = _instances(wl, route == "periodic_perm")
    elif route in ("grouped", "grouped_classes"):
        ps, d = _instances(wl, route == "grouped_classes")
        r = ps, d[np.random.RandomState(4304).permutation(d.shape[0])]
    elif route == "one_walk":
        r = _cubics(wl, rt.capi, 1.0)
    elif route == "build":
        r = _cubics(wl, rt.capi, 0.04)
    else:
        assert route == "thin"
        ps = wl.thin_fuzz_paths(4305, npaths=2049)
        r = ps, wl.fuzz_draws(ps, 4305)
    _batches[route] = r
    return r


_refs = {}


def reference(oracle, rt, wl, route):
    if route not in _refs:
        _refs[route] = oracle.tessellate(*batch(rt, wl, route))
    return _refs[route]


class _G:
    pass


def step(rt, ctx, pset, dd, nd, sizes):
    """A profiled vgx_tessellate into buffers of the counted sizes."""
    import torch
    nv, ni, nm = (sizes[k] for k in ("num_vertices", "num_indices", "num_meshes"))
    bufs = rt.MeshBuffers(dd.device, nv, ni, nm)
    bufs.pos.fill_(float("nan")); bufs.idx.fill_(-1)
    ctx.set_profiling(True)
    rt.tessellate_async(ctx, pset, dd, nd, bufs)
    torch.cuda.synchronize()
    g = _G()
    g.stages = [n for n, _ in ctx.stage_times()]
    ctx.set_profiling(False)
    g.status = int(bufs.dev_status.item())
    g.sizes = sizes
    g.pos = bufs.pos[:nv].cpu().numpy()
    g.color = bufs.color[:nv].cpu().numpy().view(np.uint32)
    g.idx = bufs.idx[:ni].cpu().numpy().view(np.uint16)
    g.meshes = bufs.meshes[:nm * 32].cpu().numpy().view(rt.capi.mesh_dtype)
    return g


def count(rt, ctx, pset, dd, nd):
    """A profiled vgx_tessellate_count -> (sizes, stages, flatten mode)."""
    ctx.set_profiling(True)
    sizes = rt.tessellate_count(ctx, pset, dd, nd)
    stages = [n for n, _ in ctx.stage_times()]
    ctx.set_profiling(False)
    return sizes, stages, ctx.failure_info()["segment_items"]


def collect(rt, wl, route):
    """On a fresh context (the caller has set the route's knobs): the count, then one step."""
    ps, d = batch(rt, wl, route)
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes, count_stages, mode = count(rt, ctx, pset, dd, d.shape[0])
    g = step(rt, ctx, pset, dd, d.shape[0], sizes)
    g.record = (mode, count_stages, g.stages)
    pset.close()
    ctx.close()
    return g


def collect_two_sets(rt, wl):
    """A count on the one-walk batch, then vgx_tessellate on a SECOND path set (the same paths, made again) with the same draws, then
    on the first one again."""
    ps, d = batch(rt, wl, "one_walk")
    ctx = rt.Context(0)
    first, second = rt.PathSet(ctx, ps), rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes, _, _ = count(rt, ctx, first, dd, d.shape[0])
    b = step(rt, ctx, second, dd, d.shape[0], sizes)
    a = step(rt, ctx, first, dd, d.shape[0], sizes)
    second.close(); first.close()
    ctx.close()
    return b, a


def collect_after_immediate(rt, wl, sizes):
    """vgx_tessellate_immediate on the one-walk batch until it runs on what it learned (its route mark is the first stage), then
    vgx_tessellate on the same context, never counted. -> (stages of the last immediate call, the vgx_tessellate step)"""
    import torch
    ps, d = batch(rt, wl, "one_walk")
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    r, bufs = rt.tessellate_grow(ctx, pset, dd, d.shape[0], max_calls=4)
    ctx.set_profiling(True)
    rt.tessellate_immediate(ctx, pset, dd, d.shape[0], bufs)
    torch.cuda.synchronize()
    imm_stages = [n for n, _ in ctx.stage_times()]
    ctx.set_profiling(False)
    assert int(bufs.dev_status.item()) == 0
    g = step(rt, ctx, pset, dd, d.shape[0], sizes)
    pset.close()
    ctx.close()
    return imm_stages, g


@pytest.mark.parametrize("route", ROUTES)
def test_route_stages_and_output(rt, wl, oracle, monkeypatch, route):
    for k, v in KNOBS.get(route, {}).items():
        monkeypatch.setenv(k, v)
    got = collect(rt, wl, route)
    assert got.status == 0
    assert got.record == PARENT[route]
    assert_mesh_equal(got, reference(oracle, rt, wl, route), route)


def test_one_walk_route_belongs_to_its_path_set(rt, wl, oracle):
    other, again = collect_two_sets(rt, wl)
    assert (other.status, again.status) == (0, 0)
    assert (other.stages, again.stages) == PARENT_TWO_SETS
    ref = reference(oracle, rt, wl, "one_walk")
    assert_mesh_equal(other, ref, "second path set")
    assert_mesh_equal(again, ref, "first path set again")


def test_an_immediate_one_walk_choice_is_that_calls_own(rt, wl, oracle):
    ref = reference(oracle, rt, wl, "one_walk")
    imm_stages, after = collect_after_immediate(rt, wl, ref.sizes)
    assert imm_stages[0] == "route_one_walk" and after.status == 0
    assert (imm_stages, after.stages) == PARENT_AFTER_IMMEDIATE
    assert_mesh_equal(after, ref, "vgx_tessellate after immediate calls")
