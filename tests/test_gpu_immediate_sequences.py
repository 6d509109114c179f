"""GPU: immediate mode under changing content, against the reference.

vgx_tessellate_immediate chooses its kernels from what the LAST call with the same tag -- (path set, number of draws) -- found: period,
distinct paths, polyline vertices, command instances, long sub-paths. A different draw list with the same tag is "known" and runs on
stale numbers; include/vgx.h promises that this is invisible. Here: every ordered pair of the batch kinds of immediate_kinds.py on one
context (a), sequences across path sets and entry points (b), the error kinds (c), calls without synchronisation (d), seeded random
walks (e) and the routing knobs (f). Every result is compared with oracle.tessellate bit for bit; guarded buffers, canaries checked
after every call; VGX_OK within three calls. tests/test_immediate_kinds_cpu.py holds the premises (what each kind is)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import immediate_kinds as K
from test_gpu_immediate import canaries_intact, guarded, immediate_loop, sizes_of, to_host
from util import assert_mesh_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = ("num_vertices", "num_indices", "num_meshes", "num_poly_vertices", "num_subpaths", "num_cmd_instances")


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


_draws_dev = {}
_ref_dev = {}


def draws_dev(rt, kind):
    if kind not in _draws_dev:
        _draws_dev[kind] = rt.upload_draws(K.make(kind)[1])
    return _draws_dev[kind]


def ref_dev(oracle, kind):
    """The reference's result of a kind, and its streams in device memory (computed once)."""
    import torch
    if kind not in _ref_dev:
        r = K.reference(oracle, kind)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).to("cuda:0")
        _ref_dev[kind] = (r, up(r.pos, np.int32), up(r.color, np.int32), up(r.idx, np.int16), up(r.meshes, np.uint8))
    return _ref_dev[kind]


def check_equal(rt, oracle, kind, bufs, sizes, what):
    """Totals and every output byte == oracle.tessellate (assert_mesh_equal's bar, pos_tol = 0; compared on the device, the host
    comparison names the first difference)."""
    import torch
    r, pos, color, idx, meshes = ref_dev(oracle, kind)
    for k in TOTALS:
        assert sizes[k] == r.sizes[k], (what, k, sizes, r.sizes)
    nv, ni, nm = r.sizes["num_vertices"], r.sizes["num_indices"], r.sizes["num_meshes"]
    same = (torch.equal(bufs.pos[:nv].view(torch.int32).reshape(-1), pos) and torch.equal(bufs.color[:nv], color)
            and torch.equal(bufs.idx[:ni], idx) and torch.equal(bufs.meshes[:nm * 32], meshes))
    if not same:
        assert_mesh_equal(to_host(rt, bufs, sizes), r, what)
        raise AssertionError("%s: output bytes differ from the reference" % (what,))


class Session:
    """One context, its path sets (made on demand, one per PathSetArrays) and the caller's output buffers, which only ever grow."""

    def __init__(self, rt, oracle):
        self.rt, self.oracle = rt, oracle
        self.ctx = rt.Context(0)
        self.psets = {}
        self.bufs = guarded(rt, "cuda:0", 1024, 1024, 64)

    def pset(self, kind):
        ps = K.make(kind)[0]
        if id(ps) not in self.psets:
            self.psets[id(ps)] = self.rt.PathSet(self.ctx, ps)
        return self.psets[id(ps)]

    def pset_of(self, key, ps):
        if key not in self.psets:
            self.psets[key] = self.rt.PathSet(self.ctx, ps)
        return self.psets[key]

    def close(self):
        for p in self.psets.values():
            p.close()
        self.ctx.close()


def run_step(S, kind, what=""):
    """One batch through the growth loop of test_gpu_immediate.immediate_loop (guarded buffers, canaries after every call, statuses
    limited to OK / GROWN / NOSPACE, at most three calls) with profiling on; the result must equal the reference.
    Returns (statuses, stage names of every call)."""
    rt = S.rt
    stages = []
    n = K.make(kind)[1].shape[0]
    S.ctx.set_profiling(True)
    try:
        statuses, seen, S.bufs = immediate_loop(rt, S.ctx, S.pset(kind), draws_dev(rt, kind), n, S.bufs,
                                                after_call=lambda st: stages.append([nm for nm, _ in S.ctx.stage_times()]))
    finally:
        S.ctx.set_profiling(False)
    check_equal(rt, S.oracle, kind, S.bufs, seen[-1], (what, kind, statuses))
    return statuses, stages


def route_of(stages):
    r = [s for s in stages if s.startswith("route_")]
    assert len(r) == 1, stages
    return r[0]


# ---- a. the transition matrix -------------------------------------------------------------------------------------------------
# Every ordered pair of the kinds on the shared path set, from the same-size kinds to the _big ones. The expected route of B's first
# call is K.first_call_route(A, B): the table K.LEARNED (checked against the host rules by test_immediate_kinds_cpu.py) where the tags
# collide -- the call then provably ran on A's knowledge --, route_build / route_frame where they do not. No cell is skipped; none is
# unobservable (no colliding kind learns route_build, which is what a new tag would show).
CELLS = sorted(((a, b) for a in K.SHARED for b in K.SHARED), key=lambda c: max(K.SHARED.index(c[0]), K.SHARED.index(c[1])))


def run_cell(rt, oracle, a, b):
    S = Session(rt, oracle)
    try:
        run_step(S, a, "A")
        statuses, stages = run_step(S, a, "A again")
        assert statuses == [0], (a, statuses)
        assert route_of(stages[0]) == K.LEARNED[a], (a, stages[0])
        statuses, stages = run_step(S, b, "B after %s" % a)
        assert route_of(stages[0]) == K.first_call_route(a, b), ("this cell no longer tests what it says", a, b, statuses, stages[0])
        statuses2, stages2 = run_step(S, b, "B again after %s" % a)
        assert statuses2 == [0], (a, b, statuses, statuses2)
        return statuses, stages, stages2
    finally:
        S.close()


@pytest.mark.parametrize("a,b", CELLS, ids=["%s->%s" % c for c in CELLS])
def test_transition(rt, oracle, a, b):
    run_cell(rt, oracle, a, b)


def test_matrix_holds_every_ordered_pair():
    assert len(CELLS) == len(set(CELLS)) == len(K.SHARED) ** 2 == 225
    assert set(K.SHARED) == set(K.PROPS) - set(K.OWN)


# ---- b. across path sets and entry points --------------------------------------------------------------------------------------
_tiger40 = {}


def foreign_count_emit(S, kind):
    rt = S.rt
    n = K.make(kind)[1].shape[0]
    res = rt.tessellate(S.ctx, S.pset(kind), draws_dev(rt, kind), n, to_host=False)
    check_equal(rt, S.oracle, kind, res.bufs, res.sizes, ("count + emit", kind))


def foreign_template(S, kind=None):
    """vgx_tessellate_count + vgx_tessellate of 40 tiger-like drawings: template mode armed on the context."""
    import torch
    rt = S.rt
    if not _tiger40:
        wl = importlib.import_module("vg-renderer_amd.workloads")
        ps, d = wl.tiger(40)
        _tiger40.update(ps=ps, d=d, dd=rt.upload_draws(d), ref=S.oracle.tessellate(ps, d))
    pset, dd, n, ref = S.pset_of("tiger40", _tiger40["ps"]), _tiger40["dd"], _tiger40["d"].shape[0], _tiger40["ref"]
    sizes = rt.tessellate_count(S.ctx, pset, dd, n)
    bufs = guarded(rt, dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_async(S.ctx, pset, dd, n, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == 0 and canaries_intact(bufs)
    assert S.ctx.failure_info()["segment_items"] == 5, "the periodic batch runs in template mode"
    assert_mesh_equal(to_host(rt, bufs, sizes), ref, "template tiger")


def foreign_flatten(S, kind):
    rt = S.rt
    n = K.make(kind)[1].shape[0]
    r = rt.flatten(S.ctx, S.pset(kind), draws_dev(rt, kind), n, to_host=False)  # (both flatten entry points, compared with each other)
    ref = K.reference(S.oracle, kind)
    for k in ("num_poly_vertices", "num_subpaths"):
        assert r.sizes[k] == ref.sizes[k], (kind, k)


def foreign_failed_count(S, kind=None):
    rt = S.rt
    with pytest.raises(rt.VgxError) as e:
        rt.tessellate_count(S.ctx, S.pset("nan_draw"), draws_dev(rt, "nan_draw"), K.NDRAWS)
    assert e.value.status == rt.capi.VGX_E_NONFINITE


def foreign_small_reserve(S, kind=None):
    before = S.ctx.scratch_bytes()
    S.ctx.reserve(16, dict(num_cmd_instances=64, num_poly_vertices=256, num_subpaths=16, num_meshes=16))
    assert S.ctx.scratch_bytes() >= before


FOREIGN = [foreign_count_emit, foreign_template, foreign_flatten, foreign_failed_count, foreign_small_reserve]

# scratch sized by thin's command instances, then cubics_long's vertices, then a frame-sized batch, and back; colliding kinds in between
SEQUENCES = {
    "forward": ["thin", "cubics_long", "frame2048", "periodic64", "cubics_short", "broken_last", "tiger10", "unique_big", "thin", "periodic64_small",
                "cubics_long", "unique", "tiger10", "shuffled64", "cubics_short", "periodic48"],
    "back": ["periodic48", "cubics_short", "shuffled64", "tiger10", "unique", "cubics_long", "periodic64_small", "thin", "unique_big", "tiger10",
             "broken_last", "cubics_short", "periodic64", "frame2048", "cubics_long", "thin"],
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_across_path_sets_and_entry_points(rt, oracle, name):
    seq = SEQUENCES[name]
    S = Session(rt, oracle)
    try:
        for i, kind in enumerate(seq):
            run_step(S, kind, "%s step %d" % (name, i))
            other = seq[(i + 5) % len(seq)]  # the foreign call works on another kind
            f = FOREIGN[(i + (0 if name == "forward" else 2)) % len(FOREIGN)]
            f(S, other)
            # the immediate step behind it: the same batch again (its tag known) or, every other time, the next kind of the sequence
            after = seq[(i + 1) % len(seq)] if i % 2 else kind
            run_step(S, after, "%s step %d after %s(%s)" % (name, i, f.__name__, other))
    finally:
        S.close()


@pytest.mark.parametrize("kind", ["periodic64", "frame2048", "cubics_long"])
def test_emit_after_immediate_needs_a_new_count(rt, oracle, kind):
    """include/vgx.h: the immediate call ends the _count / _emit pairing; an emit without a new count is VGX_E_INVALID_ARG and writes nothing."""
    import torch
    S = Session(rt, oracle)
    try:
        n = K.make(kind)[1].shape[0]
        pset, dd = S.pset(kind), draws_dev(rt, kind)
        sizes = rt.tessellate_count(S.ctx, pset, dd, n)
        run_step(S, kind)
        out = guarded(rt, dd.device, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
        out.pos.view(torch.int32)[:] = 0x11111111
        out.color[:] = 0x22222222
        out.idx[:] = 0x3333
        out.meshes[:] = 0x44
        with pytest.raises(rt.VgxError) as e:
            rt.tessellate_emit(S.ctx, pset, dd, n, out)
        assert e.value.status == rt.capi.VGX_E_INVALID_ARG
        torch.cuda.synchronize()
        assert bool((out.pos.view(torch.int32) == 0x11111111).all().item()) and bool((out.color == 0x22222222).all().item())
        assert bool((out.idx == 0x3333).all().item()) and bool((out.meshes == 0x44).all().item())
        # and a count makes the pair whole again
        rt.tessellate_count(S.ctx, pset, dd, n)
        rt.tessellate_emit(S.ctx, pset, dd, n, out)
        torch.cuda.synchronize()
        check_equal(rt, oracle, kind, out, sizes, ("emit after a new count", kind))
    finally:
        S.close()


# ---- c. nan_draw, empty, nothing ------------------------------------------------------------------------------------------------
def step_nan(S):
    """nan_draw ends with VGX_E_NONFINITE in dev_status (a scratch that has to grow first may say so before), nothing past a capacity."""
    rt = S.rt
    statuses = []
    for _ in range(3):
        rt.tessellate_immediate(S.ctx, S.pset("nan_draw"), draws_dev(rt, "nan_draw"), K.NDRAWS, S.bufs)
        statuses.append(int(S.bufs.dev_status.item()))
        assert canaries_intact(S.bufs), ("overrun (nan_draw)", statuses)
        if statuses[-1] == rt.capi.VGX_E_NONFINITE:
            return statuses
        assert statuses[-1] == rt.capi.VGX_E_GROWN, statuses
    raise AssertionError("nan_draw: no VGX_E_NONFINITE within three calls: %s" % statuses)


def step_empty(S):
    rt = S.rt
    rt.tessellate_immediate(S.ctx, S.pset("empty"), draws_dev(rt, "empty"), 0, S.bufs)
    st = int(S.bufs.dev_status.item())
    assert canaries_intact(S.bufs), "overrun (empty)"
    assert st == rt.capi.VGX_OK, st
    sz = sizes_of(rt, S.bufs)
    assert all(v == 0 for v in sz.values()), sz


def test_nan_draw_teaches_nothing(rt, oracle):
    S = Session(rt, oracle)
    try:
        step_nan(S)  # on a fresh context
        run_step(S, "periodic64", "after nan_draw (fresh)")
        statuses, stages = run_step(S, "periodic64")
        assert statuses == [0] and route_of(stages[0]) == "route_periodic"
        step_nan(S)  # same tag, known: the periodic route
        statuses, stages = run_step(S, "periodic64", "after nan_draw (known tag)")
        assert route_of(stages[0]) == "route_periodic", stages[0]  # the failed call did not replace what the context knew
        run_step(S, "unique")
        step_nan(S)  # ... on unique's knowledge
        run_step(S, "periodic64", "after unique, nan_draw")
    finally:
        S.close()


def test_empty_batch(rt, oracle):
    S = Session(rt, oracle)
    try:
        step_empty(S)  # fresh context
        run_step(S, "unique_big")
        step_empty(S)
        statuses, _ = run_step(S, "unique_big", "after empty")
        assert statuses == [0], statuses
        step_empty(S)
    finally:
        S.close()


def test_nothing_to_draw(rt, oracle):
    S = Session(rt, oracle)
    try:
        for _ in range(2):
            run_step(S, "nothing")  # (check_equal: zero output totals, the reference's flatten totals)
            sz = sizes_of(rt, S.bufs)
            assert sz["num_vertices"] == sz["num_indices"] == sz["num_meshes"] == 0
            assert sz["num_poly_vertices"] == K.reference(oracle, "periodic64").sizes["num_poly_vertices"] > 0
        run_step(S, "periodic64", "after nothing")
        run_step(S, "nothing", "after periodic64")
    finally:
        S.close()


# ---- d. no synchronisation between calls --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("periodic64", "broken_last", "unique"), ("unique_big", "periodic64_small", "shuffled64")], ids=lambda k: "-".join(k))
def test_back_to_back_without_synchronisation(rt, oracle, kinds):
    """Three colliding kinds enqueued back to back, no host read in between: the mirror may or may not have landed, both are legal. The
    context has run each of them before (twice round, so that its scratch holds all three whatever route they take)."""
    import torch
    S = Session(rt, oracle)
    try:
        for k in kinds + kinds:
            run_step(S, k, "warm-up")
        bufs = {}
        for k in kinds:
            r = K.reference(oracle, k).sizes
            bufs[k] = guarded(rt, "cuda:0", r["num_vertices"], r["num_indices"], r["num_meshes"])
        pset = S.pset(kinds[0])
        for k in kinds:
            rt.tessellate_immediate(S.ctx, pset, draws_dev(rt, k), K.NDRAWS, bufs[k])
        torch.cuda.synchronize()
        first = {k: int(bufs[k].dev_status.item()) for k in kinds}
        for k in kinds:
            assert canaries_intact(bufs[k]), ("overrun", k, first)
            assert first[k] in (rt.capi.VGX_OK, rt.capi.VGX_E_GROWN), (k, first)
            if first[k] == rt.capi.VGX_OK:
                check_equal(rt, oracle, k, bufs[k], sizes_of(rt, bufs[k]), ("back to back", k, first))
        for k in kinds:
            rt.tessellate_immediate(S.ctx, pset, draws_dev(rt, k), K.NDRAWS, bufs[k])
        torch.cuda.synchronize()
        second = {k: int(bufs[k].dev_status.item()) for k in kinds}
        for k in kinds:
            assert canaries_intact(bufs[k]), ("overrun", k, first, second)
            assert second[k] == rt.capi.VGX_OK, (first, second)
            check_equal(rt, oracle, k, bufs[k], sizes_of(rt, bufs[k]), ("back to back, again", k, first, second))
    finally:
        S.close()


# ---- e. seeded random walks --------------------------------------------------------------------------------------------------
# The number of walks: the largest one <= 64 whose wall time stays within that of the whole of tests/test_gpu_immediate.py on the same
# machine. Measured on one MI355X: test_gpu_immediate.py 8.2 s; 64 walks run on their own 8.3 s (2.4 s of it the first walk: imports and
# the references), about 0.09 s per further walk -> 60.
WALKS = 60
WALK_STEPS = 8


def random_walk(rt, oracle, seed, log=None):
    rs = np.random.RandomState(9000 + seed)
    S = Session(rt, oracle)
    done = []
    try:
        for i in range(WALK_STEPS):
            if rs.uniform() < 0.3:
                f = FOREIGN[int(rs.randint(len(FOREIGN)))]
                other = (K.SHARED + K.OWN)[int(rs.randint(len(K.SHARED + K.OWN)))]
                done.append("%s(%s)" % (f.__name__, other))
                f(S, other)
                continue
            kind = K.ALL[int(rs.randint(len(K.ALL)))]
            done.append(kind)
            if kind == "nan_draw":
                step_nan(S)
            elif kind == "empty":
                step_empty(S)
            else:
                run_step(S, kind, "walk %d: %s" % (seed, " ".join(done)))
    except BaseException:
        sys.stderr.write("walk %d so far: %s\n" % (seed, " ".join(done)))
        raise
    finally:
        S.close()
    return done


@pytest.mark.parametrize("seed", range(WALKS))
def test_random_walk(rt, oracle, seed):
    random_walk(rt, oracle, seed)


# ---- f. knobs (read once at vgx_create: a fresh process each) -----------------------------------------------------------------------
def _knob_chain(kinds, first_routes):
    """Child process: the kinds in turn on one context, each to VGX_OK and once more; first_routes: the route of each kind's first call
    (None: not asserted under this knob)."""
    rt = importlib.import_module("vg-renderer_amd.runtime")
    import pyoracle
    S = Session(rt, pyoracle)
    for kind, route in zip(kinds, first_routes):
        statuses, stages = run_step(S, kind, "knob chain")
        if route:
            assert route_of(stages[0]) == route, (kind, stages[0])
        statuses, _ = run_step(S, kind, "knob chain, again")
        assert statuses == [0], (kind, statuses)
    S.close()
    print("OK")


KNOBS = {
    # the one-walk route forced: every known call takes it, whatever the vertices per command
    "flat1_forced": (dict(VGX_TESS_FLAT1="2"), ["unique", "unique_big", "periodic64_small"], ["route_build", "route_one_walk", "route_one_walk"]),
    # no instanced flatten: the periodic kinds take the one-walk route of their long curves
    "no_inst": (dict(VGX_INST="0"), ["periodic64", "broken_last", "shuffled64"], ["route_build", "route_one_walk", "route_one_walk"]),
    # the tile kernel / k_stroke_long armed for batches of any size
    "big_emit": (dict(VGX_BIG_EMIT_MIN="0"), ["periodic64", "broken_last", "shuffled64"], ["route_build", "route_periodic", "route_periodic"]),
}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_knobs(knob):
    env, kinds, routes = KNOBS[knob]
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; import test_gpu_immediate_sequences as t; t._knob_chain(%r, %r)"
                        % ([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")], kinds, routes)],
                       env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
