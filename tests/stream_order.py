"""The "sandwich": every entry of include/vgx.h that takes a `void* stream`, driven from a NON-BLOCKING side stream S behind a delay while
the null stream idles. Not collected by pytest (tests/test_gpu_stream_order.py runs the rows of CASES on the device,
tests/test_stream_order_table_cpu.py keeps the table complete and runs the decoys' admissibility checks on the CPU). torch is imported
lazily: the module imports without a device.

One row = one entry on one fresh Context, three calls:
  1. the entry on the real inputs A, stream NULL, synchronised                      -> ref
  2. the entry on a decoy A' (valid inputs of the same structure), NULL, synchronised -> decoy_ans, which must differ from ref
  3. the input buffers hold A', the outputs a pattern; then on S, nothing on the host waiting:
         delay kernel | copies of A over the inputs | the entry with stream = S | copies of the outputs aside | copies of A' back
     S.synchronize(); every output byte must equal ref, the bytes behind a capacity must still hold the pattern.
A launch, memset or copy of the entry that lands on another stream runs during the delay and sees A' (or the scratch call 2 left);
work deferred behind the call's place in S sees A' again; a size read back after synchronising another stream is call 2's.
Entries the header classes as asynchronous must also return while the delay still runs (S.query() is False right after the call).

A decoy is never garbage: a stream bug must show as a failed comparison, not as a wild read. The draw-reading families keep every
count and offset of A (asserted on the CPU oracle, structure_checks()); the others move positions, queries, transforms, lists."""
import ctypes as C
import functools
import importlib
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgx.h")
F = np.float32
FILL = 0xA5                      # the byte every output holds before a call
DELAY_MS, DELAY_MAX_MS = 50.0, 250.0
ASYNC, HOST = "asynchronous", "returns data to the host"
GENERAL = "Calls are asynchronous"   # the header's convention, for the entries that say nothing of their own

EXCLUDED = {
    "vgx_gather_sizes": "needs a communicator; tests/native/gather_test.cpp runs it on created streams",
    "vgx_gather": "needs a communicator; tests/native/gather_test.cpp runs it on created streams",
    "vgx_gather_at": "needs a communicator; tests/native/gather_test.cpp runs it on created streams",
}

TIMINGS = []   # (row, host ms from the first enqueue of the sandwich to the entry's return, calibrated delay ms)


# ---- the header -------------------------------------------------------------------------------------------------------------------------
def header_text():
    with open(HEADER) as f:
        return f.read()


def stream_entries(text=None):
    """The names of the prototypes of include/vgx.h that have a `void* stream` parameter."""
    import re
    text = header_text() if text is None else text
    return set(m.group(1) for m in re.finditer(r"^int\s+(vgx_\w+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S) if re.search(r"void\s*\*\s*stream\b", m.group(2)))


# ---- environment ------------------------------------------------------------------------------------------------------------------------
class Env:
    """What the rows need: the runtime, torch, the workloads and the CPU oracle."""

    def __init__(self):
        import torch
        self.torch = torch
        self.rt = importlib.import_module("vg-renderer_amd.runtime")
        self.wl = importlib.import_module("vg-renderer_amd.workloads")
        self.capi = self.rt.capi
        import pyoracle
        self.oracle = pyoracle
        self.lib = self.rt.lib()


def _hip():
    """The HIP runtime torch already loaded (the mapped file, not another copy found by name)."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped: import torch first")


HIP_STREAM_NON_BLOCKING = 1


def side_stream(torch):
    """A stream whose hipStreamGetFlags says hipStreamNonBlocking: torch's own when it is one, else created with flags and wrapped."""
    hip = _hip()
    hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]

    def flags(s):
        f = C.c_uint(0xFFFF)
        assert hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(f)) == 0
        return f.value
    s = torch.cuda.Stream()
    if flags(s) != HIP_STREAM_NON_BLOCKING:
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING) == 0
        s = torch.cuda.ExternalStream(h.value)
    assert flags(s) == HIP_STREAM_NON_BLOCKING, flags(s)
    assert s.cuda_stream != 0
    return s


_delay = {}


def delay_cycles(torch):
    """(cycles, ms): the torch.cuda._sleep count for DELAY_MS, timed once with a pair of events, and the time that count took."""
    if not _delay:
        probe = 20_000_000
        torch.cuda._sleep(probe)  # warm
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        torch.cuda.synchronize()
        per_ms = probe / max(a.elapsed_time(b), 1e-3)
        cycles = int(per_ms * DELAY_MS)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert 0.5 * DELAY_MS <= ms <= DELAY_MAX_MS, ("the delay kernel does not take what its calibration says", ms)
        _delay["v"] = (cycles, ms)
    return _delay["v"]


# ---- a row's plan -------------------------------------------------------------------------------------------------------------------------
def _raw(t):
    """A contiguous tensor as its bytes."""
    import torch
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


def to_dev(a):
    """numpy -> uint8 device tensor (a copy; an empty array gives 16 zero bytes so that it has an address)."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(16, dtype=np.uint8)).to("cuda:0")


class Plan:
    """What a row's make(env, ctx) returns. inputs: (live bytes, staging A, staging A'); outputs: (tensor, fill byte or None, used bytes
    or None); status: int32 tensors that must hold VGX_OK after every call; call(): the entry on torch's CURRENT stream, returns None or
    a tuple of host values; pre(): a plain call that must precede `call` with the same inputs loaded (the count before an emit), its
    return value must be the same for A and A'."""

    def __init__(self):
        self.inputs, self.outputs, self.status, self.keep, self.closers = [], [], [], [], []
        self.call = self.pre = None

    def inp(self, live, a, d):
        """live: the contiguous device tensor the entry reads; a / d: numpy arrays of its real and decoy contents (the same size)."""
        lv = _raw(live)
        sa, sd = to_dev(a), to_dev(d)
        assert sa.numel() == sd.numel() and sa.numel() <= lv.numel(), (sa.numel(), sd.numel(), lv.numel())
        self.inputs.append((lv[:sa.numel()], sa, sd))
        return live

    def new_inp(self, a, d):
        """A fresh uint8 device tensor for an input; returns it."""
        return self.inp(to_dev(a), a, d)

    def out(self, t, fill=FILL, used=None):
        assert t.is_contiguous()
        self.outputs.append((t, fill, used))
        return t


def mesh_out(p, env, nv, ni, nm, guard=64):
    """MeshBuffers of capacity (nv, ni, nm) with `guard` elements behind every capacity, registered as outputs of the plan."""
    b = env.rt.MeshBuffers("cuda:0", nv + guard, ni + guard, nm + guard)
    b.cap = (int(nv), int(ni), int(nm))
    p.out(b.pos, used=nv * 8), p.out(b.color, used=nv * 4), p.out(b.idx, used=ni * 2), p.out(b.meshes, used=nm * 32)
    p.out(b.dev_sizes), p.out(b.dev_status)
    p.status.append(b.dev_status)
    return b


def status_word(p, env):
    t = env.torch.zeros(1, dtype=env.torch.int32, device="cuda:0")
    p.out(t)
    p.status.append(t)
    return t


# ---- the sandwich -------------------------------------------------------------------------------------------------------------------------
def _load(plan, which):
    for live, sa, sd in plan.inputs:
        live.copy_(sa if which == "A" else sd)


def _fill(plan):
    for t, fill, _ in plan.outputs:
        if fill is not None:
            _raw(t).fill_(fill)


def _snap(plan, snaps):
    for (t, _, _), s in zip(plan.outputs, snaps):
        s.copy_(t)


def _same(torch, a, b):
    return all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def _first_difference(torch, plan, got, want):
    for k, (x, y) in enumerate(zip(got, want)):
        xb, yb = x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)
        if not torch.equal(xb, yb):
            w = torch.nonzero(xb != yb).reshape(-1)
            return {"output": k, "bytes": int(xb.numel()), "differ": int(w.numel()), "first": int(w[0].item())}
    return None


def _check_status(env, plan, what):
    for t in plan.status:
        st = int(t.reshape(-1)[0].item())
        assert st == env.capi.VGX_OK, (what, "dev_status", st)


def _guards(torch, plan, snaps, what):
    for (t, fill, used), s in zip(plan.outputs, snaps):
        if fill is not None and used is not None:
            tail = s.reshape(-1).view(torch.uint8)[int(used):]
            assert bool((tail == fill).all()), (what, "written behind a capacity", int(used))


def run_row(row, env, stream):
    """The three calls of one row. Raises on any difference; appends the row's timing to TIMINGS."""
    torch, rt = env.torch, env.rt
    assert torch.cuda.current_stream().cuda_stream == 0, "the tests run on the null stream"
    cycles, delay_ms = delay_cycles(torch)
    ctx = rt.Context(0)
    plan = None
    try:
        plan = row.make(env, ctx)
        snaps = [torch.empty_like(t) for t, _, _ in plan.outputs]
        torch.cuda.synchronize()

        def plain(which):
            _load(plan, which)
            torch.cuda.synchronize()
            pre = plan.pre() if plan.pre else None
            torch.cuda.synchronize()
            _fill(plan)
            torch.cuda.synchronize()
            ret = plan.call()
            _snap(plan, snaps)
            torch.cuda.synchronize()
            if row.check_status:
                _check_status(env, plan, (row.name, which))
            _guards(torch, plan, snaps, (row.name, which))
            return ret, [s.clone() for s in snaps], pre

        ref_ret, ref, pre_a = plain("A")
        decoy_ret, decoy, pre_d = plain("D")
        assert pre_a == pre_d, (row.name, "the decoy does not keep the counts of the real inputs", pre_a, pre_d)
        assert decoy_ret != ref_ret or not _same(torch, decoy, ref), (row.name, "the decoy's answer equals the real one: the row proves nothing")

        # the sandwich
        if plan.pre:
            _load(plan, "A")
            torch.cuda.synchronize()
            assert plan.pre() == pre_a
            torch.cuda.synchronize()
        _load(plan, "D")
        _fill(plan)
        for s in snaps:
            _raw(s).fill_(0x3C)
        torch.cuda.synchronize()
        allocs = torch.cuda.memory_stats().get("allocation.all.allocated", 0)
        t0 = time.perf_counter()
        # a sensitivity row makes the CALLER's mistake: the entry (and the copy of what it wrote) on the null stream, the copies on S
        entry_stream = torch.cuda.current_stream() if row.sensitivity else stream
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            for live, sa, _ in plan.inputs:
                live.copy_(sa, non_blocking=True)
        with torch.cuda.stream(entry_stream):
            ret = plan.call()
            busy = not stream.query()
            t1 = time.perf_counter()
            _snap(plan, snaps)
        with torch.cuda.stream(stream):
            for live, _, sd in plan.inputs:
                live.copy_(sd, non_blocking=True)
        stream.synchronize()
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats().get("allocation.all.allocated", 0) == allocs, (row.name, "the sandwich allocated device memory")
        enqueue_ms = (t1 - t0) * 1e3
        TIMINGS.append((row.name, enqueue_ms, delay_ms))
        print("STREAM_ORDER %-34s enqueue %8.3f ms  delay %7.2f ms  ratio %.4f  busy %s" % (row.name, enqueue_ms, delay_ms, enqueue_ms / delay_ms, busy))
        if row.sensitivity:
            assert busy, (row.name, "the delay had ended before the entry on the null stream returned", "enqueue ms", enqueue_ms, "delay ms", delay_ms)
            assert ret == decoy_ret and _same(torch, snaps, decoy), (row.name, "an entry on the null stream must have seen the decoy", _first_difference(torch, plan, snaps, decoy))
            assert ret != ref_ret or not _same(torch, snaps, ref), (row.name, "the harness cannot tell the streams apart")
            return
        if row.check_status:
            _check_status(env, plan, (row.name, "sandwich"))
        assert ret == ref_ret, (row.name, "host values differ from the plain call's", ret, ref_ret, decoy_ret)
        assert _same(torch, snaps, ref), (row.name, "outputs differ from the plain call's", _first_difference(torch, plan, snaps, ref),
                                         "equal to the decoy's" if _same(torch, snaps, decoy) else "not the decoy's either")
        _guards(torch, plan, snaps, (row.name, "sandwich"))
        if row.cls == ASYNC:
            assert busy, (row.name, "the call waited for the stream, or its enqueue outran the delay", "enqueue ms", enqueue_ms, "delay ms", delay_ms)
    finally:
        torch.cuda.synchronize()
        if plan is not None:
            for c in plan.closers:
                c()
        ctx.close()


# ---- decoys of draw records ---------------------------------------------------------------------------------------------------------------
def moved_draws(d, dx=8.0, dy=-5.0):
    """The same records under an integer translation, colours XORed: every count and offset stays (structure_checks asserts it)."""
    e = d.copy()
    e["mtx"][:, 4] += F(dx)
    e["mtx"][:, 5] += F(dy)
    e["fill_color"] ^= np.uint32(0x00FFFFFF)
    e["stroke_color"] ^= np.uint32(0x00FFFFFF)
    return e


def resized_draws(d):
    """For the *_count entries, whose answer a count-preserving decoy would not change: every fifth draw flattened at four times the scale."""
    e = d.copy()
    e["scale"][::5] *= F(4.0)
    return e


MESH_FIELDS = ("first_vertex", "first_index", "num_vertices", "num_indices", "draw", "subpath_kind")


def same_structure(ra, rb):
    assert ra.sizes == rb.sizes, (ra.sizes, rb.sizes)
    for k in MESH_FIELDS:
        assert np.array_equal(ra.meshes[k], rb.meshes[k]), ("meshes." + k)
    assert np.array_equal(ra.subpaths.view(np.uint8), rb.subpaths.view(np.uint8)), "sub-path records"
    assert np.array_equal(ra.draw_info.view(np.uint8), rb.draw_info.view(np.uint8)), "per-draw records"
    assert np.array_equal(ra.idx, rb.idx), "indices"


class Fix:
    pass


@functools.lru_cache(maxsize=None)
def draw_fixture(n):
    """wl.tiger(n): the real draws, the count-preserving decoy and the resized decoy, checked on the CPU oracle."""
    import pyoracle as oracle
    wl = importlib.import_module("vg-renderer_amd.workloads")
    fx = Fix()
    fx.ps, fx.a = wl.tiger(n)
    fx.d, fx.s = moved_draws(fx.a), resized_draws(fx.a)
    ra, rd = oracle.tessellate(fx.ps, fx.a, want_flat=True), oracle.tessellate(fx.ps, fx.d, want_flat=True)
    same_structure(ra, rd)
    assert not np.array_equal(ra.pos, rd.pos) and not np.array_equal(ra.color, rd.color)
    rs = oracle.tessellate(fx.ps, fx.s, count_only=True)
    for k in ("num_poly_vertices", "num_vertices", "num_indices"):
        assert rs.sizes[k] > ra.sizes[k], (k, rs.sizes, ra.sizes)   # the totals differ, and the resized batch is the larger
    fx.sizes, fx.sizes_s = ra.sizes, rs.sizes
    return fx


def dash_records(draws):
    """One struct vgx_dash per draw: every second stroked draw dashed [6, 3] at phase 1.5."""
    capi = importlib.import_module("vg-renderer_amd.capi")
    dashes = np.zeros(draws.shape[0], dtype=capi.dash_dtype)
    on = np.flatnonzero(draws["stroke_flags"] & 1)[::2]
    dashes["count"][on] = 2
    dashes["phase"][on] = 1.5
    return dashes, np.array([6.0, 3.0], dtype=F)


POLY_MOVE = np.array([8.0, -5.0], dtype=F)   # the decoy of a flattened polyline: the real one under this integer translation


@functools.lru_cache(maxsize=None)
def dash_fixture():
    """vgx_dash's inputs -- wl.tiger(1) flattened with its transforms by the CPU oracle, one dash record per draw -- and the pieces
    tests/dash_model.py cuts from them. The decoy (the polyline under POLY_MOVE, records and pattern as they are) gives the same piece,
    draw and source records, so the counts, the offsets and the scratch needs of the real inputs hold for it; only coordinates differ."""
    import dash_model as M
    import pyoracle as oracle
    fx = draw_fixture(1)
    d = Fix()
    d.flat = oracle.flatten(fx.ps, fx.a, apply_transform=True)
    d.sub_draw = np.repeat(np.arange(fx.a.shape[0], dtype=np.uint32), d.flat.draw_info["num_subpaths"])
    d.dashes, d.pattern = dash_records(fx.a)
    d.moved = (d.flat.poly + POLY_MOVE).astype(F)
    st_a, poly_a, subs_a, draw_a, src_a = M.dash(d.flat.poly, d.flat.subpaths, d.sub_draw, d.dashes, d.pattern)
    st_d, poly_d, subs_d, draw_d, src_d = M.dash(d.moved, d.flat.subpaths, d.sub_draw, d.dashes, d.pattern)
    assert st_a == 0 and st_d == 0
    assert np.array_equal(subs_a.view(np.uint8), subs_d.view(np.uint8)), "piece records"
    assert np.array_equal(draw_a, draw_d) and np.array_equal(src_a, src_d), "draw and source of the pieces"
    assert poly_a.shape == poly_d.shape and not np.array_equal(poly_a, poly_d)
    assert subs_a.shape[0] > d.flat.subpaths.shape[0]   # some list is cut into several pieces
    d.num_pieces, d.num_piece_vertices = int(subs_a.shape[0]), int(poly_a.shape[0])
    return d


@functools.lru_cache(maxsize=None)
def dashed_frame_fixture():
    """vgx_tessellate_dashed's inputs -- wl.tiger(3), every second stroked draw dashed -- and the frame tests/dashed_frame_model.py
    composes for them from the CPU oracle and tests/dash_model.py. The moved draws give the same pieces, the same mesh table and the
    same indices; the fixture meets the model's own condition, so the model's totals are the call's."""
    import dashed_frame_model as DF
    import pyoracle as oracle
    fx = draw_fixture(3)
    d = Fix()
    d.dashes, d.pattern = dash_records(fx.a)
    cond = DF.fixture_condition(oracle, fx.ps, fx.a, d.dashes, d.pattern)
    assert all(cond[k] == 0 for k in ("epsilon", "negative_zeros", "short", "not_returned")), cond
    fa, fd = DF.frame(oracle, fx.ps, fx.a, d.dashes, d.pattern), DF.frame(oracle, fx.ps, fx.d, d.dashes, d.pattern)
    assert fa.sizes == fd.sizes and fa.dash_sizes == fd.dash_sizes, (fa.sizes, fd.sizes, fa.dash_sizes, fd.dash_sizes)
    for k in MESH_FIELDS:
        assert np.array_equal(fa.meshes[k], fd.meshes[k]), ("meshes." + k)
    assert np.array_equal(fa.idx, fd.idx), "indices"
    assert np.array_equal(fa.piece_draw, fd.piece_draw) and np.array_equal(fa.piece_src_sub, fd.piece_src_sub), "draw and source of the pieces"
    assert not np.array_equal(fa.pos, fd.pos) and not np.array_equal(fa.color, fd.color)
    assert fa.dash_sizes["num_subpaths"] > 100
    d.sizes, d.dash_sizes = fa.sizes, fa.dash_sizes
    return d


def structure_checks():
    """The admissibility of the decoys that have a CPU oracle or model, as callables (the CPU table test runs them; the rows run them
    again before their first GPU call)."""
    return [functools.partial(draw_fixture, 3), functools.partial(draw_fixture, 1), permuted_draw_info_check, dash_fixture, dashed_frame_fixture]


def permuted_draw_info(info):
    """vgx_subpath_draws' decoy: the same sub-paths dealt to the draws in reverse order of their counts; offsets recomputed, so the
    records still tile [0, nsubpaths)."""
    e = info.copy()
    e["num_subpaths"] = info["num_subpaths"][::-1]
    e["first_subpath"] = np.cumsum(e["num_subpaths"].astype(np.uint64)) - e["num_subpaths"]
    return e


def permuted_draw_info_check():
    capi = importlib.import_module("vg-renderer_amd.capi")
    info = np.zeros(5, dtype=capi.draw_info_dtype)
    info["num_subpaths"] = [1, 3, 0, 2, 5]
    info["first_subpath"] = [0, 1, 4, 4, 6]
    e = permuted_draw_info(info)
    assert e["num_subpaths"].tolist() == [5, 2, 0, 3, 1] and e["first_subpath"].tolist() == [0, 5, 7, 7, 10]
    assert int(e["num_subpaths"].sum()) == int(info["num_subpaths"].sum())


# ---- rows: entries that read draws ----------------------------------------------------------------------------------------------------------
def _draws(env, ctx, decoy="d", n=3):
    fx = draw_fixture(n)
    rt = env.rt
    p = Plan()
    p.pset = rt.PathSet(ctx, fx.ps)
    p.closers.append(p.pset.close)
    p.n = fx.a.shape[0]
    p.dd = p.new_inp(fx.a, getattr(fx, decoy))
    p.sizes = rt.tessellate_count(ctx, p.pset, p.dd, p.n)   # the product's totals of A; sizes the context's scratch
    for k in ("num_vertices", "num_indices", "num_meshes", "num_poly_vertices", "num_subpaths"):
        assert p.sizes[k] == fx.sizes[k], (k, p.sizes, fx.sizes)
    return p, fx


def _sizes_tuple(z):
    return tuple(sorted(z.as_dict().items()))


def make_flatten_count(env, ctx):
    p, _ = _draws(env, ctx, "s")

    def call():
        z = env.capi.Sizes()
        env.rt._check(env.lib.vgx_flatten_count(ctx.handle, p.pset.handle, p.dd.data_ptr(), p.n, C.byref(z), env.rt._stream_ptr()), "vgx_flatten_count")
        return _sizes_tuple(z)
    p.call = call
    return p


def _flat_out(p, env, guard=64):
    npv, nsp = p.sizes["num_poly_vertices"], p.sizes["num_subpaths"]
    b = env.rt.FlatBuffers("cuda:0", npv + guard, nsp + guard, p.n)
    b.cap = (npv, nsp)
    p.out(b.poly, used=npv * 8), p.out(b.subs, used=nsp * 16), p.out(b.dinfo)
    return b


def make_flatten_emit(env, ctx):
    p, _ = _draws(env, ctx)
    b = _flat_out(p, env)
    out = b.out_struct()

    def pre():
        z = env.capi.Sizes()
        env.rt._check(env.lib.vgx_flatten_count(ctx.handle, p.pset.handle, p.dd.data_ptr(), p.n, C.byref(z), env.rt._stream_ptr()), "vgx_flatten_count")
        return _sizes_tuple(z)

    def call():
        env.rt._check(env.lib.vgx_flatten_emit(ctx.handle, p.pset.handle, p.dd.data_ptr(), p.n, 1, C.byref(out), env.rt._stream_ptr()), "vgx_flatten_emit")
    p.pre, p.call = pre, call
    return p


def make_flatten(env, ctx):
    p, _ = _draws(env, ctx)
    b = _flat_out(p, env)
    p.out(b.dev_sizes), p.out(b.dev_status)
    p.status.append(b.dev_status)
    p.call = lambda: env.rt.flatten_async(ctx, p.pset, p.dd, p.n, b, True)
    return p


def make_tessellate_count(env, ctx):
    p, _ = _draws(env, ctx, "s")
    p.call = lambda: tuple(sorted(env.rt.tessellate_count(ctx, p.pset, p.dd, p.n).items()))
    return p


def _mesh_out_of(p, env):
    return mesh_out(p, env, p.sizes["num_vertices"], p.sizes["num_indices"], p.sizes["num_meshes"])


def make_tessellate_emit(env, ctx):
    p, _ = _draws(env, ctx)
    b = _mesh_out_of(p, env)
    p.status.remove(b.dev_status)   # the emit has no status word of its own: the fill pattern stays there
    p.pre = lambda: tuple(sorted(env.rt.tessellate_count(ctx, p.pset, p.dd, p.n).items()))
    p.call = lambda: env.rt.tessellate_emit(ctx, p.pset, p.dd, p.n, b)
    return p


def make_tessellate(env, ctx):
    p, _ = _draws(env, ctx)
    b = _mesh_out_of(p, env)
    p.call = lambda: env.rt.tessellate_async(ctx, p.pset, p.dd, p.n, b)
    return p


def make_tessellate_assembly(env, ctx):
    """vgx_tessellate with draw-command assembly armed: the partition and the UV fill are launches of its own."""
    torch = env.torch
    p, _ = _draws(env, ctx)
    b = _mesh_out_of(p, env)
    nv, max_vb = p.sizes["num_vertices"], 4096
    ncmd = 2 * nv // max_vb + 2 + 8
    cmds = p.out(torch.zeros((ncmd + 8) * 48, dtype=torch.uint8, device="cuda:0"), used=ncmd * 48)
    num = p.out(torch.zeros(1, dtype=torch.int64, device="cuda:0"))
    uv = p.out(torch.zeros((nv + 64, 2), dtype=torch.int16, device="cuda:0"), used=nv * 4)
    ctx.set_assembly(cmds[:ncmd * 48], max_vb, num, split_state=True, uv=uv, uv_value=(0x7FFF0001, 0))
    p.closers.append(lambda: ctx.set_assembly(None))
    p.call = lambda: env.rt.tessellate_async(ctx, p.pset, p.dd, p.n, b)
    return p


def make_tessellate_immediate(env, ctx):
    p, _ = _draws(env, ctx)
    b = _mesh_out_of(p, env)
    ctx.reserve(p.n, {k: 2 * int(v) for k, v in p.sizes.items()})   # no VGX_E_GROWN: the grow protocol is not under test here
    p.call = lambda: env.rt.tessellate_immediate(ctx, p.pset, p.dd, p.n, b)
    return p


def make_tessellate_dashed(env, ctx):
    torch, rt = env.torch, env.rt
    df = dashed_frame_fixture()   # the decoy keeps every piece, mesh record and index of the real frame (CPU model)
    p, fx = _draws(env, ctx)
    dashes, pattern = df.dashes, df.pattern
    dd, pd = to_dev(dashes), torch.from_numpy(pattern).to("cuda:0")
    p.keep += [dd, pd]
    r = rt.tessellate_dashed(ctx, p.pset, p.dd, p.n, dd, pd, pattern.shape[0], to_host=False)   # the grow protocol run to its end on the real frame
    for k, v in df.sizes.items():
        assert r.sizes[k] == v, (k, r.sizes, df.sizes)
    for k in ("num_subpaths", "num_poly_vertices"):
        assert r.dash_sizes[k] == df.dash_sizes[k], (k, r.dash_sizes, df.dash_sizes)
    ctx.reserve_dashed(p.n, r.sizes, r.dash_sizes)   # the real frame's totals: they are the decoy's
    z = df.sizes
    b = mesh_out(p, env, z["num_vertices"], z["num_indices"], z["num_meshes"])
    dds = p.out(torch.zeros(10, dtype=torch.int64, device="cuda:0"))
    p.call = lambda: rt.tessellate_dashed_async(ctx, p.pset, p.dd, p.n, dd, pd, pattern.shape[0], b, dds)
    return p


def make_partition(env, ctx):
    p, _ = _draws(env, ctx, "s")

    def call():
        bounds, weights = env.rt.partition(ctx, p.pset, p.dd, p.n, 4)
        return tuple(bounds), tuple(weights)
    p.call = call
    return p


def make_failure_info(env, ctx):
    """The status word of the call in front of it: the real batch fits the buffers, the resized decoy does not (VGX_E_NOSPACE, nothing
    written past a capacity). Both calls of the row go to the same stream."""
    p, fx = _draws(env, ctx, "s")
    assert fx.sizes_s["num_vertices"] > fx.sizes["num_vertices"]
    b = env.rt.MeshBuffers("cuda:0", p.sizes["num_vertices"], p.sizes["num_indices"], p.sizes["num_meshes"])
    p.keep.append(b)

    def call():
        env.rt.tessellate_async(ctx, p.pset, p.dd, p.n, b)
        fi = env.capi.FailureInfo()
        env.rt._check(env.lib.vgx_get_failure_info(ctx.handle, C.byref(fi), env.rt._stream_ptr()), "vgx_get_failure_info")
        return int(fi.status), int(fi.reason)
    p.call = call
    return p


# ---- rows: entries that read polylines ------------------------------------------------------------------------------------------------------
def _polylines(env, ctx, draws_decoy=None, move=True):
    """wl.tiger(1) flattened with its transforms on the row's context: poly / sub-path records / per-draw records in device memory.
    The decoy polyline is the real one under the integer translation POLY_MOVE. For vgx_dash the CPU model shows that it keeps every
    piece (dash_fixture). The stroker-level entries have no CPU oracle of their own: that the moved lists keep every mesh's counts rests
    on draw_fixture(1) (the same translation applied through the transforms, close to this input but not the same) and is pinned on
    the device -- vgx_stroke_emit by the equal vgx_stroke_count totals of both inputs, vgx_stroke by VGX_OK into exact capacities."""
    rt, torch = env.rt, env.torch
    fx = draw_fixture(1)
    p = Plan()
    pset = rt.PathSet(ctx, fx.ps)
    p.n = fx.a.shape[0]
    dd = rt.upload_draws(fx.a)
    r = rt.flatten_one_walk(ctx, pset, dd, p.n, True, to_host=True)
    p.nsp, p.npv = r.sizes["num_subpaths"], r.sizes["num_poly_vertices"]
    p.sub_draw = rt.subpath_draws(ctx, r.dinfo_dev, p.n, p.nsp)
    torch.cuda.synchronize()
    pset.close()
    p.flat = r
    p.poly, p.subs, p.dinfo = r.poly_dev, r.subs_dev, r.dinfo_dev
    p.inp(p.poly, r.poly, (r.poly + POLY_MOVE).astype(F) if move else r.poly)
    dec = fx.a.copy() if draws_decoy is None else draws_decoy(fx.a)
    p.dd = p.new_inp(fx.a, dec)
    return p, fx


def _recoloured(d):
    e = d.copy()
    e["fill_color"] ^= np.uint32(0x00FFFFFF)
    e["stroke_color"] ^= np.uint32(0x00FFFFFF)
    return e


def _fewer_strokes(d):
    e = d.copy()
    e["stroke_flags"][::3] = 0
    return e


def _stroke_count(env, ctx, p):
    z = env.capi.Sizes()
    env.rt._check(env.lib.vgx_stroke_count(ctx.handle, p.poly.data_ptr(), p.subs.data_ptr(), p.sub_draw.data_ptr(), p.nsp, p.dd.data_ptr(), p.n, C.byref(z),
                                           env.rt._stream_ptr()), "vgx_stroke_count")
    return z


def make_stroke_count(env, ctx):
    p, _ = _polylines(env, ctx, _fewer_strokes, move=False)
    p.call = lambda: _sizes_tuple(_stroke_count(env, ctx, p))
    return p


def make_stroke_emit(env, ctx):
    p, _ = _polylines(env, ctx, _recoloured)
    z = _stroke_count(env, ctx, p).as_dict()
    b = mesh_out(p, env, z["num_vertices"], z["num_indices"], z["num_meshes"])
    p.status.remove(b.dev_status)
    out = b.out_struct()

    def call():
        env.rt._check(env.lib.vgx_stroke_emit(ctx.handle, p.poly.data_ptr(), p.subs.data_ptr(), p.sub_draw.data_ptr(), p.nsp, p.dd.data_ptr(), p.n, C.byref(out),
                                              env.rt._stream_ptr()), "vgx_stroke_emit")
    p.pre, p.call = (lambda: _sizes_tuple(_stroke_count(env, ctx, p))), call
    return p


def make_stroke(env, ctx):
    p, _ = _polylines(env, ctx, _recoloured)
    z = _stroke_count(env, ctx, p).as_dict()
    b = mesh_out(p, env, z["num_vertices"], z["num_indices"], z["num_meshes"])
    p.call = lambda: env.rt.stroke_async(ctx, p.poly, p.subs, p.sub_draw, p.nsp, p.dd, p.n, b)
    return p


def _dashes(env, p, fx, pattern_decoy=None):
    dashes, pattern = dash_records(fx.a)
    p.dashes = to_dev(dashes)
    p.keep.append(p.dashes)
    pd = env.torch.from_numpy(pattern).to("cuda:0")
    p.pattern = p.inp(pd, pattern, pattern if pattern_decoy is None else np.array(pattern_decoy, dtype=F))
    p.npat = pattern.shape[0]


def make_dash_count(env, ctx):
    p, fx = _polylines(env, ctx, move=False)
    _dashes(env, p, fx, pattern_decoy=[9.0, 2.0])
    p.call = lambda: tuple(sorted(env.rt.dash_count(ctx, p.poly, p.subs, p.sub_draw, p.nsp, p.dashes, p.n, p.pattern, p.npat).items()))
    return p


def make_dash(env, ctx):
    rt = env.rt
    df = dash_fixture()   # the moved polyline gives the piece records of the real one (tests/dash_model.py)
    p, fx = _polylines(env, ctx)
    assert np.array_equal(p.flat.poly.view(np.uint32), df.flat.poly.view(np.uint32)), "the row's polyline is not the one the CPU check speaks of"
    assert np.array_equal(p.flat.subpaths.view(np.uint8), df.flat.subpaths.view(np.uint8))
    assert np.array_equal(p.sub_draw[:p.nsp].cpu().numpy().view(np.uint32), df.sub_draw)
    _dashes(env, p, fx)
    z = rt.dash_count(ctx, p.poly, p.subs, p.sub_draw, p.nsp, p.dashes, p.n, p.pattern, p.npat)   # sizes the scratch: no VGX_E_GROWN
    assert (z["num_poly_vertices"], z["num_subpaths"]) == (df.num_piece_vertices, df.num_pieces), (z, df.num_piece_vertices, df.num_pieces)
    npv, nsp = df.num_piece_vertices, df.num_pieces
    b = rt.DashBuffers("cuda:0", npv + 64, nsp + 64)
    b.cap = (npv, nsp)
    p.out(b.poly, used=npv * 8), p.out(b.subs, used=nsp * 16), p.out(b.sub_draw, used=nsp * 4), p.out(b.sub_src, used=nsp * 4)
    p.out(b.dev_sizes), p.out(b.dev_status)
    p.status.append(b.dev_status)
    p.call = lambda: rt.dash_async(ctx, p.poly, p.subs, p.sub_draw, p.nsp, p.dashes, p.n, p.pattern, p.npat, b)
    return p


def make_subpath_draws(env, ctx):
    torch = env.torch
    p, _ = _polylines(env, ctx, move=False)
    p.inputs = []   # this entry reads the per-draw records alone
    permuted_draw_info_check()
    p.inp(p.dinfo, p.flat.draw_info, permuted_draw_info(p.flat.draw_info))
    out = p.out(torch.zeros(p.nsp + 64, dtype=torch.int32, device="cuda:0"), used=p.nsp * 4)

    def call():
        env.rt._check(env.lib.vgx_subpath_draws(ctx.handle, p.dinfo.data_ptr(), p.n, out.data_ptr(), p.nsp, env.rt._stream_ptr()), "vgx_subpath_draws")
    p.call = call
    return p


def make_concave_contours(env, ctx):
    import raster_harness as H
    fl = H.Flat(H.contour_specs())
    nm, nv, ni = fl.expected_sizes()
    p = Plan()
    poly = p.new_inp(fl.poly, (fl.poly + np.array([8.0, -5.0], dtype=F)).astype(F))
    draws = p.new_inp(fl.draws, _recoloured(fl.draws))
    subs, info = to_dev(fl.subs), to_dev(fl.info)
    p.keep += [subs, info]
    b = mesh_out(p, env, nv, ni, nm)
    out = b.out_struct()

    def call():
        env.rt._check(env.lib.vgx_concave_contours(ctx.handle, poly.data_ptr(), subs.data_ptr(), info.data_ptr(), draws.data_ptr(), len(fl.specs), C.byref(out),
                                                   b.dev_sizes.data_ptr(), b.dev_status.data_ptr(), env.rt._stream_ptr()), "vgx_concave_contours")
    p.call = call
    return p


def _concave_fills(env, ctx):
    import test_gpu_concave as TC
    ref = TC.load_ref(env.oracle)
    return TC._prepare_fills(env.rt, ctx, ref, TC._fills())


def _dev_numpy(t):
    return t.cpu().numpy()


def make_concave_move(env, ctx):
    torch = env.torch
    q = _concave_fills(env, ctx)
    p = Plan()
    p.keep.append(q)
    bv = _dev_numpy(q.bv_d)
    p.inp(q.bv_d, bv, (bv + np.array([8.0, -5.0], dtype=F)).astype(F))
    n = int(q.bv_d.shape[0])
    moved = p.out(torch.zeros((n + 64, 2), dtype=torch.float32, device="cuda:0"), used=n * 8)

    def call():
        env.rt._check(env.lib.vgx_concave_move(ctx.handle, q.bv_d.data_ptr(), n, q.cont_d.data_ptr(), q.ncont, q.fr_d.data_ptr(), q.nfills, moved.data_ptr(),
                                               env.rt._stream_ptr()), "vgx_concave_move")
    p.call = call
    return p


def make_concave_emit(env, ctx):
    q = _concave_fills(env, ctx)
    p = Plan()
    p.keep.append(q)
    t = np.array([8.0, -5.0], dtype=F)
    bv, tp = _dev_numpy(q.bv_d), _dev_numpy(q.tp_d)
    p.inp(q.bv_d, bv, (bv + t).astype(F))
    p.inp(q.tp_d, tp, (tp + t).astype(F))
    fr = _dev_numpy(q.fr_d).view(env.capi.concave_fill_dtype)
    e = fr.copy()
    e["color"] ^= np.uint32(0x00FFFFFF)
    p.inp(q.fr_d, fr, e)
    b = mesh_out(p, env, q.nv, q.ni, q.nfills)
    p.call = lambda: env.rt.concave_emit(ctx, q.bv_d, q.cont_d, q.ncont, q.fr_d, q.nfills, q.tp_d, q.ti_d, b)
    return p


def make_text_quads(env, ctx):
    """The frame-sized batch of tests/test_gpu_text.py: 60 runs of 1 .. 119 quads, a UV stream of 8 bytes per vertex."""
    import test_text_cpu as TCPU
    torch, rt = env.torch, env.rt
    rng = np.random.default_rng(7)
    runs, quads = TCPU.random_runs(env.capi, rng, np.asarray(rng.integers(1, 120, 60), np.int64))
    nv, ni = rt.text_runs_dense(runs, 0, 0)
    e = runs.copy()
    e["x"] += F(8.0)
    e["y"] -= F(5.0)
    e["color"] ^= np.uint32(0x00FFFFFF)
    p = Plan()
    rd = p.new_inp(runs, e)
    qd = torch.from_numpy(np.ascontiguousarray(quads, F).reshape(-1, 8)).to("cuda:0")
    p.inp(qd, quads, (quads + np.array([3.0, 2.0, 3.0, 2.0, 0, 0, 0, 0], dtype=F)).astype(F))
    b = mesh_out(p, env, nv, ni, runs.shape[0])
    uv = p.out(torch.zeros((nv + 64, 2), dtype=torch.float32, device="cuda:0"), used=nv * 8)
    p.call = lambda: rt.text_quads(ctx, qd, quads.shape[0], rd, runs.shape[0], b, first_mesh=0, uv_dev=uv, uv_bytes=8)
    return p


# ---- rows: merging ------------------------------------------------------------------------------------------------------------------------
def _merge(env, ctx, entry):
    import mesh_streams as MS
    torch = env.torch
    rs = np.random.RandomState(3)
    a, b = MS.make_stream(rs, 300, 6, 50), MS.make_stream(rs, 200, 6, 50, holes=True)
    b_draw = b.meshes["draw"].copy()
    want = MS.merge_model(a, b, b_draw)
    p = Plan()
    t = np.array([8.0, -5.0], dtype=F)
    ta = [p.new_inp(a.pos, (a.pos + t).astype(F)), p.new_inp(a.color, a.color ^ np.uint32(0x00FFFFFF)), to_dev(a.idx), to_dev(a.meshes)]
    tb = [p.new_inp(b.pos, (b.pos + t).astype(F)), p.new_inp(b.color, b.color ^ np.uint32(0x00FFFFFF)), to_dev(b.idx), to_dev(b.meshes)]
    p.keep += ta + tb
    da = env.capi.CacheDesc(ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), ta[3].data_ptr(), a.meshes.shape[0], a.pos.shape[0], a.idx.shape[0])
    db = env.capi.CacheDesc(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3].data_ptr(), b.meshes.shape[0], b.pos.shape[0], b.idx.shape[0])
    bd = to_dev(np.ascontiguousarray(b_draw, dtype=np.uint32))
    p.keep.append(bd)
    nv = want.pos.shape[0]
    out = mesh_out(p, env, nv, want.idx.shape[0], want.meshes.shape[0])
    ms = out.out_struct()
    buv = MS._u32(np.random.RandomState(5), max(b.pos.shape[0], 1) * 2).reshape(-1, 2)
    uv_in = p.new_inp(buv, buv ^ np.uint32(0x0F0F0F0F))
    L, rt = env.lib, env.rt
    if entry == "vgx_merge":
        def call():
            rt._check(L.vgx_merge(ctx.handle, C.byref(da), C.byref(db), bd.data_ptr(), None, 0, C.byref(ms), out.dev_sizes.data_ptr(), out.dev_status.data_ptr(),
                                  rt._stream_ptr()), entry)
    elif entry == "vgx_merge_uv":
        # b_uv only has an effect under an armed assembly with a UV stream
        ncmd = 2 * nv // 256 + 2 + 8
        cmds = p.out(torch.zeros((ncmd + 8) * 48, dtype=torch.uint8, device="cuda:0"), used=ncmd * 48)
        num = p.out(torch.zeros(1, dtype=torch.int64, device="cuda:0"))
        asm_uv = p.out(torch.zeros((nv + 64, 2), dtype=torch.float32, device="cuda:0"), used=nv * 8)
        ctx.set_assembly(cmds[:ncmd * 48], 256, num, split_state=False, uv=asm_uv, uv_value=(0x7FFF0001, 0x3E800000))
        p.closers.append(lambda: ctx.set_assembly(None))

        def call():
            rt._check(L.vgx_merge_uv(ctx.handle, C.byref(da), C.byref(db), bd.data_ptr(), uv_in.data_ptr(), None, 0, C.byref(ms), out.dev_sizes.data_ptr(),
                                     out.dev_status.data_ptr(), rt._stream_ptr()), entry)
    else:
        out_uv = p.out(torch.zeros((nv + 64, 2), dtype=torch.int32, device="cuda:0"), used=nv * 8)

        def call():
            rt._check(L.vgx_merge_uv_stream(ctx.handle, C.byref(da), C.byref(db), bd.data_ptr(), uv_in.data_ptr(), 8, None, 0, C.byref(ms), out_uv.data_ptr(),
                                            out.dev_sizes.data_ptr(), out.dev_status.data_ptr(), rt._stream_ptr()), entry)
    p.call = call
    return p


# ---- rows: the shape cache ----------------------------------------------------------------------------------------------------------------
def _cache(env, ctx):
    """wl.tiger(1) tessellated and localised on the row's context: a MeshCache, its boxes, the world-space positions it was made from."""
    rt, torch = env.rt, env.torch
    fx = draw_fixture(1)
    pset = rt.PathSet(ctx, fx.ps)
    dd = rt.upload_draws(fx.a)
    n = fx.a.shape[0]
    sizes = rt.tessellate_count(ctx, pset, dd, n)
    bufs = rt.MeshBuffers("cuda:0", sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(ctx, pset, dd, n, bufs)
    torch.cuda.synchronize()
    world = bufs.pos.cpu().numpy().copy()
    cache = rt.MeshCache(ctx, bufs, sizes, dd, n)
    boxes = cache.bounds
    torch.cuda.synchronize()
    pset.close()
    return fx, cache, boxes, world, dd


def _instances(env, nm, n=9, seed=0, ranges=0):
    """n instances of mesh ranges of the cache under integer translations; `seed` moves and recolours them, `ranges` shifts the ranges."""
    inst = np.zeros(n, dtype=env.capi.cache_instance_dtype)
    k = np.arange(n)
    first = (k * 13 + 5 * ranges) % max(nm - 60, 1)
    inst["first_mesh"] = first
    inst["num_meshes"] = np.minimum(nm - first, 20 + 4 * k + ranges)
    inst["color"] = (0xFFFFFFFF - 0x00010203 * (k + 7 * seed)).astype(np.uint32)
    inst["mtx"][:, 0] = inst["mtx"][:, 3] = 1.0
    inst["mtx"][:, 4] = (40.0 * (k % 3) + 16.0 * seed).astype(F)
    inst["mtx"][:, 5] = (30.0 * (k // 3) - 9.0 * seed).astype(F)
    return inst


def make_cache_localize(env, ctx):
    fx, cache, _, world, dd = _cache(env, ctx)
    p = Plan()
    p.keep.append(cache)
    p.inp(cache.bufs.pos, world, world)          # in and out: world-space positions in front of every call
    p.inp(dd, fx.a, moved_draws(fx.a))
    p.out(cache.bufs.pos, fill=None)

    def call():
        env.rt._check(env.lib.vgx_cache_localize(ctx.handle, dd.data_ptr(), fx.a.shape[0], cache.bufs.pos.data_ptr(), cache.bufs.meshes.data_ptr(), cache.nm,
                                                 env.rt._stream_ptr()), "vgx_cache_localize")
    p.call = call
    return p


def _frame_totals(cache, inst):
    m = cache.bufs.meshes[:cache.nm * 32].cpu().numpy().view(np.dtype([("first_vertex", "<u8"), ("first_index", "<u8"), ("num_vertices", "<u4"), ("num_indices", "<u4"),
                                                                      ("draw", "<u4"), ("subpath_kind", "<u4")]))
    nv = ni = nm = 0
    for r in inst:
        a, k = int(r["first_mesh"]), int(r["num_meshes"])
        nv, ni, nm = nv + int(m["num_vertices"][a:a + k].sum()), ni + int(m["num_indices"][a:a + k].sum()), nm + k
    return nv, ni, nm


def make_cache_submit(env, ctx):
    _, cache, _, _, _ = _cache(env, ctx)
    p = Plan()
    inst = _instances(env, cache.nm)
    di = p.new_inp(inst, _instances(env, cache.nm, seed=1))
    b = mesh_out(p, env, *_frame_totals(cache, inst))
    p.call = lambda: env.rt.cache_submit(ctx, cache, di, inst.shape[0], b)
    return p


def make_cache_cull(env, ctx):
    torch, rt = env.torch, env.rt
    _, cache, boxes, _, _ = _cache(env, ctx)
    p = Plan()
    inst = _instances(env, cache.nm)
    far = _instances(env, cache.nm, seed=1)
    far["mtx"][::2, 4] += F(5000.0)   # every second instance leaves the view
    di = p.new_inp(inst, far)
    views = torch.tensor([[0.0, 0.0, 1200.0, 1200.0]], dtype=torch.float32, device="cuda:0")
    r = rt.cache_cull(ctx, cache, boxes, di, inst.shape[0], views)   # allocates the outputs once; reuse= writes them again
    torch.cuda.synchronize()
    p.keep += [views, boxes]
    p.out(r.inst), p.out(r.bounds), p.out(r.kept), p.out(r.num_kept), p.out(r.dev_status)
    p.status.append(r.dev_status)

    def call():
        rt.cache_cull(ctx, cache, boxes, di, inst.shape[0], views, reuse=r)
    p.call = call
    return p


def make_cache_layout(env, ctx):
    """The layout depends on the instances' mesh ranges alone, so this decoy names other (valid) ranges of the cache."""
    torch = env.torch
    _, cache, _, _, _ = _cache(env, ctx)
    p = Plan()
    inst = _instances(env, cache.nm)
    di = p.new_inp(inst, _instances(env, cache.nm, ranges=3))
    n = inst.shape[0]
    slots = p.out(torch.zeros((n + 1 + 4) * 32, dtype=torch.uint8, device="cuda:0"), used=(n + 1) * 32)
    st = status_word(p, env)
    d = cache.desc()

    def call():
        env.rt._check(env.lib.vgx_cache_layout(ctx.handle, C.byref(d), di.data_ptr(), n, slots.data_ptr(), st.data_ptr(), env.rt._stream_ptr()), "vgx_cache_layout")
    p.call = call
    return p


def make_cache_update(env, ctx):
    """A submitted frame, its slots and boxes; the edited instance array is the input, the list's length sits behind a device pointer."""
    torch, rt = env.torch, env.rt
    _, cache, _, _, _ = _cache(env, ctx)
    p = Plan()
    inst = _instances(env, cache.nm)
    n = inst.shape[0]
    nv, ni, nm = _frame_totals(cache, inst)
    frame = rt.MeshBuffers("cuda:0", nv, ni, nm)
    d0 = to_dev(inst)
    rt.cache_submit(ctx, cache, d0, n, frame)
    slots, st0 = rt.cache_layout(ctx, cache, d0, n)
    boxes = rt.mesh_bounds(ctx, frame.pos, frame.meshes, nm)
    torch.cuda.synchronize()
    assert int(frame.dev_status.item()) == 0 and int(st0.item()) == 0
    p.keep += [cache, d0, slots, frame]
    pos0, col0, box0 = frame.pos.cpu().numpy().copy(), frame.color.cpu().numpy().copy(), boxes.cpu().numpy().copy()
    p.inp(frame.pos, pos0, pos0), p.inp(frame.color, col0, col0), p.inp(boxes, box0, box0)   # in and out: the submitted frame in front of every call
    di = p.new_inp(_instances(env, cache.nm, seed=2), _instances(env, cache.nm, seed=3))     # two edits of the same structure
    dirty = to_dev(np.array([7, 2, 5, 0, 8, 3], dtype=np.uint32))
    limit = torch.tensor([4], dtype=torch.int64, device="cuda:0")
    p.keep += [dirty, limit]
    p.out(frame.pos, fill=None), p.out(frame.color, fill=None), p.out(boxes, fill=None)
    st = status_word(p, env)

    def call():
        rt.cache_update(ctx, cache, di, n, slots, dirty, 6, frame.pos, frame.color, nv, nm, mesh_bounds=boxes, dev_ndirty=limit, dev_status=st)
    p.call = call
    return p


# ---- rows: frames of the reference (pick) ----------------------------------------------------------------------------------------------------
def _pick_frame_streams(env, p, f, move_pos=False):
    t = np.array([8.0, -5.0], dtype=F)
    ts = [p.new_inp(f.pos, (f.pos + t).astype(F)) if move_pos else to_dev(f.pos), to_dev(f.color), to_dev(f.idx), to_dev(f.meshes)]
    p.keep += ts
    return ts, env.capi.CacheDesc(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), f.meshes.shape[0], f.pos.shape[0], f.idx.shape[0])


def make_mesh_bounds(env, ctx):
    import pick_model as P
    torch = env.torch
    f = P.frame("tiger", 65)
    p = Plan()
    ts, _ = _pick_frame_streams(env, p, f, move_pos=True)
    out = p.out(torch.zeros((f.nm + 4, 4), dtype=torch.float32, device="cuda:0"), used=f.nm * 16)

    def call():
        env.rt._check(env.lib.vgx_mesh_bounds(ctx.handle, ts[0].data_ptr(), ts[3].data_ptr(), f.nm, out.data_ptr(), env.rt._stream_ptr()), "vgx_mesh_bounds")
    p.call = call
    return p


def make_pick(env, ctx):
    """mesh_bounds == NULL: the call computes the boxes itself, launches of its own in front of the tiles."""
    import pick_model as P
    torch = env.torch
    f = P.frame("tiger", 65)
    p = Plan()
    _, desc = _pick_frame_streams(env, p, f)
    q = f.queries[:256].copy()
    e = q.copy()
    e["x"] += F(11.0)
    e["y"] += F(7.0)
    n = q.shape[0]
    qd = p.new_inp(q, e)
    hits = p.out(torch.zeros((n + 2) * 16, dtype=torch.uint8, device="cuda:0"), used=n * 16)

    def call():
        env.rt.pick(ctx, desc, qd, n, bounds_dev=None, hits_dev=hits)
    p.call = call
    return p


def make_pick_rect(env, ctx):
    import pick_rect_model as PR
    torch, capi = env.torch, env.capi
    r = PR.frame("tiger", 65)
    f = r.f
    p = Plan()
    _, desc = _pick_frame_streams(env, p, f)
    q = np.ascontiguousarray(r.queries[:capi.PICK_RECT_MAX_QUERIES]).copy()
    e = q.copy()
    for k in ("x0", "x1"):
        e[k] += F(11.0)
    for k in ("y0", "y1"):
        e[k] += F(7.0)
    n, cap = q.shape[0], PR.LIST_CAP
    qd = p.new_inp(q, e)
    top = p.out(torch.zeros((n + 2) * 16, dtype=torch.uint8, device="cuda:0"), used=n * 16)
    lst = p.out(torch.zeros((n + 2, cap), dtype=torch.int32, device="cuda:0"), used=n * cap * 4)
    cnt = p.out(torch.zeros(n + 2, dtype=torch.int32, device="cuda:0"), used=n * 4)
    out = capi.PickRectOut(top.data_ptr(), lst.data_ptr(), cnt.data_ptr(), cap, 0)

    def call():
        env.rt._check(env.lib.vgx_pick_rect(ctx.handle, C.byref(desc), None, qd.data_ptr(), n, C.byref(out), env.rt._stream_ptr()), "vgx_pick_rect")
    p.call = call
    return p


# ---- rows: the image family (vgx_raster .. vgx_raster_damaged, vgx_pick_frame) on the `classes` frame of the concave model -----------------
def _image_frame(env, ctx, p):
    import raster_concave_model as K
    import raster_harness as H
    f = K.frame("classes")
    t = np.array([3.0, 2.0], dtype=F)
    df, ds, dx, dp = H.dev_parts(f)
    p.keep += [df, ds, dx, dp]
    p.inp(df.t[0], f.pos, (f.pos + t).astype(F))
    env.rt.raster_reserve(ctx, 8192, 1 << 17)   # no VGX_E_GROWN: that protocol is not under test here
    return f, df, ds, dx, dp


def _make_raster(level):
    def make(env, ctx):
        import damage_model as DM
        import raster_harness as H
        torch, capi = env.torch, env.capi
        p = Plan()
        f, df, ds, dx, dp = _image_frame(env, ctx, p)
        tgt = f.target.with_clear(0xFF204060)
        n = H.rank(level)
        image = p.out(torch.zeros((tgt.rows() + 2, tgt.stride), dtype=torch.int32, device="cuda:0"), used=tgt.rows() * tgt.stride * 4)
        st = status_word(p, env)
        structs = [x.struct for x in (ds, dx, dp)[:min(n, 3)]] + [tgt.struct(image.data_ptr())]
        if n == 5:
            bits = H.DevBits(tgt.width, tgt.height, fill=DM.all_bits(tgt.width, tgt.height))
            p.keep.append(bits)
            structs.append(capi.RasterDamage(bits.t.data_ptr(), 1 << 20, 0))
        entry = getattr(env.lib, H.entry_name("vgx_", n))
        refs = [C.byref(s) for s in structs]

        def call():
            env.rt._check(entry(ctx.handle, C.byref(df.desc), None, 0, H.OPEN, *refs, st.data_ptr(), env.rt._stream_ptr()), level)
        p.call = call
        return p
    return make


def make_pick_frame(env, ctx):
    import pick_frame_model as PF
    torch = env.torch
    p = Plan()
    f, df, ds, _, _ = _image_frame(env, ctx, p)
    p.inputs = []   # the queries move, the frame stays
    q = PF.centre_queries(f.target)[::12][:256].copy()   # 256 pixel centres spread over the image
    e = q.copy()
    e["x"] += F(3.0)
    e["y"] += F(2.0)
    n = q.shape[0]
    qd = p.new_inp(q, e)
    hits = p.out(torch.zeros((n + 2) * 16, dtype=torch.uint8, device="cuda:0"), used=n * 16)
    st = status_word(p, env)

    def call():
        env.rt._check(env.lib.vgx_pick_frame(ctx.handle, C.byref(df.desc), None, 0, 2**64 - 1, C.byref(ds.struct), qd.data_ptr(), n, hits.data_ptr(), st.data_ptr(),
                                             env.rt._stream_ptr()), "vgx_pick_frame")
    p.call = call
    return p


def make_damage_meshes(env, ctx):
    import damage_model as DM
    import raster_harness as H
    torch = env.torch
    bounds, _, width, height, x0, y0 = DM.list_scene()   # 349 small boxes on a 528 x 40 image; the first 40 are marked
    nm = bounds.shape[0]
    p = Plan()
    bd = torch.from_numpy(bounds).to("cuda:0")
    p.inp(bd, bounds, (bounds + np.array([16.0, 0.0, 16.0, 0.0], dtype=F)).astype(F))   # every box a tile to the right
    words = DM.words(width, height)
    bits = p.out(torch.zeros(words + 2, dtype=torch.int32, device="cuda:0"), fill=0, used=words * 4)
    t = H.mark_target(width, height, x0, y0)

    def call():
        env.rt._check(env.lib.vgx_damage_meshes(ctx.handle, bd.data_ptr(), 0, 40, nm, C.byref(t), bits.data_ptr(), env.rt._stream_ptr()), "vgx_damage_meshes")
    p.call = call
    return p


def make_damage_instances(env, ctx):
    import damage_model as DM
    import raster_harness as H
    torch = env.torch
    bounds, slots, width, height, x0, y0 = DM.list_scene()
    nm, ninst = bounds.shape[0], slots.shape[0] - 1
    p = Plan()
    bd = torch.from_numpy(bounds).to("cuda:0")
    p.keep.append(bd)
    sd = to_dev(slots)
    dirty = p.new_inp(np.array([1, 2, 40, 45, 7, 9], dtype=np.uint32), np.array([3, 44, 12, 30, 7, 9], dtype=np.uint32))
    limit = torch.tensor([4], dtype=torch.int64, device="cuda:0")
    p.keep += [sd, limit]
    words = DM.words(width, height)
    bits = p.out(torch.zeros(words + 2, dtype=torch.int32, device="cuda:0"), fill=0, used=words * 4)
    st = status_word(p, env)
    t = H.mark_target(width, height, x0, y0)

    def call():
        env.rt._check(env.lib.vgx_damage_instances(ctx.handle, bd.data_ptr(), nm, sd.data_ptr(), ninst, dirty.data_ptr(), 6, limit.data_ptr(), C.byref(t), bits.data_ptr(),
                                                   st.data_ptr(), env.rt._stream_ptr()), "vgx_damage_instances")
    p.call = call
    return p


# ---- rows: draw-command tables (the `painted` scene of tests/raster_commands_harness.py) ------------------------------------------------------
def _scene(env, ctx, p, name="painted"):
    import raster_commands_harness as CH
    sc = CH.scene(name)
    dev = CH.DevScene(sc)
    p.keep.append(dev)
    p.inp(dev.t[0], sc.pos, (sc.pos + np.array([3.0, 2.0], dtype=F)).astype(F))
    n = sc.cmds.shape[0]
    env.rt.raster_commands_reserve(ctx, n + 8, 1 << 14, 1 << 17)   # no VGX_E_GROWN
    return sc, dev, n


def _scene_tables(sc, dev):
    return (dev.t[3].data_ptr() if sc.cmds.shape[0] else None, sc.cmds.shape[0], None if dev.real is None else dev.real.data_ptr())


def _make_raster_commands(damaged):
    def make(env, ctx):
        import damage_model as DM
        import raster_harness as H
        torch, capi = env.torch, env.capi
        p = Plan()
        sc, dev, n = _scene(env, ctx, p)
        tgt = sc.target.with_clear(0xFF204060)
        image = p.out(torch.zeros((tgt.rows() + 2, tgt.stride), dtype=torch.int32, device="cuda:0"), used=tgt.rows() * tgt.stride * 4)
        st = status_word(p, env)
        t = tgt.struct(image.data_ptr())
        images = (dev.images.data_ptr() if sc.images else None, len(sc.images), None if dev.paints is None else C.byref(dev.paints.struct))
        if damaged:
            bits = H.DevBits(tgt.width, tgt.height, fill=DM.all_bits(tgt.width, tgt.height))
            dmg = capi.RasterDamage(bits.t.data_ptr(), 1 << 20, 0)
            p.keep.append(bits)

            def call():
                env.rt._check(env.lib.vgx_raster_commands_damaged(ctx.handle, C.byref(dev.streams), *_scene_tables(sc, dev), None, *images, C.byref(t), C.byref(dmg),
                                                                  st.data_ptr(), env.rt._stream_ptr()), "vgx_raster_commands_damaged")
        else:
            def call():
                env.rt._check(env.lib.vgx_raster_commands(ctx.handle, C.byref(dev.streams), *_scene_tables(sc, dev), *images, C.byref(t), st.data_ptr(),
                                                          env.rt._stream_ptr()), "vgx_raster_commands")
        p.call = call
        return p
    return make


def _grid_queries(env, tgt):
    q = np.zeros(192, dtype=env.capi.pick_cmd_query_dtype)
    j, i = np.mgrid[0:12, 0:16]
    q["x"] = (tgt.x0 + (i.reshape(-1) + 0.5) * tgt.width / 16.0).astype(F)
    q["y"] = (tgt.y0 + (j.reshape(-1) + 0.5) * tgt.height / 12.0).astype(F)
    q["cmd_end"] = q["tri_end"] = 0xFFFFFFFF
    return q


def _make_pick_commands(boxed):
    def make(env, ctx):
        torch = env.torch
        p = Plan()
        sc, dev, n = _scene(env, ctx, p)
        q = _grid_queries(env, sc.target)
        nq = q.shape[0]
        hits = p.out(torch.zeros((nq + 2) * 16, dtype=torch.uint8, device="cuda:0"), used=nq * 16)
        st = status_word(p, env)
        if boxed:   # true boxes of the real table; the decoy moves the queries, the boxes and the positions stay
            p.inputs = []
            boxes, st0 = env.rt.command_bounds(ctx, dev.streams, dev.t[3], n)
            torch.cuda.synchronize()
            assert int(st0.item()) == 0
            p.keep.append(boxes)
            e = q.copy()
            e["x"] += F(5.0)
            e["y"] += F(3.0)
            qd = p.new_inp(q, e)

            def call():
                env.rt._check(env.lib.vgx_pick_commands_boxed(ctx.handle, C.byref(dev.streams), *_scene_tables(sc, dev), boxes.data_ptr(), None, qd.data_ptr(), nq,
                                                              hits.data_ptr(), st.data_ptr(), env.rt._stream_ptr()), "vgx_pick_commands_boxed")
        else:
            qd = to_dev(q)
            p.keep.append(qd)

            def call():
                env.rt._check(env.lib.vgx_pick_commands(ctx.handle, C.byref(dev.streams), *_scene_tables(sc, dev), None, qd.data_ptr(), nq, hits.data_ptr(), st.data_ptr(),
                                                        env.rt._stream_ptr()), "vgx_pick_commands")
        p.call = call
        return p
    return make


def make_command_bounds(env, ctx):
    torch = env.torch
    p = Plan()
    sc, dev, n = _scene(env, ctx, p)
    boxes = p.out(torch.zeros((n + 2, 4), dtype=torch.float32, device="cuda:0"), used=n * 16)
    st = status_word(p, env)

    def call():
        env.rt._check(env.lib.vgx_command_bounds(ctx.handle, C.byref(dev.streams), *_scene_tables(sc, dev), 0, 0xFFFFFFFF, boxes.data_ptr(), st.data_ptr(),
                                                 env.rt._stream_ptr()), "vgx_command_bounds")
    p.call = call
    return p


def make_cmds_from_assembly(env, ctx):
    """A hand-made assembled frame: 40 commands of one mesh each over 40 draws; the decoy's draw states carry other scissors and colours."""
    torch, capi = env.torch, env.capi
    n = 40
    meshes = np.zeros(n, dtype=capi.mesh_dtype)
    meshes["draw"] = np.arange(n)
    meshes["num_vertices"], meshes["num_indices"] = 4, 6
    meshes["first_vertex"], meshes["first_index"] = 4 * np.arange(n), 6 * np.arange(n)

    def tables(k):
        dc = np.zeros(n, dtype=capi.drawcmd_dtype)
        dc["first_mesh"], dc["num_meshes"] = np.arange(n), 1
        dc["first_vertex"], dc["first_index"] = 4 * np.arange(n), 6 * np.arange(n)
        dc["num_vertices"], dc["num_indices"] = 4, 6
        ds = np.zeros(n, dtype=capi.draw_state_dtype)
        ds["scissor"] = np.array([k, 2 * k, 100 + k, 80 + k], dtype=np.uint16)
        ds["clip_first_draw"] = capi.CLIP_NONE
        ds["raw_color"] = 0xFF102030 + k
        return dc, ds
    (dc, ds), (dc2, ds2) = tables(0), tables(1)
    p = Plan()
    dcd, dsd = p.new_inp(dc, dc2), p.new_inp(ds, ds2)
    md = to_dev(meshes)
    p.keep.append(md)
    out = p.out(torch.zeros((n + 2) * capi.raster_cmd_dtype.itemsize, dtype=torch.uint8, device="cuda:0"), used=n * capi.raster_cmd_dtype.itemsize)
    num = p.out(torch.zeros(1, dtype=torch.int32, device="cuda:0"))
    st = status_word(p, env)
    draws = capi.RasterDraws(None, dsd.data_ptr(), n, 0)

    def call():
        env.rt._check(env.lib.vgx_raster_cmds_from_assembly(ctx.handle, dcd.data_ptr(), n, None, md.data_ptr(), n, C.byref(draws), out.data_ptr(), num.data_ptr(),
                                                            st.data_ptr(), env.rt._stream_ptr()), "vgx_raster_cmds_from_assembly")
    p.call = call
    return p


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, entry, make, cls=ASYNC, header=GENERAL, name=None, sensitivity=False, check_status=True):
        self.entry, self.make, self.cls, self.header = entry, make, cls, header
        self.name = name or entry
        self.sensitivity, self.check_status = sensitivity, check_status


CASES = [
    Row("vgx_flatten_count", make_flatten_count, HOST, "synchronises the stream once to read them back"),
    Row("vgx_flatten_emit", make_flatten_emit),
    Row("vgx_flatten", make_flatten, header="Single asynchronous call, the form for steady state"),
    Row("vgx_tessellate_count", make_tessellate_count, HOST, "returns totals (one stream sync)"),
    Row("vgx_tessellate_emit", make_tessellate_emit),
    Row("vgx_tessellate", make_tessellate, header="Single asynchronous call for steady state"),
    Row("vgx_tessellate", make_tessellate_assembly, header="Single asynchronous call for steady state", name="vgx_tessellate+assembly"),
    Row("vgx_tessellate_immediate", make_tessellate_immediate, header="Asynchronous: nothing on the host waits for the stream"),
    Row("vgx_stroke_count", make_stroke_count, HOST, "_count sizes the output (one stream sync)"),
    Row("vgx_stroke_emit", make_stroke_emit),
    Row("vgx_stroke", make_stroke, header="The same in ONE asynchronous call"),
    Row("vgx_dash_count", make_dash_count, HOST, "with one stream sync, and returns the batch's verdict"),
    Row("vgx_dash", make_dash, header="vgx_dash is the asynchronous steady-state form"),
    Row("vgx_subpath_draws", make_subpath_draws, header="All DEVICE pointers; asynchronous"),
    Row("vgx_tessellate_dashed", make_tessellate_dashed, header="The call never blocks"),
    Row("vgx_cache_localize", make_cache_localize),
    Row("vgx_cache_submit", make_cache_submit, header="Asynchronous like vgx_tessellate (capacities checked on the device"),
    Row("vgx_mesh_bounds", make_mesh_bounds, header="Asynchronous, no scratch of the context is used"),
    Row("vgx_cache_cull", make_cache_cull, header="Asynchronous; uses a small scratch of its own"),
    Row("vgx_pick", make_pick, header="Exactly nqueries hit records are written and nothing else of the caller's. Asynchronous"),
    Row("vgx_pick_rect", make_pick_rect, header="Asynchronous, no host round trip, a fixed number of kernels"),
    Row("vgx_raster", _make_raster("raster"), header="Nothing but pixels inside image and scissor and dev_status is written. Asynchronous. Uses scratch"),
    Row("vgx_raster_frame", _make_raster("frame")),
    Row("vgx_raster_textured", _make_raster("textured")),
    Row("vgx_raster_painted", _make_raster("painted")),
    Row("vgx_raster_concave", _make_raster("concave")),
    Row("vgx_pick_frame", make_pick_frame, header="Exactly nqueries hit records and dev_status are written, nothing else of the caller's. Asynchronous. Uses"),
    Row("vgx_cache_layout", make_cache_layout, header="Asynchronous; capacities are not checked (no frame is written)"),
    Row("vgx_cache_update", make_cache_update, header="writes nothing but VGX_OK to dev_status. Asynchronous"),
    Row("vgx_damage_meshes", make_damage_meshes, header="Asynchronous; scratch of their own"),
    Row("vgx_damage_instances", make_damage_instances, header="Asynchronous; scratch of their own"),
    Row("vgx_raster_damaged", _make_raster("damaged")),
    Row("vgx_raster_commands", _make_raster_commands(False), header="Nothing but pixels inside image and scissor and dev_status is written. Asynchronous. Scratch"),
    Row("vgx_raster_cmds_from_assembly", make_cmds_from_assembly),
    Row("vgx_pick_commands", _make_pick_commands(False), header="Exactly nqueries hit records and dev_status are written, nothing else of the caller's. Asynchronous. Scratch"),
    Row("vgx_command_bounds", make_command_bounds, header="Exactly the entries of the range and dev_status are written. Asynchronous"),
    Row("vgx_raster_commands_damaged", _make_raster_commands(True)),
    Row("vgx_pick_commands_boxed", _make_pick_commands(True)),
    Row("vgx_concave_move", make_concave_move, header="`moved` has the layout of contour_verts. Asynchronous"),
    Row("vgx_concave_emit", make_concave_emit, header="(not the moved ones). Asynchronous"),
    Row("vgx_concave_contours", make_concave_contours, header="Asynchronous, with the dev_sizes / dev_status protocol of vgx_concave_emit"),
    Row("vgx_merge", functools.partial(_merge, entry="vgx_merge"), header="the num_* members of `a` / `b` are host values. Asynchronous"),
    Row("vgx_merge_uv", functools.partial(_merge, entry="vgx_merge_uv")),
    Row("vgx_merge_uv_stream", functools.partial(_merge, entry="vgx_merge_uv_stream")),
    Row("vgx_text_quads", make_text_quads, header="Asynchronous like vgx_concave_emit / vgx_cache_submit"),
    Row("vgx_get_failure_info", make_failure_info, HOST, "Synchronises `stream`. Not needed on the happy path", check_status=False),
    Row("vgx_partition", make_partition, HOST, "Synchronises the stream."),
]

# The caller's mistake, on purpose: the entry on the null stream, the copies on S. The answer must then be the decoy's -- else the rows
# above could not see a launch that went to the wrong stream. The decoy is a valid input: nothing is provoked.
SENSITIVITY = [
    Row("vgx_tessellate_immediate", make_tessellate_immediate, name="sensitivity:vgx_tessellate_immediate", sensitivity=True),
    Row("vgx_pick", make_pick, name="sensitivity:vgx_pick", sensitivity=True),
    Row("vgx_raster", _make_raster("raster"), name="sensitivity:vgx_raster", sensitivity=True),
]
