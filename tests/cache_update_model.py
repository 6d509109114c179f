"""vgx_cache_layout / vgx_cache_update: a numpy statement of both specifications in include/vgx.h, the inputs the CPU and GPU tests
share, and the assertions both make on what the product wrote (tests/test_cache_update_cpu.py: the lane code through
libvgx_hosttest.so; tests/test_gpu_cache_update.py: the kernels). Both test files hand a `backend` to the check_* functions below, so
they carry the same assertions by construction.

The truth is the reference: for a list of edited instances, oracle.cache_submit(cache, mixed) with mixed = the submitted array inst0
where the listed (and admitted) entries are replaced from the edited array inst1. Positions of instances with a finite matrix compare
as bit patterns, those of the nan / inf instances as "equal, or NaN in both" (x86 and the GPU produce different NaN payloads), colours
exactly. Inputs come from tests/cache_cull_model.py, which stays as it is.

A backend provides:
  layout(c, inst, guard)                 -> (status, slots[ninst + 1 + guard] as capi.cache_slot_dtype; the guard entries pattern-filled)
  frame(c, inst0, ref0)                  -> a frame object: the inst0 frame inside pattern-filled guard regions, with a box table that
                                            vgx_mesh_bounds computed for it (also inside guards)
  update(fr, c, inst, slots, dirty, limit, with_bounds, num_vertices=None) -> status   (limit: None, or the value behind dev_ndirty)
  read(fr)                               -> (pos [nv, 2], color [nv], bounds [nm, 4], guards_intact, others_intact)
                                            others_intact: idx and the mesh table are byte-equal to what they were before the update
"""
import functools

import numpy as np

import cache_cull_model as M

capi = M.capi
oracle = M.oracle
F = np.float32
# the issue's scenes, whose caches hold AA meshes only, and one of this file's own: 'plain', the Tiger with two draws of three non-AA,
# so that the rule "non-AA meshes take the instance's colour, AA meshes keep theirs" has both kinds to act on
SCENES = [("tiger", 1), ("tiger", 65), ("tiger", 257), ("walk", 1), ("walk", 65), ("plain", 65)]
GUARD = 5
SLOT_PATTERN = 0xA5A5A5A5A5A5A5A5


# ---- the specification, in numpy -----------------------------------------------------------------------------------------
def cache_first(cache, k, what):
    nm = cache.meshes.shape[0]
    if k < nm:
        return int(cache.meshes[what][k])
    return cache.pos.shape[0] if what == "first_vertex" else cache.idx.shape[0]


def range_counts(cache, a, k):
    """(valid, meshes, vertices, indices) of the mesh range [a, a + k) of the cache; a range outside it counts nothing."""
    nm = cache.meshes.shape[0]
    if a > nm or k > nm - a:
        return False, 0, 0, 0
    return (True, k, cache_first(cache, a + k, "first_vertex") - cache_first(cache, a, "first_vertex"),
            cache_first(cache, a + k, "first_index") - cache_first(cache, a, "first_index"))


def layout_model(cache, inst):
    """vgx_cache_layout: (status, slots [ninst + 1])."""
    n = inst.shape[0]
    slots = np.zeros(n + 1, dtype=capi.cache_slot_dtype)
    status = capi.VGX_OK
    m = v = x = 0
    for i in range(n):
        ok, km, kv, kx = range_counts(cache, int(inst["first_mesh"][i]), int(inst["num_meshes"][i]))
        if not ok:
            status = capi.VGX_E_INVALID_ARG
        slots[i] = (m, v, x, int(inst["first_mesh"][i]))
        m, v, x = m + km, v + kv, x + kx
    slots[n] = (m, v, x, 0)
    return status, slots


def xform_all(mtx, p):
    """v2xform over an array of points, one binary32 rounding per operation."""
    m = mtx.astype(F)
    x, y = p[:, 0].astype(F), p[:, 1].astype(F)
    with np.errstate(all="ignore"):
        return np.stack([F(F(F(m[0] * x) + F(m[2] * y)) + m[4]), F(F(F(m[1] * x) + F(m[3] * y)) + m[5])], axis=1).astype(F)


def update_model(cache, inst, slots, dirty, limit, pos, color, num_vertices, num_meshes, bounds):
    """vgx_cache_update on numpy arrays, in place (bounds may be None). Returns (status, the set of instances that were written)."""
    n = inst.shape[0]
    nlist = dirty.shape[0] if limit is None else min(dirty.shape[0], int(limit))
    invalid = stale = False
    written = set()
    for d in [int(x) for x in dirty[:nlist]]:
        if d >= n:
            invalid = True
            continue
        a, k = int(inst["first_mesh"][d]), int(inst["num_meshes"][d])
        ok, km, kv, _ = range_counts(cache, a, k)
        if not ok:
            invalid = True
            continue
        s0, s1 = slots[d], slots[d + 1]
        if (a != int(s0["cache_first_mesh"]) or km != int(s1["first_mesh"]) - int(s0["first_mesh"])
                or kv != int(s1["first_vertex"]) - int(s0["first_vertex"])):
            stale = True
            continue
        if int(s1["first_vertex"]) > num_vertices or int(s1["first_mesh"]) > num_meshes:
            invalid = True
            continue
        written.add(d)
        v0, o0 = cache_first(cache, a, "first_vertex"), int(s0["first_vertex"])
        pos[o0:o0 + kv] = xform_all(inst["mtx"][d], cache.pos[v0:v0 + kv])
        for j in range(k):
            me = cache.meshes[a + j]
            off, nv = int(me["first_vertex"]) - v0, int(me["num_vertices"])
            if (int(me["subpath_kind"]) >> 28) in (capi.MESH_FILL, capi.MESH_STROKE):
                color[o0 + off:o0 + off + nv] = inst["color"][d]
            if bounds is not None:
                q = pos[o0 + off:o0 + off + nv]
                with np.errstate(all="ignore"):
                    bounds[int(s0["first_mesh"]) + j] = [q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()] if nv else M.EMPTY
    status = capi.VGX_E_INVALID_ARG if invalid else (capi.VGX_E_STALE if stale else capi.VGX_OK)
    return status, written


# ---- inputs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """M.case for 'tiger' / 'walk'; 'plain': the same Tiger recorded with the AA flag cleared on two draws of three (fills and strokes)."""
    if name != "plain":
        return M.case(name)
    t = M.case("tiger")
    c = M.Case()
    c.name, c.ps = name, t.ps
    d = t.draws.copy()
    sel = np.arange(d.shape[0]) % 3 != 0
    d["fill_flags"][sel] &= ~np.uint32(capi.FILL_AA)
    d["stroke_flags"][sel] &= ~np.uint32(capi.STROKE_AA)
    c.draws = d
    c.cache = oracle.cache_localize(d, oracle.tessellate(c.ps, d))
    c.nm = c.cache.meshes.shape[0]
    c.mesh_boxes = M.mesh_boxes(c.cache.pos, c.cache.meshes)
    c.box = np.array([c.mesh_boxes[:, 0].min(), c.mesh_boxes[:, 1].min(), c.mesh_boxes[:, 2].max(), c.mesh_boxes[:, 3].max()], dtype=F)
    c.extent = float(max(c.box[2] - c.box[0], c.box[3] - c.box[1]))
    c.pitch = 1.25 * c.extent
    return c


@functools.lru_cache(maxsize=None)
def arrays(name, n):
    """(case, inst0, inst1): the submitted array and the edited one -- the same structure, mtx and color from another seed."""
    c = case(name)
    inst0, _ = M.make_instances(c, n) if name == "plain" else M.scene(name, n)[1:3]
    other, _ = M.make_instances(c, n, seed=6)
    inst1 = inst0.copy()
    inst1["mtx"], inst1["color"] = other["mtx"], other["color"]
    return c, inst0, inst1


def whole_drawing(c, inst):
    """An instance to list alone: the first with the largest mesh range (a whole Tiger where the array has one)."""
    return int(np.argmax(inst["num_meshes"])) if inst.shape[0] else 0


LIST_KINDS = ("empty", "one", "k63", "k64", "k65", "all", "shuffled", "twice", "limit", "many")
LAYOUT_SCENES = SCENES + [("tiger", 5000)]  # more than 1 024 instances: the scan's three-pass form


def list_kinds(n):
    """'many' (more than 1 024 entries: the list scan's three-pass form) needs a frame whose every instance listed five times is that long."""
    return [k for k in LIST_KINDS if not (k[0] == "k" and k[1:].isdigit() and int(k[1:]) > n) and not (k == "many" and 5 * n <= 1024)]


def dirty_list(name, n, kind):
    """(dirty uint32 array, limit or None): limit is the value behind dev_ndirty."""
    c, inst0, _ = arrays(name, n)
    perm = np.random.RandomState(100 + n).permutation(n).astype(np.uint32)
    if kind == "empty":
        return np.zeros(0, dtype=np.uint32), None
    if kind == "one":
        return np.array([whole_drawing(c, inst0)], dtype=np.uint32), None
    if kind in ("k63", "k64", "k65"):
        return perm[:int(kind[1:])].copy(), None
    if kind == "all":
        return np.arange(n, dtype=np.uint32), None
    if kind == "shuffled":
        return perm.copy(), None
    if kind == "twice":  # every index twice, the copies apart from each other
        return np.concatenate([perm, perm[::-1]]), None
    if kind == "many":
        return np.tile(perm, 5), None
    assert kind == "limit"
    return perm.copy(), max(n // 2, 0)


def mix(inst0, inst1, listed):
    out = inst0.copy()
    for d in listed:
        out[d] = inst1[d]
    return out


class Ref:
    pass


_refs = {}


def reference(c, mixed):
    """The reference's frame of `mixed`, its per-vertex owner and (lazily) its mesh boxes; computed once per distinct array."""
    key = (c.name, mixed.tobytes())
    if key not in _refs:
        r = Ref()
        r.frame = oracle.cache_submit(c.cache, mixed)
        r.mesh_owner = r.frame.meshes["draw"].astype(np.int64)
        r.owner = np.repeat(r.mesh_owner, r.frame.meshes["num_vertices"].astype(np.int64))
        r.fin = M.finite_mask(mixed)
        r._boxes = None
        _refs[key] = r
    return _refs[key]


def ref_boxes(r):
    if r._boxes is None:
        with np.errstate(all="ignore"):
            r._boxes = M.mesh_boxes(r.frame.pos, r.frame.meshes)
    return r._boxes


def ref_slots(frame, inst):
    """What slots must be, read off the reference frame's mesh table: the first mesh with draw == i, for an empty instance its
    successor's values, the totals at the end."""
    n = inst.shape[0]
    out = np.zeros(n + 1, dtype=capi.cache_slot_dtype)
    out[n] = (frame.meshes.shape[0], frame.pos.shape[0], frame.idx.shape[0], 0)
    first = {}
    for m in range(frame.meshes.shape[0] - 1, -1, -1):
        first[int(frame.meshes["draw"][m])] = m
    for i in range(n - 1, -1, -1):
        if i in first:
            m = first[i]
            out[i] = (m, int(frame.meshes["first_vertex"][m]), int(frame.meshes["first_index"][m]), int(inst["first_mesh"][i]))
        else:
            out[i] = (int(out["first_mesh"][i + 1]), int(out["first_vertex"][i + 1]), int(out["first_index"][i + 1]), int(inst["first_mesh"][i]))
    return out


# ---- the assertions on what the product wrote ----------------------------------------------------------------------------
def same_or_nan(a, b):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_frame(pos, color, r):
    """pos / color against the reference frame r: bit patterns for the vertices of finite instances, equal-or-NaN for the others."""
    fv = r.fin[r.owner]
    assert pos.shape == r.frame.pos.shape and color.shape == r.frame.color.shape
    assert np.array_equal(pos[fv].view(np.uint32), r.frame.pos[fv].view(np.uint32))
    assert same_or_nan(pos[~fv], r.frame.pos[~fv])
    assert np.array_equal(color.view(np.uint32), r.frame.color.view(np.uint32))


def check_slots(backend, name, n):
    c, inst0, _ = arrays(name, n)
    r0 = reference(c, inst0)
    st, got = backend.layout(c, inst0, GUARD)
    assert st == capi.VGX_OK
    assert np.array_equal(got[:n + 1].view(np.uint64), ref_slots(r0.frame, inst0).view(np.uint64))
    assert np.all(got[n + 1:].view(np.uint64) == SLOT_PATTERN)
    return got[:n + 1].copy()


def check_layout_invalid(backend):
    """A range outside the cache contributes zero and sets VGX_E_INVALID_ARG; the slots are those of the array with that range empty."""
    c, inst0, _ = arrays("tiger", 65)
    bad = inst0.copy()
    bad["first_mesh"][5], bad["num_meshes"][5] = c.nm - 1, 2
    bad["first_mesh"][9], bad["num_meshes"][9] = c.nm + 1, 0
    st, got = backend.layout(c, bad, GUARD)
    assert st == capi.VGX_E_INVALID_ARG
    emptied = bad.copy()
    emptied["first_mesh"][[5, 9]], emptied["num_meshes"][[5, 9]] = 0, 0
    want = ref_slots(reference(c, emptied).frame, bad)
    assert np.array_equal(got[:66].view(np.uint64), want.view(np.uint64))
    ms, mslots = layout_model(c.cache, bad)
    assert ms == st and np.array_equal(mslots.view(np.uint64), got[:66].view(np.uint64))


def check_dirty_list(backend, name, n, kind):
    """One update of the inst0 frame with one dirty list, with mesh_bounds: frame, boxes, guards, everything else."""
    c, inst0, inst1 = arrays(name, n)
    r0 = reference(c, inst0)
    _, slots = layout_model(c.cache, inst0)
    dirty, limit = dirty_list(name, n, kind)
    listed = set(int(d) for d in (dirty if limit is None else dirty[:limit]))
    if kind in ("all", "shuffled", "twice", "many"):
        assert listed == set(range(n))
    r1 = reference(c, mix(inst0, inst1, listed))
    fr = backend.frame(c, inst0, r0)
    _, _, before, _, _ = backend.read(fr)
    assert M.boxes_equal(before[r0.fin[r0.mesh_owner]], ref_boxes(r0)[r0.fin[r0.mesh_owner]])  # the table the update starts from
    st = backend.update(fr, c, inst1, slots, dirty, limit, True)
    assert st == capi.VGX_OK
    pos, color, bounds, guards, others = backend.read(fr)
    assert guards and others
    assert_frame(pos, color, r1)
    # boxes: the meshes of finite instances against the true boxes of the mixed frame; unlisted instances keep their bytes
    fm = r1.fin[r1.mesh_owner]
    assert M.boxes_equal(bounds[fm], ref_boxes(r1)[fm])
    unlisted = ~np.isin(r1.mesh_owner, np.array(sorted(listed), dtype=np.int64))
    assert np.array_equal(bounds[unlisted].view(np.uint32), before[unlisted].view(np.uint32))
    if kind == "limit":
        assert 0 < len(listed) < n or n == 1
    return fr, r1


def check_without_bounds(backend, name, n):
    """mesh_bounds == NULL: the frame is updated, the table is not touched."""
    c, inst0, inst1 = arrays(name, n)
    r0 = reference(c, inst0)
    _, slots = layout_model(c.cache, inst0)
    dirty, _ = dirty_list(name, n, "shuffled")
    fr = backend.frame(c, inst0, r0)
    _, _, before, _, _ = backend.read(fr)
    assert backend.update(fr, c, inst1, slots, dirty, None, False) == capi.VGX_OK
    pos, color, bounds, guards, others = backend.read(fr)
    assert guards and others
    assert_frame(pos, color, reference(c, mix(inst0, inst1, range(n))))
    assert np.array_equal(bounds.view(np.uint32), before.view(np.uint32))


def error_case(what):
    """(inst, dirty, expected status, the listed instances that must be written) on the tiger-65 arrays."""
    c, inst0, inst1 = arrays("tiger", 65)
    ed = inst1.copy()
    one = [i for i in range(65) if int(inst0["num_meshes"][i]) == 1][:2]
    threes = [i for i in range(65) if int(inst0["num_meshes"][i]) == 3 and np.isfinite(inst0["mtx"][i]).all()]
    three, good = threes[:1], [whole_drawing(c, inst0)] + threes[1:3]
    assert len(one) == 2 and len(good) == 3 and not set(good) & set(one + three)
    moved, shrunk = one[0], three[0]
    stale = []
    if what in ("stale", "both"):
        ed["first_mesh"][moved] = (int(ed["first_mesh"][moved]) + 1) % c.nm  # another valid 1-mesh range
        ed["num_meshes"][shrunk] = 2
        stale = [moved, shrunk]
    dirty = list(good[:2]) + stale + ([65, 4000000000] if what in ("range", "both") else []) + good[2:]
    status = {"range": capi.VGX_E_INVALID_ARG, "stale": capi.VGX_E_STALE, "both": capi.VGX_E_INVALID_ARG}[what]
    return ed, np.array(dirty, dtype=np.uint32), status, good


def check_errors(backend, what):
    """Offending entries keep their old bytes (frame and boxes), every other listed slice is updated, the status is deterministic."""
    c, inst0, inst1 = arrays("tiger", 65)
    r0 = reference(c, inst0)
    _, slots = layout_model(c.cache, inst0)
    ed, dirty, status, good = error_case(what)
    fr = backend.frame(c, inst0, r0)
    _, _, before, _, _ = backend.read(fr)
    assert backend.update(fr, c, ed, slots, dirty, None, True) == status
    pos, color, bounds, guards, others = backend.read(fr)
    assert guards and others
    r1 = reference(c, mix(inst0, inst1, good))  # the structure of inst0: the offenders were not written
    assert_frame(pos, color, r1)
    fm = r1.fin[r1.mesh_owner]
    assert M.boxes_equal(bounds[fm], ref_boxes(r1)[fm])
    unlisted = ~np.isin(r1.mesh_owner, np.array(good, dtype=np.int64))
    assert np.array_equal(bounds[unlisted].view(np.uint32), before[unlisted].view(np.uint32))
    # the same list the other way round: the same status, the same frame
    fr2 = backend.frame(c, inst0, r0)
    assert backend.update(fr2, c, ed, slots, dirty[::-1].copy(), None, True) == status
    pos2, color2, bounds2, guards, others = backend.read(fr2)
    assert guards and others
    assert_frame(pos2, color2, r1)
    assert np.array_equal(bounds2.view(np.uint32), bounds.view(np.uint32))


def check_short_frame(backend):
    """frame->num_vertices smaller than a slice's end: VGX_E_INVALID_ARG, that slice is not written, the others are. The same for
    frame->num_meshes through the model only (the backends pass the real mesh count)."""
    c, inst0, inst1 = arrays("tiger", 65)
    r0 = reference(c, inst0)
    _, slots = layout_model(c.cache, inst0)
    listed = [i for i in range(65) if int(inst0["num_meshes"][i])][-4:]
    last = listed[-1]
    short = int(slots["first_vertex"][last + 1]) - 1
    assert all(int(slots["first_vertex"][d + 1]) <= short for d in listed[:-1])
    fr = backend.frame(c, inst0, r0)
    assert backend.update(fr, c, inst1, slots, np.array(listed, dtype=np.uint32), None, True, num_vertices=short) == capi.VGX_E_INVALID_ARG
    pos, color, bounds, guards, others = backend.read(fr)
    assert guards and others
    r1 = reference(c, mix(inst0, inst1, listed[:-1]))
    assert_frame(pos, color, r1)
    fm = r1.fin[r1.mesh_owner]
    assert M.boxes_equal(bounds[fm], ref_boxes(r1)[fm])
