"""Made-up mesh streams, and numpy models of what vgx_merge / vgx_merge_uv do with them (numpy only, no torch).

The entries that move finished meshes into a frame -- vgx_merge[_uv], vgx_cache_submit, vgx_cache_localize and the draw-command
assembly behind them -- need no tessellator: any packed stream of mesh records is a valid input, and the CPU oracle accepts the same
arrays. make_stream() writes such streams at any size, instances() the instance lists of a cached frame, merge_model() /
merge_uv_model() the merged frame (include/vgx.h: both sequences interleaved by draw, a mesh of `a` before a mesh of `b` of the same
draw). tests/test_mesh_streams_cpu.py pins the generator and the models, tests/test_gpu_mesh_streams.py runs the product on them."""
import functools
import importlib

import numpy as np

import pyoracle

capi = importlib.import_module("vg-renderer_amd.capi")

ALL_KINDS = (capi.MESH_FILL, capi.MESH_FILL_AA, capi.MESH_STROKE, capi.MESH_STROKE_AA, capi.MESH_STROKE_AA_THIN,
             capi.MESH_CONCAVE_FILL_AA, capi.MESH_TRILIST, capi.MESH_TEXT)  # every VGX_MESH_* of include/vgx.h
MAX_TRIANGLES = 43  # up to 129 indices per mesh: more than one pass of a wave, every remainder of the four-index copies


def _u32(rs, n):
    return rs.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def make_stream(rs, num_meshes, max_vertices, num_draws, kinds=ALL_KINDS, holes=False, num_vertices=None):
    """A pyoracle.MeshResult (pos, color, idx, meshes, sizes) of `num_meshes` random meshes, sorted by draw.
    num_vertices is random in [0, max_vertices] with about one mesh in ten forced to 0 (or the given array); num_indices is a random
    multiple of 3, odd and even, 0 below three vertices; indices are below the mesh's num_vertices; subpath_kind carries every kind
    of `kinds` in its top four bits over random low bits. Packed (every mesh directly behind its predecessor, what vgx_tessellate
    writes) unless holes: then 1-5 unowned vertices / indices sit in front of about half of the meshes and behind the last."""
    n = int(num_meshes)
    if num_vertices is None:
        nv = rs.randint(0, max_vertices + 1, size=n).astype(np.int64)
        nv[rs.uniform(size=n) < 0.1] = 0
    else:
        nv = np.asarray(num_vertices, dtype=np.int64)
        assert nv.shape == (n,)
    tri = rs.randint(1, MAX_TRIANGLES + 1, size=n).astype(np.int64)
    tri = np.minimum(tri, np.maximum(nv, 1))  # small meshes stay small, large ones do not grow an index stream to match
    ni = np.where(nv >= 3, 3 * tri, 0)
    gap_v, gap_i = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    if holes:
        gap_v = rs.randint(1, 6, size=n + 1) * (rs.uniform(size=n + 1) < 0.5)
        gap_i = rs.randint(1, 6, size=n + 1) * (rs.uniform(size=n + 1) < 0.5)
        gap_v[n], gap_i[n] = max(int(gap_v[n]), 1), max(int(gap_i[n]), 1)
    r = pyoracle.MeshResult()
    m = np.zeros(n, dtype=capi.mesh_dtype)
    m["first_vertex"] = np.cumsum(nv + gap_v[:n]) - nv
    m["first_index"] = np.cumsum(ni + gap_i[:n]) - ni
    m["num_vertices"], m["num_indices"] = nv, ni
    m["draw"] = np.sort(rs.randint(0, max(int(num_draws), 1), size=n))
    k = np.asarray(kinds, dtype=np.uint32)[np.arange(n) % len(kinds)]
    rs.shuffle(k)
    m["subpath_kind"] = (k << np.uint32(28)) | (_u32(rs, n) & np.uint32(0x0FFFFFFF))
    tv, ti = int(nv.sum() + gap_v.sum()), int(ni.sum() + gap_i.sum())
    r.pos = rs.uniform(-1000.0, 1000.0, size=(tv, 2)).astype(np.float32)
    r.color = _u32(rs, tv)
    r.idx = rs.randint(0, 1 << 16, size=ti).astype(np.uint16)  # unowned indices keep these values
    owner = np.repeat(np.arange(n), ni)
    at = np.repeat(m["first_index"].astype(np.int64) - (np.cumsum(ni) - ni), ni) + np.arange(int(ni.sum()))
    r.idx[at] = np.floor(rs.uniform(size=owner.shape[0]) * np.minimum(nv[owner], 65536)).astype(np.uint16)  # a uint16 reaches no further
    r.meshes = m
    r.sizes = {"num_vertices": tv, "num_indices": ti, "num_meshes": n}
    return r


def repack(src, keep):
    """The meshes src.meshes[keep] (a mask or an index array, order kept) as a packed stream of their own."""
    m = src.meshes[keep].copy()
    nv, ni = m["num_vertices"].astype(np.int64), m["num_indices"].astype(np.int64)
    ov, oi = np.cumsum(nv) - nv, np.cumsum(ni) - ni
    gv = np.repeat(m["first_vertex"].astype(np.int64) - ov, nv) + np.arange(int(nv.sum()))
    gi = np.repeat(m["first_index"].astype(np.int64) - oi, ni) + np.arange(int(ni.sum()))
    r = pyoracle.MeshResult()
    r.pos, r.color, r.idx = src.pos[gv].copy(), src.color[gv].copy(), src.idx[gi].copy()
    m["first_vertex"], m["first_index"] = ov, oi
    r.meshes = m
    r.sizes = {"num_vertices": int(nv.sum()), "num_indices": int(ni.sum()), "num_meshes": int(m.shape[0])}
    return r


def merge_model(a, b, b_draw=None):
    """vgx_merge(a, b, b_draw) as include/vgx.h states it: a stable sort by draw of concat(a, b) -- `a` in front, so that a mesh of `a`
    wins a tie --, streams gathered mesh by mesh, records renumbered, draw of b's meshes from b_draw when given. The result also
    carries .order: for every merged mesh its index in concat(a, b) (>= a's mesh count: a mesh of b)."""
    na = a.meshes.shape[0]
    mb = b.meshes.copy()
    if b_draw is not None:
        mb["draw"] = np.asarray(b_draw, dtype=np.uint32)
    mb["first_vertex"] += np.uint64(a.pos.shape[0])
    mb["first_index"] += np.uint64(a.idx.shape[0])
    both = pyoracle.MeshResult()
    both.meshes = np.concatenate([a.meshes, mb])
    both.pos, both.color, both.idx = np.concatenate([a.pos, b.pos]), np.concatenate([a.color, b.color]), np.concatenate([a.idx, b.idx])
    order = np.argsort(both.meshes["draw"], kind="stable")
    r = repack(both, order)
    r.order = order
    r.num_a = na
    return r


def merge_uv_model(merged_order, a, b, b_uv, white, uv_bytes):
    """The UV stream of the merged frame as uint32 words [vertices, uv_bytes / 4]: the white value everywhere (what the assembly step
    writes), b_uv's rows over the vertices of b's meshes. white: the raw words; b_uv: [b's vertices, uv_bytes / 4] uint32."""
    words = uv_bytes // 4
    na = a.meshes.shape[0]
    m = np.concatenate([a.meshes, b.meshes])[merged_order]
    nv = m["num_vertices"].astype(np.int64)
    out_first = np.cumsum(nv) - nv
    uv = np.empty((int(nv.sum()), words), dtype=np.uint32)
    uv[:] = np.asarray(white[:words], dtype=np.uint32)
    from_b = merged_order >= na
    nb_, fb, ob = nv[from_b], m["first_vertex"][from_b].astype(np.int64), out_first[from_b]
    span = np.arange(int(nb_.sum()))
    uv[np.repeat(ob, nb_) + span - np.repeat(np.cumsum(nb_) - nb_, nb_)] = b_uv[np.repeat(fb, nb_) + span - np.repeat(np.cumsum(nb_) - nb_, nb_)]
    return uv


def draw_records(rs, num_draws):
    """vgx_draw records of which only state_key matters: runs of 1-40 draws share a key, neighbouring runs differ, and with four keys
    in all some runs return to an earlier key."""
    d = np.zeros(num_draws, dtype=capi.draw_dtype)
    d["mtx"][:] = [1, 0, 0, 1, 0, 0]
    keys = (0x11, 0x2222, 0x333333, 0x44444444)
    k, cur = 0, -1
    while k < num_draws:
        run = int(rs.randint(1, 41))
        cur = int(rs.choice([x for x in range(4) if x != cur]))
        d["state_key"][k:k + run] = keys[cur]
        k += run
    return d


def instances(rs, cache_nm, n, empties=True):
    """n vgx_cache_instance records over a cache of cache_nm meshes: ranges of 0-4 meshes, random colours, random rotations and
    scales with one all-zero linear part. With empties: the first three instances, the last two and [250, 520) when n > 520 have
    empty ranges, one of them with first_mesh == cache_nm."""
    inst = np.zeros(n, dtype=capi.cache_instance_dtype)
    first = rs.randint(0, cache_nm + 1, size=n).astype(np.int64)
    num = np.minimum(rs.randint(0, 5, size=n), cache_nm - first)
    if empties:
        num[:3] = 0
        num[max(n - 2, 0):] = 0
        if n > 520:
            num[250:520] = 0
        if n > 1:
            first[1] = cache_nm
    inst["first_mesh"], inst["num_meshes"] = first, num
    inst["color"] = _u32(rs, n)
    ang, sx, sy = rs.uniform(0, 6.28, size=n), rs.uniform(0.25, 3.0, size=n), rs.uniform(0.25, 3.0, size=n)
    mtx = np.stack([sx * np.cos(ang), sx * np.sin(ang), -sy * np.sin(ang), sy * np.cos(ang), rs.uniform(-500, 500, size=n), rs.uniform(-500, 500, size=n)], axis=1)
    inst["mtx"] = mtx.astype(np.float32)
    if n:
        k = int(np.flatnonzero(num > 0)[0]) if np.any(num > 0) else n // 2
        inst["mtx"][k][:4] = 0  # every vertex of the instance lands on its translation
    return inst


def instance_totals(cache, inst):
    """(meshes, vertices, indices) of the frame of `inst`, from the records alone."""
    m = cache.meshes
    sel = np.repeat(inst["first_mesh"].astype(np.int64), inst["num_meshes"]) + np.arange(int(inst["num_meshes"].sum())) \
        - np.repeat(np.cumsum(inst["num_meshes"].astype(np.int64)) - inst["num_meshes"], inst["num_meshes"])
    return int(sel.shape[0]), int(m["num_vertices"][sel].sum()), int(m["num_indices"][sel].sum())


# ---- the cached frames both test files use: (instances, vertices per cache mesh at most) ------------------------------------------
CACHE_MESHES = 200
CACHE_FRAMES = ((1024, 40), (1025, 40), (131073, 12))
CACHE_MAX_VB = 4096


@functools.lru_cache(maxsize=None)
def cache_frame(ninst):
    """(cache, instances, reference frame) of the listed frame with `ninst` instances; computed once, shared, not to be changed.
    The reference frame is None where the oracle does not accept the instance list (its status is asserted inside pyoracle)."""
    maxv = dict(CACHE_FRAMES)[ninst]
    rs = np.random.RandomState(7000 + ninst % 1000)
    cache = make_stream(rs, CACHE_MESHES, maxv, 1)
    inst = instances(rs, CACHE_MESHES, ninst)
    try:
        ref = pyoracle.cache_submit(cache, inst)
    except AssertionError as e:  # pyoracle asserts `st == 0, st`: only the oracle's own verdict makes a frame a left-out one
        if not (e.args and isinstance(e.args[0], int) and e.args[0] != 0):
            raise
        ref = None
    return cache, inst, ref


def left_out():
    """The listed frames the oracle does not accept (vgo_cache_submit, or vgo_assemble at CACHE_MAX_VB): what the oracle leaves out,
    the GPU tests leave out. tests/test_mesh_streams_cpu.py asserts that there are none."""
    out = []
    for ninst, _ in CACHE_FRAMES:
        ref = cache_frame(ninst)[2]
        if ref is None or pyoracle.assemble(ref.meshes, ref.idx, CACHE_MAX_VB)[0] != 0:
            out.append(ninst)
    return out


# ---- the merge inputs both test files use ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_case(n, kind="ties"):
    """(a, b, b_draw, draws) with n meshes of 0-6 vertices in all: 700 in `a` up to n = 1 025, else split 3:1; about n / 8 draws.
    kind "ties": both sides draw from all the draws, so most draws have meshes on both sides; "a_first" / "b_first": every draw of one
    side below every draw of the other; "draw7": every mesh of both has draw 7. From 40 000 meshes on `b` has holes; above 500 000
    b_draw is given and b's own draw field is scrambled. draws: the frame's vgx_draw records (state keys). Shared: do not change."""
    rs = np.random.RandomState(n % 100003 + 17 * len(kind))
    na = min(n, 700) if n <= 1025 else n * 3 // 4
    nb = n - na
    nd = max(n // 8, 8)
    holes = n >= 40000
    if kind == "ties":
        a, b = make_stream(rs, na, 6, nd), make_stream(rs, nb, 6, nd, holes=holes)
    elif kind in ("a_first", "b_first"):
        a, b = make_stream(rs, na, 6, nd // 2), make_stream(rs, nb, 6, nd // 2, holes=holes)
        (b if kind == "a_first" else a).meshes["draw"] += np.uint32(nd // 2)
    else:
        assert kind == "draw7"
        a, b = make_stream(rs, na, 6, 1), make_stream(rs, nb, 6, 1, holes=holes)
        a.meshes["draw"], b.meshes["draw"] = 7, 7
    b_draw = None
    if n > 500000:
        b_draw = b.meshes["draw"].copy()
        b.meshes["draw"] = _u32(rs, nb)
    return a, b, b_draw, draw_records(rs, nd)
