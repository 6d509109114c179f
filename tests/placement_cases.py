"""The inputs of tests/test_gpu_output_placement.py, their reference answers (computed once, shared, never modified) and the
conditions the placement tests need of them: a stream that ends in the middle of a 16-byte word and meshes that start in one.
No GPU here: tests/test_guarded_streams_cpu.py checks the conditions on the reference's sizes beforehand.

Seeds (recorded here, chosen so that the conditions hold): FUZZ_SEED for the small fuzz drawing of routes a / b / g and the template
batches of route e, ROUND_SEED / CLASS_SEED / SCENE_SEED for the Round-join, three-class and static-batch templates, IMM_SEED for
the batch of route f, the seeds of tests/mesh_streams.py's merge_case(1025) / cache_frame(1025), SMALL_SEED for the 3-mesh
streams of route h and CONCAVE_SEEDS / CONCAVE_SMALL_SEED for its concave fills."""
import functools
import importlib

import numpy as np

import mesh_streams as MS
import transform_extremes as tx

wl = importlib.import_module("vg-renderer_amd.workloads")
capi = importlib.import_module("vg-renderer_amd.capi")

FUZZ_SEED = 900
ROUND_SEED = 3995
CLASS_SEED = 973
SCENE_SEED = 11
IMM_SEED = 300
SMALL_SEED = 1
TMPL_INSTANCES = 33   # odd: instance count and totals are odd multiples where the drawing allows
FRAME_INSTANCES = 3   # of the fuzz drawing: 216 draws, far below the sizes at which tile_emit / tmpl_emit take a batch
SCENE_INSTANCES = 13  # tigers of the shuffled scene: just above 2 048 draws after culling

ROUTES = {
    "a": ("fuzz3", "tiger1"),
    "b": ("fuzz3", "tiger1"),
    "c": ("closed40", "closed39"),
    "d": ("walks", "walks_after_fill"),
    "e": ("tmpl_miter", "tmpl_round", "tmpl_classes", "tmpl_static"),
    "f": ("imm_fuzz",),
    "g": ("asm_fuzz3", "asm_tmpl"),
}


def _state_keys(d, seed):
    """Runs of 7 draws per state, three states (as tests/test_gpu_tmpl.py's assembly tests)."""
    rs = np.random.RandomState(seed)
    d["state_key"] = np.repeat(rs.randint(0, 3, size=(d.shape[0] + 6) // 7), 7)[:d.shape[0]].astype(np.uint32)
    return d


def scene(ninst, seed):
    """tests/test_gpu_tmpl.py's _scene: an instanced scene after culling and reordering -- no period left."""
    ps, ops = wl.tiger_paths()
    d = wl.tiger_draws(ops, ninst, join=0)
    rs = np.random.RandomState(seed)
    d = d[rs.uniform(size=d.shape[0]) < 0.7]
    return ps, d[rs.permutation(d.shape[0])]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(path set, draws) of a named input. Shared: do not change."""
    if name in ("fuzz3", "asm_fuzz3", "tmpl_miter", "asm_tmpl"):
        ps = wl.closed_fuzz_paths(FUZZ_SEED, npaths=72)
        d = wl.template_draws(ps, FUZZ_SEED, FRAME_INSTANCES if name.endswith("fuzz3") else TMPL_INSTANCES)
        return ps, (_state_keys(d, FUZZ_SEED) if name.startswith("asm") else d)
    if name == "tiger1":
        return wl.tiger(1)
    if name == "closed40":
        ps, d, _ = tx.closed_case("miter")
        return ps, d
    if name == "closed39":  # forty instances give even totals whatever the drawing: the first 39 of them give odd ones
        ps, d, _ = tx.closed_case("miter")
        return ps, d[:39 * ps.npaths].copy()
    if name == "walks":
        return tx.case("walks", "identity")
    if name == "walks_after_fill":
        # every stroke mesh of the walks has an even number of vertices: a plain (non-AA) fill of the first walk in front, 401
        # vertices, makes every stroke mesh start at an odd vertex and the totals odd. Its polyline is as long as the strokes'.
        ps, d = tx.case("walks", "identity")
        f = tx.vgr.make_draws(1)
        f["path"] = 0
        f["mtx"][:] = d["mtx"][0]
        wl.set_fill(f, 0, 0xFF3060C0, aa=False)
        return ps, np.concatenate([f, d])
    if name == "tmpl_round":
        ps = wl.fuzz_paths(ROUND_SEED, npaths=72, with_shapes=True, degenerate=False)
        return ps, wl.template_general_draws(ps, ROUND_SEED, TMPL_INSTANCES, round_joins=True)
    if name == "tmpl_classes":
        ps = wl.closed_fuzz_paths(CLASS_SEED, npaths=72)
        d, pick = wl.template_class_draws(ps, CLASS_SEED, TMPL_INSTANCES, 3)
        assert len(set(pick.tolist())) == 3
        return ps, d
    if name == "tmpl_static":
        return scene(SCENE_INSTANCES, SCENE_SEED)
    if name == "imm_fuzz":
        ps = wl.fuzz_paths(IMM_SEED, npaths=96)
        return ps, wl.fuzz_draws(ps, IMM_SEED)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's answer (with its flattened polylines: route f feeds them to vgx_stroke). Shared: do not change."""
    import pyoracle
    assert pyoracle.available("reference"), "oracle/_ref/libvgref.so (the reference compiled from its own sources) is what these cases are pinned on"
    if name == "closed40":
        return tx.reference("closed", "miter", "counted")
    if name == "walks":
        return tx.reference("walks", "identity")
    ps, d = inputs(name)
    return pyoracle.tessellate(ps, d, kind="reference", want_flat=True)


# ---- route h: the copying entries on made-up streams -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_inputs(which):
    """(a, b, b_draw, merged model). "slices": merge_case(1025), the smallest of tests/mesh_streams.py past one scan slice (1 024
    meshes); "three": 3 meshes in all."""
    if which == "slices":
        a, b, b_draw, _ = MS.merge_case(1025)
    else:
        rs = np.random.RandomState(SMALL_SEED)
        a, b, b_draw = MS.make_stream(rs, 2, 0, 3, num_vertices=[5, 7]), MS.make_stream(rs, 1, 0, 3, num_vertices=[9]), None
    return a, b, b_draw, MS.merge_model(a, b, b_draw)


@functools.lru_cache(maxsize=None)
def submit_inputs(which):
    """(cache, instances, reference frame). "slices": cache_frame(1025); "three": a cache of 3 meshes, 5 instances."""
    import pyoracle
    if which == "slices":
        return MS.cache_frame(1025)
    rs = np.random.RandomState(SMALL_SEED)
    cache = MS.make_stream(rs, 3, 0, 1, num_vertices=[5, 7, 9])
    inst = MS.instances(rs, 3, 5, empties=False)
    return cache, inst, pyoracle.cache_submit(cache, inst)


CONCAVE_SEEDS = range(100, 259)  # tests/test_gpu_concave.py's random fills of these seeds, one behind the other: 1 025 fills
CONCAVE_SMALL_SEED = 104         # the first three fills of this seed: 129 + 115 + 123 vertices


@functools.lru_cache(maxsize=None)
def concave_fills(which):
    """The fills vgx_concave_emit gets: "slices": more than one scan slice (1 024 items) of them; "three": three. Made-up mesh
    streams cannot feed this entry (its input is contours and the caller's libtess2 passes), so the fills are those of
    tests/test_gpu_concave.py. Shared: do not change."""
    import test_gpu_concave as TC
    if which == "three":
        return tuple(TC._random_fills(CONCAVE_SMALL_SEED)[:3])
    out = []
    for seed in CONCAVE_SEEDS:
        out += TC._random_fills(seed)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def concave_reference(which):
    """(nv, ni, mesh records) of the reference's meshes of concave_fills(which), packed one behind the other. No GPU."""
    import pyoracle
    import test_gpu_concave as TC
    lib = TC.load_ref(pyoracle)
    refs = [TC._reference_mesh(lib, c, col, fr, eo) for (c, col, fr, eo) in concave_fills(which)]
    m = np.zeros(len(refs), dtype=capi.mesh_dtype)
    nv = np.array([r[0].shape[0] for r in refs], dtype=np.int64)
    ni = np.array([r[2].shape[0] for r in refs], dtype=np.int64)
    m["num_vertices"], m["num_indices"] = nv, ni
    m["first_vertex"], m["first_index"] = np.cumsum(nv) - nv, np.cumsum(ni) - ni
    return int(nv.sum()), int(ni.sum()), m


# ---- the conditions ---------------------------------------------------------------------------------------------------------------------
def conditions(nv, ni, meshes):
    """Which of the three conditions an output of nv vertices, ni indices and the given mesh records meets."""
    return {"odd_vertices": nv % 2 == 1, "index_bytes_off_16": (2 * ni) % 16 != 0,
            "odd_first_vertex": bool(np.any((meshes["first_vertex"] % 2 == 1) & (meshes["num_vertices"] > 0)))}


def route_conditions(outputs):
    """outputs: (nv, ni, meshes) per parametrisation of a route. Every condition must hold in at least one of them."""
    met = {}
    for nv, ni, meshes in outputs:
        for k, v in conditions(int(nv), int(ni), meshes).items():
            met[k] = met.get(k, False) or v
    return met


def assert_route(route, outputs):
    met = route_conditions(outputs)
    assert all(met.values()), (route, met)


def of_ref(ref):
    return ref.sizes["num_vertices"], ref.sizes["num_indices"], ref.meshes


def of_stream(r):
    return r.pos.shape[0], r.idx.shape[0], r.meshes
