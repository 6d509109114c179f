"""Named, deterministic batches for the immediate-mode sequence tests (helper, not collected).

vgx_tessellate_immediate picks the route of a call from what the LAST call with the same tag found, tag = (path set generation, number
of draws). The kinds below therefore share one path set of 3 072 fuzz paths and, unless said otherwise, have 3 072 draws: their tags
collide, and a batch runs on the period, distinct-path count, polyline vertices and command instances of whatever came before it.
Every kind is generated (nothing stored); tests/test_immediate_kinds_cpu.py pins, from the reference alone, the property of each kind
that steers the route, tests/test_gpu_immediate_sequences.py runs them.
"""
import importlib

import numpy as np

SEED = 4130
NPATHS = 3072
NDRAWS = 3072

# kinds on the shared path set, from same-size ones to the _big ones (the order the transition matrix runs in)
SHARED = ["periodic64", "periodic48", "shuffled64", "broken_last", "broken_first", "fill_only64", "nothing", "p96x32", "periodic64_small",
          "unique", "p96x31", "frame2048", "large2049", "periodic64_big", "unique_big"]
ERRORS = ["empty", "nan_draw"]  # shared path set too; not part of the matrix
OWN = ["cubics_long", "cubics_short", "thin", "tiger10"]  # path sets of their own
ALL = SHARED + ERRORS + OWN

# What each kind is built to have (checked against the reference by test_immediate_kinds_cpu.py): number of draws, the smallest period
# of its paths (0: none below the number of draws), distinct paths used, and which side of 10 polyline vertices per command instance.
#             ndraws period distinct long_curves
PROPS = {
    "periodic64":       (3072, 64, 64, True),
    "periodic48":       (3072, 48, 48, True),
    "shuffled64":       (3072, 0, 64, True),
    "broken_last":      (3072, 0, 65, True),
    "broken_first":     (3072, 0, 65, True),
    "fill_only64":      (3072, 64, 64, True),
    "nothing":          (3072, 64, 64, True),
    "p96x32":           (3072, 96, 96, True),
    "periodic64_small": (3072, 64, 64, False),
    "unique":           (3072, 0, 3072, True),
    "p96x31":           (2976, 96, 96, True),
    "frame2048":        (2048, 0, 2048, True),
    "large2049":        (2049, 0, 2049, True),
    "periodic64_big":   (3072, 64, 64, True),
    "unique_big":       (3072, 0, 3072, True),
    "cubics_long":      (4096, 0, 4096, True),
    "cubics_short":     (4096, 0, 4096, False),
    "thin":             (3072, 64, 64, False),
    "tiger10":          (2400, 240, 240, False),
}

MIN_INSTANCES, SMALL_DRAWS = 32, 2048  # VGX_INST_MIN_INSTANCES, VGX_SMALL_DRAWS (written down, not imported: see test_immediate_kinds_cpu.py)


def route_from_knowledge(ndraws, period, distinct, long_curves):
    """The route of vgx_tessellate_immediate (vgx_route_choose, csrc/vgx_route_plan.h) for a batch of `ndraws` draws whose tag is known, from
    the mirrored knowledge: period usable -> paths reused -> long curves (vertices >= 10 x command instances) -> k_flatten_build."""
    if ndraws <= SMALL_DRAWS:
        return "route_frame"
    if period and ndraws % period == 0 and ndraws // period >= MIN_INSTANCES:
        return "route_periodic"
    if distinct and ndraws // distinct >= MIN_INSTANCES:
        return "route_grouped"
    return "route_one_walk" if long_curves else "route_build"


# The route a kind runs on once the context knows it (second call onwards on a fresh context): the table the sequence tests assert.
# test_immediate_kinds_cpu.py checks it against route_from_knowledge(*PROPS[kind]).
LEARNED = {
    "periodic64": "route_periodic", "periodic48": "route_periodic", "fill_only64": "route_periodic", "nothing": "route_periodic",
    "p96x32": "route_periodic", "periodic64_small": "route_periodic", "periodic64_big": "route_periodic",
    "shuffled64": "route_grouped", "broken_last": "route_grouped", "broken_first": "route_grouped",
    "unique": "route_one_walk", "unique_big": "route_one_walk", "p96x31": "route_one_walk", "large2049": "route_one_walk",
    "frame2048": "route_frame",
    "cubics_long": "route_one_walk", "cubics_short": "route_build", "thin": "route_periodic", "tiger10": "route_build",
}


def collide(a, b):
    """Same path set and same number of draws: one tag."""
    return make(a)[0] is make(b)[0] and PROPS[a][0] == PROPS[b][0]


def first_call_route(a, b):
    """The route of the FIRST call of kind b on a context whose last immediate batch was kind a (run until it was known): a's learned
    route when the tags collide -- b runs on a's period, distinct-path count, vertices and command instances --, else a new tag."""
    if PROPS[b][0] <= SMALL_DRAWS:
        return "route_frame"
    return LEARNED[a] if collide(a, b) else "route_build"


_cache = {}


def _wl():
    return importlib.import_module("vg-renderer_amd.workloads")


def _capi():
    return importlib.import_module("vg-renderer_amd.capi")


def shared_paths():
    if "_ps" not in _cache:
        _cache["_ps"] = _wl().fuzz_paths(SEED, npaths=NPATHS, with_shapes=True, degenerate=True)
    return _cache["_ps"]


def _unique():
    """Draw i -> path i, general stroke styles (all caps and joins, AA and not, hairlines)."""
    if "_unique" not in _cache:
        _cache["_unique"] = _wl().fuzz_draws(shared_paths(), SEED, ndraws=NDRAWS)
    return _cache["_unique"]


def _periodic(P, n=NDRAWS):
    """Draws i -> path i % P, the per-path draw fields of `unique` tiled; every instance under its own translation."""
    d = np.tile(_unique()[:P], n // P)
    inst = np.arange(n) // P
    d["mtx"][:, 4] += (37.0 * (inst % 10)).astype(np.float32)
    d["mtx"][:, 5] += (41.0 * (inst // 10)).astype(np.float32)
    return d


def _scaled(d, f):
    """Transform and `scale` times f (the stroke widths stay)."""
    d = d.copy()
    f = np.float32(f)
    d["mtx"][:, :4] *= f
    d["scale"] *= f
    return d


def _other_path(d, i):
    """The path of draw i changed to one that no other draw of a periodic64 batch uses (draw fields kept)."""
    d = d.copy()
    d["path"][i] = 1000 + i % 7
    return d


def _own_set(name):
    wl, capi = _wl(), _capi()
    if name in ("cubics_long", "cubics_short"):
        ps, d = wl.random_cubics(4096, seed=99, box=10000.0)
        d = d.copy()
        d["fill_flags"] = 0
        d["stroke_flags"] = capi.stroke_flags(capi.CAP_BUTT, capi.JOIN_MITER)
        d["stroke_width"] = 2.0
        return ps, (d if name == "cubics_long" else _scaled(d, 0.004))
    if name == "thin":
        ps = wl.thin_fuzz_paths(SEED, npaths=64)
        return ps, np.tile(wl.fuzz_draws(ps, SEED), 48)
    assert name == "tiger10"
    return wl.tiger(10)


def make(name):
    """(PathSetArrays, draws) of a kind. Kinds of SHARED and ERRORS return the same PathSetArrays object."""
    if name in _cache:
        return _cache[name]
    if name in OWN:
        r = _own_set(name)
    else:
        ps = shared_paths()
        if name == "unique":
            d = _unique()
        elif name == "periodic64":
            d = _periodic(64)
        elif name == "periodic48":
            d = _periodic(48)
        elif name == "shuffled64":
            d = _periodic(64)[np.random.RandomState(SEED).permutation(NDRAWS)]
        elif name == "broken_last":
            d = _other_path(_periodic(64), NDRAWS - 1)
        elif name == "broken_first":
            d = _other_path(_periodic(64), 5)
        elif name == "periodic64_big":
            d = _scaled(_periodic(64), 12.0)
        elif name == "unique_big":
            d = _scaled(_unique(), 12.0)
        elif name == "periodic64_small":
            d = _scaled(_periodic(64), 0.05)
        elif name == "fill_only64":
            d = _periodic(64)
            d["stroke_flags"] = 0
        elif name == "nothing":
            d = _periodic(64)
            d["stroke_flags"] = 0
            d["fill_flags"] = 0
        elif name == "p96x32":
            d = _periodic(96)
        elif name == "p96x31":
            d = _periodic(96, 2976)
        elif name == "frame2048":
            d = _unique()[:2048].copy()
        elif name == "large2049":
            d = _unique()[:2049].copy()
        elif name == "empty":
            d = _unique()[:0].copy()
        elif name == "nan_draw":
            d = _periodic(64)
            d["mtx"][1234, 2] = np.float32("nan")
        else:
            raise KeyError(name)
        r = (ps, d)
    _cache[name] = r
    return r


def period_of(paths):
    """Smallest P < len with paths == tile(paths[:P]) (P divides len); 0 when there is none."""
    n = paths.shape[0]
    for P in range(1, n):
        if n % P == 0 and np.array_equal(paths, np.tile(paths[:P], n // P)):
            return P
    return 0


_refs = {}


def reference(oracle, name):
    """oracle.tessellate of a kind, computed once per process."""
    if name not in _refs:
        ps, d = make(name)
        _refs[name] = oracle.tessellate(ps, d)
    return _refs[name]
