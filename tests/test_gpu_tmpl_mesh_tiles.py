"""GPU: template mode's tiles end at mesh boundaries (csrc/vgx_tmpl_plan.h: a tile boundary that falls inside a mesh of at most
tile / 8 elements moves down to that mesh's first element; k_tmpl_mesh_lmax / k_tmpl_classes / k_tmpl_elems), and the caller's mesh
table is written from three words parked in LDS (tmpl_mesh_out_parts). One period of 70 lineTo polygons whose lengths sit around
every threshold of the rule at tile sizes 64, 128 and 2048 (the snap limits 8, 16, 256; the tile sizes themselves; meshes longer than
a tile, which stay cut and keep the cross-tile loads), 33 instances under their own rotation, scale and translation. Positions,
colours, indices and every record of the mesh table: byte for byte the ordinary pipeline's (VGX_TMPL=0) and the reference's."""
import importlib

import numpy as np
import pytest

from util import assert_mesh_equal, bytes_equal
from test_gpu_tmpl import _run, _assembled, MODE_TEMPLATE, VGX_E_STALE

pytestmark = pytest.mark.gpu

LENGTHS = [3, 4, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 2047, 2048, 2049, 5000]
NINST = 33
NDRAWS = 70
MAX_VB = 65536  # vertices per vertex buffer with assembly armed (the longest mesh, 5000 points, has 10 000)


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


def _lengths():
    """70 sub-path lengths from LENGTHS: the four beyond a tile once each (they carry most of the vertices), the others in turn."""
    short = [n for n in LENGTHS if n < 2047]
    out = [short[k % len(short)] for k in range(NDRAWS - 4)]
    for at, n in ((5, 5000), (22, 2047), (40, 2048), (58, 2049)):  # spread over the period, short meshes on both sides
        out.insert(at, n)
    assert len(out) == NDRAWS and set(out) == set(LENGTHS)
    return out


def _paths(open_strokes=False):
    """One polygon (moveTo + lineTos [+ close]) per path: points on a circle, about one unit apart. open_strokes: the stroked paths
    (every third) stay open."""
    pm = importlib.import_module("vg-renderer_amd.pathset")
    rs = np.random.RandomState(31)
    b = pm.PathSetBuilder()
    for k, n in enumerate(_lengths()):
        r = max(4.0, n / (2.0 * np.pi))
        cx, cy = rs.uniform(-300, 300, size=2)
        ang = np.arange(n) * (2.0 * np.pi / n) + rs.uniform(0, 1)
        b.begin_path()
        b.move_to(cx + r * np.cos(ang[0]), cy + r * np.sin(ang[0]))
        for a in ang[1:]:
            b.line_to(cx + r * np.cos(a), cy + r * np.sin(a))
        if not (open_strokes and k % 3 == 0):
            b.close()
        b.end_path()
    return b.arrays()


def _draws(rt, wl, ninst=NINST, join=None, scales=(1.0,)):
    """Every sub-path filled (AA); every third one stroked closed Miter (`join`: another join), alternating AA and Thin. Instance k
    takes scales[k % len(scales)] (more than one: classes) and a rotation, scale and translation of its own."""
    join = rt.capi.JOIN_MITER if join is None else join
    rs = np.random.RandomState(32)
    per = []
    for sc in scales:
        one = wl.make_draws(NDRAWS)
        one["path"] = np.arange(NDRAWS, dtype=np.uint32)
        one["scale"] = np.float32(sc)
        for i in range(NDRAWS):
            wl.set_fill(one, i, 0xFF000000 | (i * 0x030507 & 0xFFFFFF), aa=True)
            if i % 3 == 0:
                wl.set_stroke(one, i, 0xC0000000 | (i * 0x070305 & 0xFFFFFF), 3.0 if (i // 3) % 2 == 0 else 0.6, rt.capi.CAP_BUTT, join, aa=True, avg_scale=sc)
        per.append(one)
    d = np.concatenate([per[k % len(per)] for k in range(ninst)])
    ang = rs.uniform(0, 2 * np.pi, size=ninst)
    s = rs.uniform(0.6, 1.6, size=ninst)
    t = rs.uniform(-500, 500, size=(ninst, 2))
    m = d["mtx"].reshape(ninst, NDRAWS, 6)
    m[:, :, 0] = (np.cos(ang) * s)[:, None]; m[:, :, 1] = (np.sin(ang) * s)[:, None]
    m[:, :, 2] = (-np.sin(ang) * s)[:, None]; m[:, :, 3] = (np.cos(ang) * s)[:, None]
    m[:, :, 4] = t[:, 0, None]; m[:, :, 5] = t[:, 1, None]
    return d


class _Batch:
    pass


@pytest.fixture(scope="module")
def batch(rt, wl, oracle):
    """The batch, the reference's output and the ordinary pipeline's (VGX_TMPL=0) for it: computed once, read by every tile size."""
    import os
    b = _Batch()
    b.ps = _paths()
    b.d = _draws(rt, wl)
    assert b.d.shape[0] > 2048 and b.d.shape[0] // NDRAWS >= 32
    b.ref = oracle.tessellate(b.ps, b.d)
    assert 1_200_000 < b.ref.sizes["num_vertices"] < 2_400_000, b.ref.sizes
    b.old = _ordinary(rt, b.ps, b.d)
    return b


def _ordinary(rt, ps, d, static=False):
    import os
    saved = os.environ.get("VGX_TMPL")
    os.environ["VGX_TMPL"] = "0"
    try:
        ctx = rt.Context(0)
        old = _run(rt, ctx, ps, d)
        ctx.close()
    finally:
        if saved is None:
            del os.environ["VGX_TMPL"]
        else:
            os.environ["VGX_TMPL"] = saved
    assert old.mode != MODE_TEMPLATE and "tmpl_emit" not in old.stages and old.status == 0
    return old


def _same_bytes(got, old, what):
    for k in ("pos", "color", "idx", "meshes"):
        assert bytes_equal(getattr(got, k), getattr(old, k)), (what, k)


@pytest.mark.parametrize("tile", ["64", "128", None])
def test_tiles_at_mesh_boundaries_equal_ordinary_pipeline_and_reference(rt, batch, monkeypatch, tile):
    """Tile 64: lengths up to 8 lie whole in a tile, 9 and up are cut (the 300 among them); tile 128: up to 16; the default tile: up
    to 256, the 257 / 300 / 2047 / 2048 / 2049 / 5000 are cut -- the cross-tile path runs at every size."""
    if tile:
        monkeypatch.setenv("VGX_TMPL_TILE", tile)
    ctx = rt.Context(0)
    got = _run(rt, ctx, batch.ps, batch.d)
    ctx.close()
    assert got.mode == MODE_TEMPLATE and got.stages == ["tmpl_emit"], (got.mode, got.stages)  # template mode really ran
    assert got.status == 0
    assert int(got.dev_sizes[3]) == batch.ref.sizes["num_vertices"] and int(got.dev_sizes[4]) == batch.ref.sizes["num_indices"]
    assert_mesh_equal(got, batch.ref, "mesh tiles, tile=%s" % tile)
    _same_bytes(got, batch.old, "mesh tiles, tile=%s" % tile)


def test_tiles_at_mesh_boundaries_two_classes(rt, wl, oracle, batch, monkeypatch):
    """The same period at two scales: two classes, each with tiles (and a stride) of its own."""
    monkeypatch.setenv("VGX_TMPL_TILE", "64")
    d = _draws(rt, wl, scales=(1.0, 2.0))
    ref = oracle.tessellate(batch.ps, d)
    ctx = rt.Context(0)
    got = _run(rt, ctx, batch.ps, d)
    ctx.close()
    assert got.mode == MODE_TEMPLATE and got.stages == ["tmpl_emit"] and got.status == 0, (got.mode, got.stages, got.status)
    assert_mesh_equal(got, ref, "mesh tiles, two classes")
    _same_bytes(got, _ordinary(rt, batch.ps, d), "mesh tiles, two classes")


def test_tiles_at_mesh_boundaries_static_batch(rt, oracle, batch, monkeypatch):
    """A shuffled 70 % of the draws has no period: with vgx_set_static_batches one template of one instance."""
    monkeypatch.setenv("VGX_TMPL_TILE", "64")
    rs = np.random.RandomState(33)
    d = batch.d[rs.uniform(size=batch.d.shape[0]) < 0.7]
    d = d[rs.permutation(d.shape[0])]
    ref = oracle.tessellate(batch.ps, d)
    ctx = rt.Context(0)
    ctx.set_static_batches(True)
    got = _run(rt, ctx, batch.ps, d)
    ctx.close()
    assert got.mode == MODE_TEMPLATE and got.stages == ["tmpl_emit"] and got.status == 0, (got.mode, got.stages, got.status)
    assert_mesh_equal(got, ref, "mesh tiles, static batch")
    _same_bytes(got, _ordinary(rt, batch.ps, d), "mesh tiles, static batch")


def test_tiles_at_mesh_boundaries_with_draw_command_assembly(rt, oracle, batch, monkeypatch):
    """Assembly armed: indices carry their mesh's base inside its draw command; commands and streams == the ordinary pipeline's."""
    monkeypatch.setenv("VGX_TMPL_TILE", "64")
    d = batch.d.copy()
    d["state_key"] = (np.arange(d.shape[0]) // 11).astype(d["state_key"].dtype)
    ctx = rt.Context(0)
    got = _assembled(rt, ctx, batch.ps, d, MAX_VB, True)
    ctx.close()
    assert got.mode == MODE_TEMPLATE and got.stages[-1] == "tmpl_emit" and "assemble" in got.stages, (got.mode, got.stages)
    assert got.status == 0
    monkeypatch.setenv("VGX_TMPL", "0")
    ctx = rt.Context(0)
    old = _assembled(rt, ctx, batch.ps, d, MAX_VB, True)
    ctx.close()
    assert old.mode != MODE_TEMPLATE and old.status == 0
    assert got.ncmd == old.ncmd and bytes_equal(got.cmds, old.cmds)
    _same_bytes(got, old, "mesh tiles, assembly")
    keys = d["state_key"][batch.ref.meshes["draw"]]
    st, rcmds, ridx = oracle.assemble(batch.ref.meshes, batch.ref.idx, MAX_VB, mesh_keys=keys)
    assert st == 0 and rcmds.shape[0] == got.ncmd
    assert np.array_equal(got.idx, ridx)


@pytest.mark.parametrize("style", ["open_butt", "bevel"])
def test_tiles_at_mesh_boundaries_open_and_bevel_kernels(rt, wl, oracle, monkeypatch, style):
    """The stroked sub-paths open with Butt caps (k_tmpl_emit_open) / closed with Bevel joins (k_tmpl_emit_bevel): the same tables."""
    monkeypatch.setenv("VGX_TMPL_TILE", "64")
    ps = _paths(open_strokes=style == "open_butt")
    d = _draws(rt, wl, join=rt.capi.JOIN_BEVEL if style == "bevel" else None)
    ref = oracle.tessellate(ps, d)
    ctx = rt.Context(0)
    got = _run(rt, ctx, ps, d)
    ctx.close()
    assert got.mode == MODE_TEMPLATE and got.stages == ["tmpl_emit"] and got.status == 0, (got.mode, got.stages, got.status)
    assert_mesh_equal(got, ref, "mesh tiles, " + style)
    _same_bytes(got, _ordinary(rt, ps, d), "mesh tiles, " + style)


def test_tiles_at_mesh_boundaries_still_verify_every_draw(rt, batch, monkeypatch):
    """Two draws of one instance swapped after the count: the tiles' draw ranges still cover the period -- VGX_E_STALE."""
    monkeypatch.setenv("VGX_TMPL_TILE", "64")
    ctx = rt.Context(0)
    for a, b in ((1, 2), (0, NDRAWS - 1), (30, 31)):  # short neighbours (inside one tile), the period's ends, around a long mesh
        d3 = batch.d.copy()
        i, j = 19 * NDRAWS + a, 19 * NDRAWS + b
        d3[[i, j]] = d3[[j, i]]
        got = _run(rt, ctx, batch.ps, batch.d, d_steady=d3)
        assert got.mode == MODE_TEMPLATE and got.status == VGX_E_STALE, (a, b, got.status)
    ctx.close()
