"""CPU: dashed strokes in frames (vgx_tessellate_dashed) without a device.
  1. the fixture condition of the reference model for every fixture the GPU tests compare against it;
  2. the worked square of include/vgx.h with a fill and [4,2] phase 1 through the model: one fill mesh, then 7 stroke meshes, all
     with sub-path index 0;
  3. the slot arithmetic of csrc/vgx_dashframe.h (vgxt_dashframe_ranks of libvgx_hosttest.so) against the model's interleave on the
     fuzz seeds, and on hand cases;
  4. examples/vgx_dashed_frame_example.cpp compiles and links against libvgx.so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dash_util as U
import dashed_frame_fixtures as F
import dashed_frame_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = U.capi


def ranks(dashed, piece_src):
    lib = U.hosttest()
    lib.vgxt_dashframe_ranks.restype = C.c_uint64
    lib.vgxt_dashframe_ranks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    dashed = np.ascontiguousarray(dashed, dtype=np.uint8)
    piece_src = np.ascontiguousarray(piece_src, dtype=np.uint32)
    kept = np.zeros(max(dashed.shape[0], 1), np.uint64)
    piece = np.zeros(max(piece_src.shape[0], 1), np.uint64)
    n = lib.vgxt_dashframe_ranks(dashed.ctypes.data if dashed.size else None, dashed.shape[0], piece_src.ctypes.data if piece_src.size else None,
                                 piece_src.shape[0], kept.ctypes.data, piece.ctypes.data)
    return int(n), kept[:dashed.shape[0]], piece[:piece_src.shape[0]]


def sequential_slots(dashed, piece_src):
    """The interleave written as the loop it replaces."""
    kept, piece, k, p = [], [0] * len(piece_src), 0, 0
    for m, f in enumerate(dashed):
        if not f:
            kept.append(k); k += 1
            continue
        kept.append(2 ** 64 - 1)
        while p < len(piece_src) and piece_src[p] == m:
            piece[p] = k; k += 1; p += 1
    assert p == len(piece_src)
    return k, kept, piece


@pytest.fixture(scope="module")
def fixtures(wl, vgr):
    return F.model_fixtures(wl, vgr)


@pytest.mark.parametrize("k", range(6))
def test_fixture_condition(oracle, fixtures, k):
    name, ps, d, dashes, pattern = fixtures[k]
    c = DM.fixture_condition(oracle, ps, d, dashes, pattern)
    print("%s: %d pieces, smallest end-segment distSqr %.3g" % (name, c["pieces"], c["smallest"]))
    assert c["pieces"] > 0
    assert (c["epsilon"], c["negative_zeros"], c["short"], c["not_returned"]) == (0, 0, 0, 0), (name, c)


def test_worked_square(oracle, wl, vgr):
    b = vgr.PathSetBuilder()
    b.begin_path()
    for i, (x, y) in enumerate(((0, 0), (10, 0), (10, 10), (0, 10))):
        (b.move_to if i == 0 else b.line_to)(float(x), float(y))
    b.close()
    b.end_path()
    d = wl.make_draws(1)
    wl.set_fill(d, 0, 0xFF112233, aa=True)
    wl.set_stroke(d, 0, 0xFF445566, 2.0, capi.CAP_BUTT, capi.JOIN_MITER, aa=True)
    dashes, pattern = U.make_dashes([([4.0, 2.0], 1.0)])
    fr = DM.frame(oracle, b.arrays(), d, dashes, pattern)
    kinds = (fr.meshes["subpath_kind"] >> 28).tolist()
    assert kinds == [capi.MESH_FILL_AA] + [capi.MESH_STROKE_AA] * 7
    assert np.all((fr.meshes["subpath_kind"] & 0x0FFFFFFF) == 0) and np.all(fr.meshes["draw"] == 0)
    assert fr.dash_sizes["num_subpaths"] == 7 and fr.dash_sizes["num_poly_vertices"] == 16
    assert np.array_equal(fr.meshes["first_vertex"], np.cumsum(fr.meshes["num_vertices"]) - fr.meshes["num_vertices"])


@pytest.mark.parametrize("seed", F.FUZZ_SEEDS)
def test_ranks_equal_the_models_interleave(oracle, wl, seed):
    _, ps, d, dashes, pattern = F.fuzz(wl, seed)
    fr = DM.frame(oracle, ps, d, dashes, pattern)
    src = oracle.tessellate(ps, d).meshes  # what the flatten stage describes: every mesh of the undashed frame
    is_dashed = ((src["subpath_kind"] >> 28) >= capi.MESH_STROKE) & DM.dashed_mask(d, dashes)[src["draw"]]
    where = {(int(m["draw"]), int(m["subpath_kind"]) & 0x0FFFFFFF): i for i, m in enumerate(src) if is_dashed[i]}
    piece_src = np.array([where[(int(a), int(b))] for a, b in zip(fr.piece_draw, fr.piece_src_sub)], dtype=np.uint32)
    assert np.all(np.diff(piece_src.astype(np.int64)) >= 0)
    n, kept, piece = ranks(is_dashed, piece_src)
    assert n == fr.meshes.shape[0]
    pos = {o: k for k, o in enumerate(fr.order)}
    assert [int(x) for x in kept[~is_dashed]] == [pos[(0, j)] for j in range(fr.a_meshes.shape[0])]
    assert [int(x) for x in piece] == [pos[(1, p)] for p in range(piece_src.shape[0])]
    assert int(is_dashed.sum()) > 0 and piece_src.shape[0] > int(is_dashed.sum())


HAND = {
    "a draw with zero pieces between two dashed ones": ([0, 1, 0, 1, 0, 1, 0], [1, 1, 1, 5, 5]),
    "fill-only": ([0, 0, 0], []),
    "stroke-only, all dashed": ([1, 1, 1], [0, 0, 1, 2, 2, 2]),
    "neither": ([], []),
    "first and last draw dashed": ([1, 0, 0, 1], [0, 0, 3]),
    "first and last draw dashed, no pieces": ([1, 0, 0, 1], []),
    "dashed neighbours, the first without pieces": ([0, 1, 1, 0], [2, 2]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_ranks_hand_cases(name):
    dashed, src = HAND[name]
    want = sequential_slots(dashed, src)
    n, kept, piece = ranks(dashed, src)
    assert (n, [int(x) for x in kept], [int(x) for x in piece]) == want


def test_ranks_random():
    rng = np.random.default_rng(7)
    for _ in range(50):
        m = int(rng.integers(1, 200))
        dashed = (rng.random(m) < 0.4).astype(np.uint8)
        counts = np.where(dashed != 0, rng.integers(0, 6, m), 0)
        src = np.repeat(np.arange(m, dtype=np.uint32), counts)
        want = sequential_slots(dashed.tolist(), src.tolist())
        n, kept, piece = ranks(dashed, src)
        assert (n, [int(x) for x in kept], [int(x) for x in piece]) == want


def test_example_compiles_and_links(tmp_path):
    exe = str(tmp_path / "vgx_dashed_frame_example")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_dashed_frame_example.cpp"),
                           "-L", os.path.join(ROOT, "vg-renderer_amd"), "-lvgx", "-Wl,-rpath," + os.path.join(ROOT, "vg-renderer_amd"), "-o", exe])
    assert os.path.exists(exe)
