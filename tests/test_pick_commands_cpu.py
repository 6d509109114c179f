"""CPU: the lane code of vgx_pick_commands (csrc/vgx_pick_cmds.h through libvgx_hosttest.so: vgxt_pick_commands, a plain loop over
queries, commands and triangles) against the numpy statement of the specification (tests/pick_commands_model.py), against the IMAGE of the
ID table (relation (a) of include/vgx.h: a check that does not rest on the model's walk), against the model of vgx_pick_frame on the
one-mesh-per-command frame (relation (b)), the owner search against a brute-force loop, the statuses and the host refusals. Exact
everywhere, in all four words of every hit; the GPU suite (tests/test_gpu_pick_commands.py) makes the same comparisons on the kernels."""
import ctypes as C

import numpy as np
import pytest

import pick_commands_harness as PH
import pick_commands_model as PC
import pick_frame_model as PF
import raster_commands_harness as CH
import raster_commands_model as CM

capi = PC.capi
NONE = PC.NONE
OK, BAD, RANGE = PH.OK, PH.BAD, PH.RANGE


@pytest.fixture(scope="module")
def host():
    return PH.load_host()


@pytest.mark.parametrize("name", sorted(PH.SCENES))
def test_lane_code_equals_model(host, name):
    sc, (q, _) = PH.scene(name), PH.query_set(name)
    PH.check_conditions(name)
    want = PH.expected(name)
    got = PH.host_pick(host, sc, q, PH.owner_table(name))
    assert PH.same(got, want.hits), PH.differences(got, want.hits, q)
    # without owners: the same commands and triangles, mesh = draw = none
    bare = PH.host_pick(host, sc, q)
    assert np.array_equal(bare["cmd"], got["cmd"]) and np.array_equal(bare["triangle"], got["triangle"])
    assert (bare["mesh"] == NONE).all() and (bare["draw"] == NONE).all()


def test_limits_inside_a_command(host):
    """tri_end at 0, in the middle of a chunk, at both chunk boundaries and behind the end: the answer is the largest covering triangle
    below the limit, and the model's stack holds it."""
    sc, q = PH.scene("limits"), PH.limit_queries()
    want = PC.pick(sc, q)
    got = PH.host_pick(host, sc, q)
    assert PH.same(got, want.hits), PH.differences(got, want.hits, q)
    PH.check_limit_answers(sc, q, got)


@pytest.mark.parametrize("name", [n for n in sorted(PH.SCENES) if n not in PH.NAN_SCENES])
def test_relation_b_equals_pick_frame(host, name):
    """With tri_end = 0 the words cmd and triangle are mesh and triangle of vgx_pick_frame on the equivalent frame."""
    sc, (q, _) = PH.scene(name), PH.query_set(name)
    q = q[(q["tri_end"] == 0) & (q["reserved"] == 0)]
    f = CM.equivalent_frame(sc)
    want = PF.pick(f, PC.frame_queries(q))
    assert want.status == OK
    got = PH.host_pick(host, sc, q)
    assert np.array_equal(got["cmd"], want.hits["mesh"]) and np.array_equal(got["triangle"], want.hits["triangle"])
    assert (got["cmd"] != NONE).any()


@pytest.fixture(scope="module")
def id_images():
    """The model's image of every scene's ID table, rendered once."""
    out = {}
    for name in sorted(PH.SCENES):
        ids, _ = PC.id_scene(PH.scene(name))
        assert CM.status(ids) == OK
        out[name] = CM.render(ids)
    return out


@pytest.mark.parametrize("name", sorted(PH.SCENES))
def test_relation_a_the_image_is_the_oracle(host, id_images, name):
    """At every pixel centre (cmd, triangle) is the triangle the model of vgx_raster_commands leaves in the pixel of the ID table."""
    sc = PH.scene(name)
    PH.check_id_image(name, id_images[name], PH.host_pick(host, sc, PC.centre_queries(sc.target)))


def test_relation_a_images_are_not_empty(id_images):
    """The check above cannot pass on empty images: they show at least three distinct commands, and every tested region state -- an In
    user shown, an In user refused, an Out user shown -- has a pixel whose topmost user is in that state."""
    seen, states = set(), {"passed_in": False, "refused_in": False, "passed_out": False}
    for name in sorted(PH.SCENES):
        sc = PH.scene(name)
        c, _ = PC.decode_ids(id_images[name], sc.target, PC.id_scene(sc)[1])
        seen.update((name, int(v)) for v in np.unique(c) if v >= 0)
        a, n = PH.expected(name), sc.target.width * sc.target.height
        for k in states:
            states[k] = states[k] or bool(getattr(a, k)[:n].any())
    assert all(any(n == name for n, _ in seen) for name in PH.SCENES)   # no scene's image is empty
    PH.check_id_images_are_not_empty({v for _, v in seen}, states)


def test_owner_search_against_brute_force(host):
    rs = np.random.RandomState(3)
    for trial in range(40):
        n = int(rs.randint(0, 12))
        meshes = np.zeros(n, dtype=capi.mesh_dtype)
        at = 0
        for m in range(n):
            at += int(rs.randint(0, 3)) * 3                      # a gap no mesh owns
            meshes["first_index"][m], meshes["num_indices"][m] = at, int(rs.choice([0, 0, 3, 9, 30]))   # empty meshes among them
            meshes["draw"][m] = rs.randint(0, 100)
            at += int(meshes["num_indices"][m])
        for p in list(range(0, at + 6)) + [1 << 40]:
            got = host.vgxt_pick_owner(meshes.ctypes.data if n else None, n, p)
            assert got == PC.owner(meshes, p), (trial, p)
    assert host.vgxt_pick_owner(None, 0, 0) == NONE


RECORD_FAULTS = ("type", "reserved", "num_vertices", "vertex_range", "vertex_range_64", "index_range", "index_range_64", "clip_range")
NOT_FAULTS = ("image_handle", "gradient_handle", "pattern_handle", "no_uv", "no_paints", "image_record", "paint_type")


@pytest.mark.parametrize("case", RECORD_FAULTS)
def test_each_invalid_record_alone(host, case):
    sc = CH.invalid_cases()[case]
    q = PC.centre_queries(sc.target)[::7]
    assert PC.status(sc) == BAD
    got = PH.host_pick(host, sc, q, want=BAD)
    assert (got.view(np.uint32) == NONE).all()


@pytest.mark.parametrize("case", NOT_FAULTS)
def test_handles_are_not_checked(host, case):
    """What vgx_raster_commands refuses for the handle's sake is fine here: nothing a handle names is read."""
    sc = CH.invalid_cases()[case]
    q = PC.centre_queries(sc.target)[::7]
    want = PC.pick(sc, q)
    assert want.status == OK and (want.hits["cmd"] != NONE).any()
    assert PH.same(PH.host_pick(host, sc, q), want.hits)


def test_empty_calls(host):
    sc = PH.scene("relative")
    assert PH.host_pick(host, sc, PC.queries(np.zeros((0, 2)))).shape[0] == 0   # nqueries == 0: the status alone
    empty = sc.with_cmds(sc.cmds[:0])
    got = PH.host_pick(host, empty, PC.centre_queries(sc.target)[:9])
    assert (got.view(np.uint32) == NONE).all()


def test_host_refusals(host):
    sc = PH.scene("relative")
    q = PC.centre_queries(sc.target)[:4].copy()
    h = np.zeros(8, dtype=capi.pick_cmd_hit_dtype)
    meshes = PH.owner_table("relative")
    base = h.ctypes.data + (-h.ctypes.data) % 16

    def call(sm=None, cmds=sc.cmds.ctypes.data, n=sc.cmds.shape[0], real=None, own=None, queries=q.ctypes.data, nq=4, hits=base, status=None):
        sm = CH.streams_struct(sc, (sc.pos.ctypes.data, sc.color.ctypes.data, sc.uv.ctypes.data, sc.idx.ctypes.data)) if sm is None else sm
        return host.vgxt_pick_commands(C.byref(sm) if sm != 0 else None, cmds, n, real, None if own is None else C.byref(own), queries, nq, hits, status)

    assert call() == OK
    assert call(sm=0) == BAD and call(cmds=None) == BAD and call(queries=None) == BAD and call(hits=None) == BAD
    assert call(cmds=None, n=0) == OK and call(queries=None, hits=None, nq=0) == OK
    assert call(nq=capi.PICK_MAX_QUERIES + 1) == RANGE
    for k, v in (("reserved", 1), ("uv_bytes", 3), ("uv_bytes", 0), ("pos", None), ("color", None), ("idx", None)):
        sm = CH.streams_struct(sc, (sc.pos.ctypes.data, sc.color.ctypes.data, sc.uv.ctypes.data, sc.idx.ctypes.data))
        setattr(sm, k, v)
        assert call(sm=sm) == BAD, k
    for k, off in (("pos", 4), ("color", 2), ("idx", 1), ("uv", 4)):
        sm = CH.streams_struct(sc, (sc.pos.ctypes.data, sc.color.ctypes.data, sc.uv.ctypes.data, sc.idx.ctypes.data))
        setattr(sm, k, getattr(sm, k) + off)
        assert call(sm=sm) == BAD, k
    assert call(cmds=sc.cmds.ctypes.data + 4) == BAD and call(queries=q.ctypes.data + 4) == BAD and call(hits=base + 8) == BAD
    assert call(real=base + 2) == BAD and call(status=base + 2) == BAD
    assert call(own=capi.PickOwners(None, 3)) == BAD and call(own=capi.PickOwners(meshes.ctypes.data + 4, meshes.shape[0])) == BAD
    assert call(own=capi.PickOwners(None, 0)) == OK and call(own=capi.PickOwners(meshes.ctypes.data, meshes.shape[0])) == OK


@pytest.fixture(scope="module")
def rt():
    import importlib
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.mark.skipif(not CH.ref_available(), reason="oracle/_ref/libvgref_vg.so not built")
def test_reference_frame_owners_equal_pick_frame(host, rt):
    """A frame of the reference's own Context (vertex buffers of 512) as a command table in buffer order, the mesh table of the same
    scenario tessellated without assembly as owners (first_index renamed to the position in the index stream): at every pixel centre of
    the reference windows mesh and draw are vgxt_pick_frame's on the unassembled frame, and the triangle is its triangle counted from the
    command's first index."""
    import raster_harness as H
    rs = CH.RefScene(rt, False)
    cmds, f = rs.buffer_order(), rs.unassembled((0, 0))
    meshes = f.meshes.copy()
    meshes["first_index"] = np.concatenate([[0], np.cumsum(f.meshes["num_indices"].astype(np.int64))])[:-1]
    hit = 0
    for w in CH.REF_WINDOWS:
        sc = rs.scene(cmds, w, "ref_buffer")
        q = PC.centre_queries(sc.target)
        got = PH.host_pick(host, sc, q, meshes)
        want = H.host_pick_frame(host, f, PC.frame_queries(q))
        assert np.array_equal(got["mesh"], want["mesh"]) and np.array_equal(got["draw"], want["draw"]), w
        ok = got["cmd"] != NONE
        m, c = got["mesh"][ok].astype(np.int64), got["cmd"][ok].astype(np.int64)
        off = (meshes["first_index"][m].astype(np.int64) - cmds["first_index"][c].astype(np.int64)) // 3
        assert (off >= 0).all() and np.array_equal(got["triangle"][ok].astype(np.int64), off + want["triangle"][ok].astype(np.int64)), w
        hit += int(ok.sum())
    assert hit > 2000
