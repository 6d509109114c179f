"""What the CPU and the GPU tests of vgx_pick_commands share: the callers of the host lane code (vgxt_pick_commands) and of the device
entry, the hand-built scenes -- the smallest at which the kernels can go wrong -- their query sets and the model's answers, computed once.
Not collected by pytest; nothing here touches torch at import time."""
import ctypes as C
import functools
import os

import numpy as np

import pick_commands_model as PC
import pick_frame_model as PF
import raster_commands_harness as CH
import raster_commands_model as CM
import raster_frame_model as M
import raster_harness as H
import raster_model as R

capi = R.capi
F = np.float32
OK, BAD, RANGE = capi.VGX_OK, capi.VGX_E_INVALID_ARG, capi.VGX_E_RANGE
NONE = PC.NONE
SKIP = PC.SKIP
GUARD = H.HITS_GUARD
rgba = CH.rgba

_V, _U32, _U64 = C.c_void_p, C.c_uint32, C.c_uint64
PROTOTYPES = {
    "vgxt_pick_commands": (C.c_int, [C.POINTER(capi.RasterStreams), _V, _U32, _V, C.POINTER(capi.PickOwners), _V, _U32, _V, _V]),
    "vgxt_pick_owner": (_U32, [_V, _U64, _U64]),
}


def load_host():
    """libvgx_hosttest.so with the prototypes above, beside those of the raster harnesses; one from before these calls is built once."""
    path = os.path.join(R.CM.ROOT, "vg-renderer_amd", "libvgx_hosttest.so")
    if not (os.path.exists(path) and all(hasattr(C.CDLL(path), name) for name in PROTOTYPES)):
        import __graft_entry__ as g
        g.build()
    lib = CH.load_host()
    for name, (restype, argtypes) in PROTOTYPES.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    return lib


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def limits():
    """One command of 129 overlapping triangles (three chunks, the last of one triangle) under a second, plain command: the queries
    put tri_end in the middle of a chunk, at both chunk boundaries, at 0 and behind the end."""
    b = CM.Builder()
    CH._pad(b)
    b.add(*CH.strip(129, 2.25, 3.5, step=0.11))
    b.add(M.quad(1.0, 1.0, 30.0, 16.0), rgba(9, 9, 9, 255), M.QUAD)
    return b.scene("limits", R.Target(32, 18, 32, 0, 0))


def shared_vertices():
    """Two commands over ONE vertex range and two index ranges (the two triangles of a quad, one each), a third over both."""
    b = CM.Builder()
    b.add(M.quad(2.0, 2.0, 14.0, 12.0), [rgba(1, 2, 3, 255), rgba(4, 5, 6, 0), rgba(7, 8, 9, 255), rgba(1, 1, 1, 255)], [0, 1, 2])
    b.idx += [0, 2, 3]
    b.cmds.append(CM.cmd(0, 3, 4, 3))
    b.cmds.append(CM.cmd(0, 0, 4, 6, scissor=(0, 0, 8, 8)))
    return b.scene("shared_vertices", R.Target(16, 14, 17, 0, 0))


STACK = 300


def stack():
    """More than 256 commands on one column under an In and an Out use of region A (command 0), then region B's clip command, a user
    of B and two users of A BEHIND it: where B stamped they see S = B, elsewhere S = A from more than 256 commands below -- the resolve
    carries a stamp across a block of 256."""
    b = CM.Builder()
    b.add(M.quad(0.0, 0.0, 8.0, 12.0), 0, M.QUAD, typ=CM.CLIP)                                   # A: the left half
    for k in range(STACK):
        b.add(M.quad(3.0 + 0.01 * k, 1.0, 13.0, 11.0), rgba(k & 255, k >> 8, 7, 255), M.QUAD, region=(0, 1), rule=k & 1)
    kb = b.add(M.quad(0.0, 0.0, 16.0, 5.0), 0, M.QUAD, typ=CM.CLIP)                              # B: the upper part
    b.add(M.quad(1.0, 1.0, 15.0, 3.0), rgba(200, 0, 0, 255), M.QUAD, region=(kb, 1), rule=0)
    b.add(M.quad(5.0, 2.0, 7.0, 10.0), rgba(0, 200, 0, 255), M.QUAD, region=(0, 1), rule=0)      # In A: refused where B stamped
    b.add(M.quad(9.0, 2.0, 11.0, 10.0), rgba(0, 0, 200, 255), M.QUAD, region=(0, 1), rule=1)     # Out A: passes everywhere right of A
    return b.scene("stack", R.Target(16, 12, 16, 0, 0))


def clip_zero():
    """A clip command whose colours are 0 -- it must stamp under VGX_PICK_SKIP_TRANSPARENT too -- an In user, and on top a quad with one
    vertex of alpha 0, which the flag skips."""
    b = CM.Builder()
    b.add(M.quad(2.0, 2.0, 12.0, 10.0), 0, M.QUAD, typ=CM.CLIP)
    b.add(M.quad(0.0, 0.0, 16.0, 12.0), rgba(50, 60, 70, 255), M.QUAD, region=(0, 1), rule=0)
    b.add(M.quad(4.0, 3.0, 15.0, 11.0), [rgba(1, 1, 1, 255), rgba(1, 1, 1, 0), rgba(1, 1, 1, 255), rgba(1, 1, 1, 255)], M.QUAD)
    return b.scene("clip_zero", R.Target(16, 12, 19, 0, 0))


def nan_positions():
    """A command two of whose triangles have a NaN corner (x of one, y of the other), beside triangles that cover."""
    b = CM.Builder()
    v = M.quad(2.0, 2.0, 12.0, 10.0) + [(CH.NAN, 4.0), (13.0, CH.NAN), (5.0, 5.0)]
    b.add(v, rgba(9, 99, 199, 255), M.QUAD + [0, 4, 2, 1, 5, 6])
    b.add(M.quad(6.0, 1.0, 15.0, 6.0), rgba(99, 9, 19, 128), M.QUAD)
    return b.scene("nan_positions", R.Target(16, 12, 16, 0, 0))


SCENES = dict({k: CH.SCENES[k] for k in ("count_63", "count_64", "count_65", "count_129", "odd_lists", "seam", "relative", "shared_indices", "scissors", "clip",
                                         "short_table")},
              limits=limits, shared_vertices=shared_vertices, stack=stack, clip_zero=clip_zero, nan_positions=nan_positions)
NAN_SCENES = ("nan_positions",)  # a NaN inside a command's vertex range: the box of the equivalent mesh is unspecified, relation (b) is not asked


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def owner_table(name):
    """A mesh table over the scene's index stream: runs of 9, 0 (an empty mesh), 3 and 6 indices in turn, a gap of 3 indices no mesh
    owns behind every fourth, draws that are no function of the mesh number."""
    sc = scene(name)
    rows, at, k = [], 0, 0
    while at < sc.ni:
        n = min((9, 0, 3, 6)[k & 3], sc.ni - at)
        rows.append((0, at, 0, n, (k * 7 + 3) % 11, capi.MESH_FILL << 28))
        at += n + (3 if (k & 3) == 3 else 0)
        k += 1
    return np.array(rows, dtype=capi.mesh_dtype) if rows else np.zeros(0, dtype=capi.mesh_dtype)


def _points(sc, seed):
    """Vertices, edge midpoints and seeded random points of the scene, then NaN, +-inf and +-2^31: those of pick_frame_model."""
    return PF.off_centre_points(CM.equivalent_frame(sc), seed, nvert=40, nmid=40, nrand=80)


@functools.lru_cache(maxsize=None)
def query_set(name):
    """(queries, centres): every pixel centre of the target (flags 0, no limit), then the off-centre points four times over -- flags 0 and
    VGX_PICK_SKIP_TRANSPARENT, each without a limit and with a (cmd_end, tri_end) drawn from below, inside and behind the table and its
    commands' chunks; a few queries with reserved != 0."""
    sc = scene(name)
    parts = [PC.centre_queries(sc.target)]
    pts = _points(sc, 7 + len(name))
    rs = np.random.RandomState(23)
    nt = [int(c["num_indices"]) // 3 for c in sc.cmds[:sc.n]] or [0]
    for flags in (0, SKIP):
        q = PC.queries(pts, flags=flags)
        parts.append(q)
        q = PC.queries(pts, flags=flags)
        q["cmd_end"] = rs.randint(0, sc.n + 2, size=q.shape[0])
        ends = np.array([0, 1, 63, 64, 65, 70, 128, 129, 1000])
        q["tri_end"] = np.where(rs.randint(0, 2, size=q.shape[0]) == 0, ends[rs.randint(0, ends.size, size=q.shape[0])],
                                rs.randint(0, max(nt) + 2, size=q.shape[0]))
        parts.append(q)
    bad = PC.queries(pts[:6])
    bad["reserved"] = [1, 0, 0xFFFFFFFF, 0, 2, 0]
    parts.append(bad)
    return np.concatenate(parts), parts[0].shape[0]


@functools.lru_cache(maxsize=None)
def _prep(name):
    return PC.prepare(scene(name))


@functools.lru_cache(maxsize=None)
def expected(name, owners=True):
    """The model's answer to the scene's query set: computed once per session, never changed."""
    return PC.pick(scene(name), query_set(name)[0], owner_table(name) if owners else None, prep=_prep(name))


def limit_queries():
    """Scene `limits`, one point under most of the 129 triangles: no limit; tri_end at 0, in the middle of chunk 1, at both chunk
    boundaries, at the last triangle and behind it, for command 0; the same for command 1, which lies above."""
    pts = [(12.0, 8.0)] * 16
    q = PC.queries(pts)
    q["cmd_end"] = [NONE, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 0, 1, NONE]
    q["tri_end"] = [0, 0, 1, 64, 70, 128, 129, 500, 0, 1, 2, 0, 5, 63, 0xFFFFFFFF, 0xFFFFFFFF]
    return q


def check_limit_answers(sc, q, got):
    """The answers to limit_queries() from the list of covering triangles alone (no walk, no stamps: the scene is plain): the largest
    covering (c, t) below the limit. The point lies under triangles of both full chunks of command 0."""
    p = _prep("limits")
    Tr = p.tris
    cov = PF.cover_many(Tr.a, Tr.b, Tr.c, np.float64(q["x"][0]), np.float64(q["y"][0]))[0] & Tr.valid
    covering = sorted(zip(Tr.mesh[cov].tolist(), Tr.t[cov].tolist()))
    ts = [t for c, t in covering if c == 0]
    assert any(t < 64 for t in ts) and any(64 <= t < 128 for t in ts) and any(c == 1 for c, _ in covering)
    for k in range(q.shape[0]):
        lim = (int(q["cmd_end"][k]), int(q["tri_end"][k]))
        below = [ct for ct in covering if ct < lim]
        want = below[-1] if below else (NONE, NONE)
        assert (int(got["cmd"][k]), int(got["triangle"][k])) == want, (k, lim, tuple(got[k]), want)


# ---- callers ---------------------------------------------------------------------------------------------------------------------------
def chunks(n):
    return PF.chunks(n) or [(0, 0)]


def host_pick(host, sc, q, meshes=None, want=OK, guard=2):
    """vgxt_pick_commands in calls of at most 256 queries, each into a pattern-filled array whose records behind nqueries must stay."""
    sm = CH.streams_struct(sc, (sc.pos.ctypes.data, sc.color.ctypes.data, None if sc.uv is None else sc.uv.ctypes.data, sc.idx.ctypes.data))
    real = None if sc.real is None else np.array([sc.real], dtype=np.uint32)
    own = None if meshes is None else capi.PickOwners(meshes.ctypes.data if meshes.shape[0] else None, meshes.shape[0])
    out = np.zeros(q.shape[0], dtype=capi.pick_cmd_hit_dtype)
    for a, b in chunks(q.shape[0]):
        qq = np.ascontiguousarray(q[a:b])
        h = np.full((b - a + guard) * 4, GUARD, dtype=np.uint32)
        status = np.full(3, 77, dtype=np.uint32)
        rc = host.vgxt_pick_commands(C.byref(sm), sc.cmds.ctypes.data if sc.cmds.shape[0] else None, sc.cmds.shape[0], None if real is None else real.ctypes.data,
                                     None if own is None else C.byref(own), qq.ctypes.data if b > a else None, b - a, h.ctypes.data, status.ctypes.data)
        assert rc == OK, rc
        assert status.tolist() == [want, 77, 77], status.tolist()
        assert np.all(h[(b - a) * 4:] == GUARD)
        out[a:b] = h[:(b - a) * 4].view(capi.pick_cmd_hit_dtype)
    return out


class DevOwners:
    def __init__(self, meshes):
        self.t = H.to_dev(meshes) if meshes.shape[0] else None
        self.struct = capi.PickOwners(None if self.t is None else self.t.data_ptr(), meshes.shape[0])


def gpu_pick(rt, ctx, sc, q, meshes=None, dev=None, want=OK, guard=2, sizes=None):
    """vgx_pick_commands in calls of `sizes` queries (default: at most 256), each into a pattern-filled array: the records behind nqueries,
    the words beside dev_status and the queries must stay as they were."""
    import torch
    dev = CH.DevScene(sc) if dev is None else dev
    own = None if meshes is None else DevOwners(meshes)
    out = np.zeros(q.shape[0], dtype=capi.pick_cmd_hit_dtype)
    for a, b in (chunks(q.shape[0]) if sizes is None else sizes):
        qd = H.to_dev(q[a:b]) if b > a else None
        h = torch.full(((b - a + guard) * 4,), GUARD, dtype=torch.int32, device="cuda:0")
        status = torch.full((3,), 77, dtype=torch.int32, device="cuda:0")
        st = rt.lib().vgx_pick_commands(ctx.handle, C.byref(dev.streams), dev.t[3].data_ptr() if sc.cmds.shape[0] else None, sc.cmds.shape[0],
                                        None if dev.real is None else dev.real.data_ptr(), None if own is None else C.byref(own.struct),
                                        None if qd is None else qd.data_ptr(), b - a, h.data_ptr(), status.data_ptr(), rt._stream_ptr())
        torch.cuda.synchronize()
        assert st == OK, st
        assert status.cpu().tolist() == [want, 77, 77], (status.cpu().tolist(), want)
        got = h.cpu().numpy().view(np.uint32)
        assert np.all(got[(b - a) * 4:] == GUARD)
        if qd is not None:
            assert np.array_equal(qd.cpu().numpy()[:(b - a) * 24], np.ascontiguousarray(q[a:b]).view(np.uint8).reshape(-1))
        out[a:b] = got[:(b - a) * 4].view(capi.pick_cmd_hit_dtype)
    return out


def same(a, b):
    return H.same(a, b)


def differences(got, want, q):
    return H.first_difference(got, want, q)


# ---- checks on the model's output alone ------------------------------------------------------------------------------------------------
def check_conditions(name):
    """What a scene's query set must exercise, asserted before the product's answer is looked at."""
    sc, (q, centres), a = scene(name), query_set(name), expected(name)
    hit = a.hits["cmd"] != NONE
    bad = ~(np.abs(q["x"].astype(np.float64)) < PF.LIMIT) | ~(np.abs(q["y"].astype(np.float64)) < PF.LIMIT) | (q["reserved"] != 0)
    assert int(bad.sum()) >= 24 and not hit[bad].any()
    if name != "odd_lists":
        assert hit.any() and (~hit & ~bad).any()
    owned = hit & (a.hits["mesh"] != NONE)
    assert owned.any() or not hit.any()
    if name in ("clip", "stack"):
        assert a.passed_in.any() and a.refused_in.any() and a.passed_out.any()
    if name == "stack":
        c = a.hits["cmd"][hit].astype(np.int64)
        assert (c > 256).any() and (c > STACK + 1).any()   # hits tested against command 0 from another block of 256
    if name == "clip_zero":
        plain, skip = q["flags"] == 0, q["flags"] == SKIP
        assert (a.hits["cmd"][plain] == 2).any() and (a.hits["cmd"][skip] == 1).any()   # under the flag the In user shows: the clip command stamped
    if name == "seam":
        assert ((a.hits["cmd"][:centres] == 0) & (a.hits["triangle"][:centres] == 63)).any() and ((a.hits["triangle"][:centres] == 64)).any()
    if name in ("limits", "count_129"):
        assert (a.hits["triangle"][hit] >= 64).any() and (a.hits["triangle"][hit] < 64).any()


def check_id_image(name, image, picked):
    """Relation (a): `image` is the ID table's image (uint32 [rows, stride]), `picked` the hits of the scene's centre queries."""
    sc = scene(name)
    _, first = PC.id_scene(sc)
    c, t = PC.decode_ids(image, sc.target, first)
    pc = np.where(picked["cmd"] == NONE, -1, picked["cmd"].astype(np.int64)).reshape(sc.target.height, sc.target.width)
    pt = np.where(picked["cmd"] == NONE, -1, picked["triangle"].astype(np.int64)).reshape(sc.target.height, sc.target.width)
    assert np.array_equal(pc, c) and np.array_equal(pt, t), (np.argwhere((pc != c) | (pt != t))[:5].tolist())
    return c


def check_id_images_are_not_empty(seen, states):
    """Over all scenes: at least three distinct commands show, and every tested region state has a pixel."""
    assert len(seen) >= 3, seen
    assert all(states.values()), states
