"""GPU: vgx_pick_commands (csrc/vgx_pick_cmds.hip: k_pickc_cmds, the command scan, k_pickc_tris, k_pickc_resolve) against the numpy
statement of the specification (tests/pick_commands_model.py), against the lane code (vgxt_pick_commands), against the image the KERNELS
of vgx_raster_commands draw of the ID table (relation (a) of include/vgx.h), against vgx_pick_frame on the one-mesh-per-command frame
(relation (b)) and, through the product's own assembled frame, against vgx_pick_frame on the unassembled frame. Every comparison is exact:
all four words of every hit. Scenes, query sets and answers are those of tests/test_pick_commands_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import pick_commands_harness as PH
import pick_commands_model as PC
import pick_frame_model as PF
import raster_commands_harness as CH
import raster_commands_model as CM
import raster_harness as H
import raster_model as R
from raster_harness import rt  # noqa: F401

pytestmark = pytest.mark.gpu
capi = PC.capi
NONE = PC.NONE
OK, BAD = PH.OK, PH.BAD


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    rt.raster_reserve(c, 1024, 1 << 14)
    rt.raster_commands_reserve(c, 512, 2048, 1 << 15)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    return PH.load_host()


_devs = {}


def dev(name):
    if name not in _devs:
        _devs[name] = CH.DevScene(PH.scene(name))
    return _devs[name]


class DevEq:
    """The one-mesh-per-command frame of a scene and its draw table in device memory."""

    def __init__(self, sc):
        self.f = CM.equivalent_frame(sc)
        self.frame, self.state = H.DevFrame(self.f), H.DevState(self.f)


def gpu_pick_frame(rt, ctx, frame_desc, state_struct, q16):
    """vgx_pick_frame with mesh_bounds == NULL in calls of at most 256 queries."""
    import torch
    out = np.zeros(q16.shape[0], dtype=capi.pick_hit_dtype)
    for a, b in PH.chunks(q16.shape[0]):
        if b == a:
            continue
        qd = H.to_dev(q16[a:b])
        h = torch.full(((b - a) * 4,), PH.GUARD, dtype=torch.int32, device="cuda:0")
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
        assert rt.lib().vgx_pick_frame(ctx.handle, C.byref(frame_desc), None, 0, H.OPEN, C.byref(state_struct), qd.data_ptr(), b - a, h.data_ptr(), status.data_ptr(),
                                       rt._stream_ptr()) == OK
        torch.cuda.synchronize()
        assert int(status.item()) == OK
        out[a:b] = h.cpu().numpy().view(np.uint32).view(capi.pick_hit_dtype)
    return out


@pytest.mark.parametrize("name", sorted(PH.SCENES))
def test_kernels_equal_model_and_lane_code(rt, ctx, host, name):
    sc, (q, _) = PH.scene(name), PH.query_set(name)
    PH.check_conditions(name)
    want = PH.expected(name)
    d = dev(name)
    got = PH.gpu_pick(rt, ctx, sc, q, PH.owner_table(name), dev=d)
    assert PH.same(got, want.hits), PH.differences(got, want.hits, q)
    assert PH.same(PH.host_pick(host, sc, q, PH.owner_table(name)), got)
    bare = PH.gpu_pick(rt, ctx, sc, q, dev=d)
    assert np.array_equal(bare["cmd"], got["cmd"]) and np.array_equal(bare["triangle"], got["triangle"])
    assert (bare["mesh"] == NONE).all() and (bare["draw"] == NONE).all()
    assert H._as_uploaded(d.t, (sc.pos, sc.color, sc.idx, sc.cmds))   # the streams and the table as they were


def test_limits_inside_a_command(rt, ctx):
    sc, q = PH.scene("limits"), PH.limit_queries()
    PH.check_limit_answers(sc, q, PH.gpu_pick(rt, ctx, sc, q, dev=dev("limits")))


@pytest.mark.parametrize("nq", [0, 1, 65, 256])
def test_query_counts(rt, ctx, nq):
    name = "clip"
    (q, centres), want = PH.query_set(name), PH.expected(name)
    lo = centres - nq // 2  # pixel centres and off-centre points in one call
    got = PH.gpu_pick(rt, ctx, PH.scene(name), q[lo:lo + nq], PH.owner_table(name), dev=dev(name), sizes=[(0, nq)])
    assert PH.same(got, want.hits[lo:lo + nq])


@pytest.mark.parametrize("name", ["clip", "stack", "seam", "scissors", "shared_indices", "shared_vertices", "count_129", "nan_positions", "short_table"])
def test_relation_a_the_image_is_the_oracle(rt, ctx, name):
    """vgx_pick_commands at every pixel centre against vgx_raster_commands of the ID table, both run by the kernels."""
    sc = PH.scene(name)
    ids, _ = PC.id_scene(sc)
    image = CH.gpu_commands(rt, ctx, ids)[1]
    c = PH.check_id_image(name, image, PH.gpu_pick(rt, ctx, sc, PC.centre_queries(sc.target), dev=dev(name)))
    assert (c >= 0).any()
    if name in ("clip", "stack"):
        assert np.unique(c[c >= 0]).size >= 3


@pytest.mark.parametrize("name", [n for n in sorted(PH.SCENES) if n not in PH.NAN_SCENES and CH.buffer_order(PH.scene(n))])
def test_relation_b_equals_pick_frame_on_the_device(rt, ctx, name):
    sc, (q, _) = PH.scene(name), PH.query_set(name)
    q = q[(q["tri_end"] == 0) & (q["reserved"] == 0)]
    e = DevEq(sc)
    want = gpu_pick_frame(rt, ctx, e.frame.desc, e.state.struct, PC.frame_queries(q))
    got = PH.gpu_pick(rt, ctx, sc, q, dev=dev(name))
    assert np.array_equal(got["cmd"], want["mesh"]) and np.array_equal(got["triangle"], want["triangle"])
    assert (got["cmd"] != NONE).any()


def test_buffer_order_scenes_are_enough():
    names = [n for n in sorted(PH.SCENES) if n not in PH.NAN_SCENES and CH.buffer_order(PH.scene(n))]
    assert {"clip", "stack", "seam", "scissors", "limits"} <= set(names), names


@pytest.mark.parametrize("case", ["type", "reserved", "num_vertices", "vertex_range_64", "index_range", "index_range_64", "clip_range"])
def test_each_invalid_record_alone(rt, ctx, case):
    sc = CH.invalid_cases()[case]
    got = PH.gpu_pick(rt, ctx, sc, PC.centre_queries(sc.target)[::7], want=BAD)
    assert (got.view(np.uint32) == NONE).all()


def test_handles_are_not_checked_and_empty_calls(rt, ctx):
    sc = CH.invalid_cases()["gradient_handle"]
    q = PC.centre_queries(sc.target)[::7]
    want = PC.pick(sc, q)
    assert want.status == OK and PH.same(PH.gpu_pick(rt, ctx, sc, q), want.hits)
    base = PH.scene("relative")
    empty = base.with_cmds(base.cmds[:0])
    assert (PH.gpu_pick(rt, ctx, empty, q[:9]).view(np.uint32) == NONE).all()
    assert rt.lib().vgx_pick_commands(None, None, None, 0, None, None, None, 0, None, None, None) == BAD
    d = dev("relative")
    assert rt.lib().vgx_pick_commands(ctx.handle, C.byref(d.streams), d.t[3].data_ptr(), 2, None, None, d.t[3].data_ptr(), capi.PICK_MAX_QUERIES + 1, d.t[3].data_ptr(),
                                      None, None) == capi.VGX_E_RANGE


# ---- through the product ---------------------------------------------------------------------------------------------------------------
class Product:
    """The reference scenario through vgx_set_assembly (split state, max_vb_vertices 512) and vgx_raster_cmds_from_assembly: the assembled
    streams, the command table and the mesh table in device memory, and the same scenario unassembled."""

    def __init__(self, rt):
        import torch
        self.rs = rs = CH.RefScene(rt, False)
        self.f = f = rs.unassembled((0, 0))
        self.ctx = c = rt.Context(0)
        pset = rt.PathSet(c, rs.ps)
        dd = rt.upload_draws(rs.draws)
        cap = 256
        dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device="cuda:0")
        num = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        self.uv = torch.zeros((f.nv, 2), dtype=torch.int16, device="cuda:0")
        self.bufs = rt.MeshBuffers(dd.device, f.nv, f.ni, f.nm)
        c.set_assembly(dcmds, max_vb_vertices=512, dev_num=num, split_state=True, uv=self.uv, uv_value=(int(rs.ref["white_uv"][0][0]), 0))
        try:
            sizes = rt.tessellate_count(c, pset, dd, rs.draws.shape[0])
            assert (sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]) == (f.nv, f.ni, f.nm)
            rt.tessellate_emit(c, pset, dd, rs.draws.shape[0], self.bufs)
        finally:
            c.set_assembly(None)
        torch.cuda.synchronize()
        self.dstate = H.to_dev(rs.dstate)
        self.cmds_dev, self.n_dev, status = rt.raster_cmds_from_assembly(c, dcmds, cap, num, self.bufs.meshes, f.nm, self.dstate, rs.dstate.shape[0])
        torch.cuda.synchronize()
        self.k = int(num.item())
        assert int(status.item()) == OK and int(self.n_dev.item()) == self.k
        self.cmds = self.cmds_dev.cpu().numpy()[:self.k * 56].view(capi.raster_cmd_dtype).copy()
        self.meshes = self.bufs.meshes.cpu().numpy()[:f.nm * 32].view(capi.mesh_dtype).copy()
        self.streams = rt.raster_streams(self.bufs.pos, self.bufs.color, self.bufs.idx, f.nv, f.ni, uv_dev=self.uv, uv_bytes=4)
        self.frame, self.state = H.DevFrame(f), H.DevState(f)
        pset.close()

    def pick(self, rt, q):
        import torch
        hits, status = rt.pick_commands(self.ctx, self.streams, self.cmds_dev, 256, H.to_dev(q), q.shape[0], meshes_dev=self.bufs.meshes, num_meshes=self.f.nm,
                                        dev_num_cmds=self.n_dev)
        torch.cuda.synchronize()
        assert int(status.item()) == OK
        return hits.cpu().numpy()[:q.shape[0] * 16].view(capi.pick_cmd_hit_dtype)


@pytest.fixture(scope="module")
def product(rt):
    p = Product(rt)
    yield p
    p.ctx.close()


def test_through_the_product(rt, product):
    """At every pixel centre of the reference windows, mesh and draw are vgx_pick_frame's on the unassembled frame, and the triangle is
    its triangle counted from the command's first index."""
    p = product
    hit = 0
    for w in CH.REF_WINDOWS:
        tgt = R.Target(64, 48, 67, w[0], w[1])
        q = PC.centre_queries(tgt)
        want = gpu_pick_frame(rt, p.ctx, p.frame.desc, p.state.struct, PC.frame_queries(q))
        got = np.concatenate([p.pick(rt, q[a:b]) for a, b in PH.chunks(q.shape[0])])
        assert np.array_equal(got["mesh"], want["mesh"]) and np.array_equal(got["draw"], want["draw"]), w
        ok = got["cmd"] != NONE
        assert np.array_equal(ok, want["mesh"] != NONE)
        m, c = got["mesh"][ok].astype(np.int64), got["cmd"][ok].astype(np.int64)
        off = (p.meshes["first_index"][m].astype(np.int64) - p.cmds["first_index"][c].astype(np.int64)) // 3
        assert (off >= 0).all() and np.array_equal(got["triangle"][ok].astype(np.int64), off + want["triangle"][ok].astype(np.int64)), w
        hit += int(ok.sum())
    assert hit > 2000  # the windows are not empty


def test_click_through_walks_the_stack_of_draws(rt, product):
    """cmd_end / tri_end from the owners walk the same stack as vgx_pick_frame's mesh_end walk."""
    p = product
    point = (60.5, 40.5)  # under several of the circles (fill and stroke each) and the scissored rectangle
    walk_c, walk_f = [], []
    q = PC.queries([point])
    q16 = PC.frame_queries(q)
    for _ in range(8):
        h = p.pick(rt, q)[0]
        g = gpu_pick_frame(rt, p.ctx, p.frame.desc, p.state.struct, q16)[0]
        walk_c.append((int(h["mesh"]), int(h["draw"])))
        walk_f.append((int(g["mesh"]), int(g["draw"])))
        if int(h["cmd"]) == NONE or int(g["mesh"]) == NONE:
            break
        q["cmd_end"] = int(h["cmd"])
        q["tri_end"] = (int(p.meshes["first_index"][int(h["mesh"])]) - int(p.cmds["first_index"][int(h["cmd"])])) // 3
        q16["mesh_end"] = int(g["mesh"])
    assert walk_c == walk_f
    assert len({d for _, d in walk_c if d != NONE}) >= 3, walk_c


def test_no_leak_between_calls(rt, ctx):
    """vgx_pick_frame, vgx_raster_commands and vgx_pick_commands interleaved on one context: each gives its own answers."""
    name = "clip"
    sc, (q, _), want = PH.scene(name), PH.query_set(name), PH.expected(name, owners=False)
    e = DevEq(sc)
    q = q[:256]
    frame_want = gpu_pick_frame(rt, ctx, e.frame.desc, e.state.struct, PC.frame_queries(q))
    image_want = CH.expected(name, True)
    for _ in range(2):
        assert PH.same(PH.gpu_pick(rt, ctx, sc, q, dev=dev(name)), want.hits[:256])
        assert np.array_equal(CH.gpu_commands(rt, ctx, sc, sc.target.with_clear(CH.CLEAR), dev=dev(name))[1], image_want)
        assert PH.same(gpu_pick_frame(rt, ctx, e.frame.desc, e.state.struct, PC.frame_queries(q)), frame_want)
        other = "stack"
        oq = PH.query_set(other)[0][:1]
        assert PH.same(PH.gpu_pick(rt, ctx, PH.scene(other), oq, dev=dev(other)), PH.expected(other, owners=False).hits[:1])


def test_scratch_bytes(rt):
    """The call keeps 40 bytes per command and 4 per pair of a command and a query (and the head room of every scratch table); a second
    call of the same size grows nothing."""
    name = "stack"
    sc, (q, _) = PH.scene(name), PH.query_set(name)
    c = rt.Context(0)
    try:
        lib = rt.lib()
        lib.vgx_scratch_bytes.restype = C.c_uint64
        n = sc.cmds.shape[0]
        b0 = lib.vgx_scratch_bytes(c.handle)
        PH.gpu_pick(rt, c, sc, q[:256], dev=dev(name))
        b1 = lib.vgx_scratch_bytes(c.handle)
        need = 40 * n + 4 * n * 256
        fixed = 512 * 32 + 4 * 8
        assert need <= b1 - b0 <= int((need + 64) * 1.25) + fixed + 5 * 4096, (b0, b1, need)
        PH.gpu_pick(rt, c, sc, q[:256], dev=dev(name))
        PH.gpu_pick(rt, c, sc, q[:7], dev=dev(name))
        assert lib.vgx_scratch_bytes(c.handle) == b1
    finally:
        c.close()


def test_counted_state_survives(rt, gpu_ctx, wl, oracle):
    """vgx_tessellate_count -> vgx_pick_commands -> vgx_tessellate_emit gives the oracle's meshes."""
    name = "clip"
    sc, (q, _), want = PH.scene(name), PH.query_set(name), PH.expected(name, owners=False)
    d = dev(name)
    qd = H.to_dev(q[:256])

    def call():
        hits, status = rt.pick_commands(gpu_ctx, d.streams, d.t[3], sc.cmds.shape[0], qd, 256)
        return hits[:256 * 16], status

    H.check_counted_state_survives(rt, gpu_ctx, wl, oracle, call, want.hits[:256].view(np.uint32))
