"""GPU: vgx_merge / vgx_merge_uv, vgx_cache_submit, vgx_cache_localize and the draw-command assembly behind them on made-up mesh
streams (tests/mesh_streams.py) far past frame size: the three-pass scan of the merged sequence, the grid-stride loops of
k_merge_rank / k_merge_copy / k_cache_localize, the multi-launch assembly route with and without VGX_ASM_SPLIT_STATE, runs of empty
instances across scan slices. Expected values: merge_model / merge_uv_model (pinned in tests/test_mesh_streams_cpu.py) and the CPU
oracle (cache_submit, cache_localize, assemble). Every comparison is exact, positions as uint32.

Every output sits between 64 pattern-filled elements, is handed over with its exact size, and the guards are checked in every test;
the VGX_E_NOSPACE cases lower the capacity by one and leave the allocation as it is.

The context is the module's own: the assembly route depends on the mesh-table scratch of the context when a caller passes no mesh
table (scan_bound = ctx->mtab.cap in runAssemble), and these tests grow that scratch to half a million records, which would change
the route of every later test on the session's context."""
import ctypes as C
import importlib

import numpy as np
import pytest

import mesh_streams as MS

pytestmark = pytest.mark.gpu
capi = MS.capi
G = 64
POS_PATTERN, COLOR_PATTERN, IDX_PATTERN, MESH_BYTE, CMD_BYTE = -12345.5, 0x3C0FFEE1, 0x5EED, 0xEE, 0xC3
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(8, dtype=np.uint8)).to(DEV)


class DevStream:
    """A host stream (MeshResult) in device memory, as a vgx_cache_desc."""

    def __init__(self, r):
        self.t = [to_dev(x) for x in (r.pos, r.color, r.idx, r.meshes)]
        self.desc = capi.CacheDesc(self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), self.t[3].data_ptr(),
                                   r.meshes.shape[0], r.pos.shape[0], r.idx.shape[0])


class Out:
    """Output buffers of exactly (nv, ni, nm) elements between guards. short: the index of the capacity handed over one too small."""

    def __init__(self, rt, nv, ni, nm, short=None):
        self.n = nv, ni, nm = int(nv), int(ni), int(nm)
        self.all = rt.MeshBuffers(DEV, nv + 2 * G, ni + 2 * G, nm + 2 * G)
        self.all.pos.fill_(POS_PATTERN), self.all.color.fill_(COLOR_PATTERN), self.all.idx.fill_(IDX_PATTERN), self.all.meshes.fill_(MESH_BYTE)
        self.view = self.all.view(G, nv, G, ni, G, nm)
        cap = list(self.n)
        if short is not None:
            cap[short] -= 1
        self.view.cap = tuple(cap)

    @classmethod
    def of(cls, rt, want, short=None):
        return cls(rt, want.pos.shape[0], want.idx.shape[0], want.meshes.shape[0], short)

    def read(self):
        """(pos as uint32, color, idx, meshes, dev_sizes, dev_status) of the inner part; asserts the guards."""
        import torch
        torch.cuda.synchronize()
        nv, ni, nm = self.n
        pos, color = self.all.pos.cpu().numpy(), self.all.color.cpu().numpy().view(np.uint32)
        idx, meshes = self.all.idx.cpu().numpy().view(np.uint16), self.all.meshes.cpu().numpy()
        assert np.all(pos[:G] == np.float32(POS_PATTERN)) and np.all(pos[G + nv:] == np.float32(POS_PATTERN)), "pos guard"
        assert np.all(color[:G] == COLOR_PATTERN) and np.all(color[G + nv:] == COLOR_PATTERN), "color guard"
        assert np.all(idx[:G] == IDX_PATTERN) and np.all(idx[G + ni:] == IDX_PATTERN), "idx guard"
        assert np.all(meshes[:G * 32] == MESH_BYTE) and np.all(meshes[(G + nm) * 32:] == MESH_BYTE), "mesh guard"
        return (pos[G:G + nv].view(np.uint32), color[G:G + nv], idx[G:G + ni], meshes[G * 32:(G + nm) * 32].view(capi.mesh_dtype),
                self.view.dev_sizes.cpu().numpy(), int(self.view.dev_status.item()))

    def assert_untouched(self):
        """Every element between the guards still holds its fill pattern: the call wrote nothing at all."""
        pos, color, idx, meshes, _, _ = self.read()
        assert np.all(pos.view(np.float32) == np.float32(POS_PATTERN)) and np.all(color == COLOR_PATTERN), "vertex streams written"
        assert np.all(idx == IDX_PATTERN) and np.all(meshes.view(np.uint8) == MESH_BYTE), "index stream or mesh table written"


def assert_frame(out, want, idx=None):
    """The whole frame == want (a MeshResult); idx: the index buffer to expect instead of want.idx (an assembled frame)."""
    pos, color, gidx, meshes, sizes, status = out.read()
    print("dev_sizes meshes / vertices / indices:", int(sizes[2]), int(sizes[3]), int(sizes[4]), "status", status)
    assert status == capi.VGX_OK
    assert (int(sizes[2]), int(sizes[3]), int(sizes[4])) == (want.meshes.shape[0], want.pos.shape[0], want.idx.shape[0])
    for f in want.meshes.dtype.names:
        assert np.array_equal(meshes[f], want.meshes[f]), f
    assert np.array_equal(pos, want.pos.view(np.uint32))
    assert np.array_equal(color, want.color)
    assert np.array_equal(gidx, want.idx if idx is None else idx)
    return sizes


class Armed:
    """Arms draw-command assembly with a guarded command table of exactly ncmd records (and a UV stream); disarm() in a finally."""

    def __init__(self, ctx, ncmd, max_vb, split, uv=None, white=None):
        import torch
        self.ctx, self.ncmd = ctx, ncmd
        self.all = torch.full(((ncmd + 2 * G) * 48,), CMD_BYTE, dtype=torch.uint8, device=DEV)
        self.num = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        ctx.set_assembly(self.all[G * 48:(G + ncmd) * 48], max_vb, self.num, split_state=split, uv=uv, uv_value=white)

    def disarm(self):
        self.ctx.set_assembly(None)

    def assert_commands(self, rcmds, sizes):
        raw = self.all.cpu().numpy()
        assert np.all(raw[:G * 48] == CMD_BYTE) and np.all(raw[(G + self.ncmd) * 48:] == CMD_BYTE), "command guard"
        assert int(self.num.item()) == len(rcmds) and int(sizes[9]) == len(rcmds)
        got = raw[G * 48:(G + self.ncmd) * 48].view(capi.drawcmd_dtype)
        for f in rcmds.dtype.names:
            assert np.array_equal(got[f], rcmds[f]), f


# ---- vgx_merge ---------------------------------------------------------------------------------------------------------------------
def run_merge(rt, ctx, a, b, b_draw, out, draws=None, b_uv=None):
    import torch
    da, db = DevStream(a), DevStream(b)
    bd = to_dev(np.ascontiguousarray(b_draw, dtype=np.uint32)) if b_draw is not None else None
    dd = to_dev(draws) if draws is not None else None
    uv = to_dev(b_uv) if b_uv is not None else None
    rt.merge(ctx, da.desc, db.desc, bd, dd, 0 if draws is None else draws.shape[0], out.view, uv)
    torch.cuda.synchronize()


def check_merge(rt, ctx, a, b, b_draw):
    want = MS.merge_model(a, b, b_draw)
    out = Out.of(rt, want)
    run_merge(rt, ctx, a, b, b_draw, out)
    assert_frame(out, want)
    return want


@pytest.mark.parametrize("na,nb", [(0, 0), (1, 0), (0, 1)])
def test_merge_empty(rt, ctx, na, nb):
    rs = np.random.RandomState(10 + na + 2 * nb)
    check_merge(rt, ctx, MS.make_stream(rs, na, 6, 1, num_vertices=[5] * na), MS.make_stream(rs, nb, 6, 1, num_vertices=[4] * nb), None)


@pytest.mark.parametrize("n", [1024, 1025, 131072, 131073, 524288 + 257])
def test_merge_ties(rt, ctx, n):
    """1 024 / 1 025: the single-workgroup scan and the first size of the three-pass one; 131 072 / 131 073: scan slices of 256 and of
    512 items, b with holes; 524 545: more meshes than the grids of k_merge_rank (2 048 x 256 threads) and k_merge_copy (8 192 x 4
    waves) cover at once, b_draw given and b's own draw field scrambled. Draws are shared by both sides throughout (the tie rule)."""
    a, b, b_draw, _ = MS.merge_case(n)
    want = check_merge(rt, ctx, a, b, b_draw)
    da, db = a.meshes["draw"], (b.meshes["draw"] if b_draw is None else b_draw)
    assert np.intersect1d(da, db).shape[0] > min(n // 16, 100)  # ties there are
    assert (b_draw is not None) == (n > 500000) and np.any(want.order[1:] < want.order[:-1])


@pytest.mark.parametrize("kind", ["a_first", "b_first", "draw7"])
def test_merge_orders(rt, ctx, kind):
    a, b, b_draw, _ = MS.merge_case(40000, kind)
    want = check_merge(rt, ctx, a, b, b_draw)
    na = a.meshes.shape[0]
    if kind == "b_first":
        assert np.array_equal(want.order, np.concatenate([np.arange(na, 40000), np.arange(na)]))
    else:
        assert np.array_equal(want.order, np.arange(40000))  # draw7: one tie of 40 000 meshes, all of `a` in front


@pytest.mark.parametrize("side", ["a", "b"])
def test_merge_one_side_at_size(rt, ctx, side):
    rs = np.random.RandomState(77)
    full, none = MS.make_stream(rs, 40000, 6, 5000, holes=side == "b"), MS.make_stream(rs, 0, 6, 1)
    check_merge(rt, ctx, full if side == "a" else none, none if side == "a" else full, None)


def test_merge_large_meshes(rt, ctx):
    """300 meshes, most of up to 3 000 vertices, twenty of up to 65 536 and one of exactly 65 536 (the largest a uint16 index reaches)."""
    rs = np.random.RandomState(5)
    nv = rs.randint(0, 3001, size=300)
    big = rs.choice(300, size=21, replace=False)
    nv[big[:20]] = rs.randint(3001, 65537, size=20)
    nv[big[20]] = 65536
    a = MS.make_stream(rs, 200, 0, 40, num_vertices=nv[:200])
    b = MS.make_stream(rs, 100, 0, 40, num_vertices=nv[200:], holes=True)
    want = check_merge(rt, ctx, a, b, None)
    assert int(want.meshes["num_vertices"].max()) == 65536 and int(want.idx.max()) > 60000


@pytest.mark.parametrize("n,max_vb,split,uv_bytes", [(1025, 4096, False, 0), (40000, 64, True, 4), (131073, 700, True, 8)])
def test_merge_armed(rt, ctx, oracle, n, max_vb, split, uv_bytes):
    """vgx_merge with draw-command assembly armed. 1 025 meshes: one launch (k_asm_small); 40 000 at 64 vertices per buffer: more than
    1 024 buffer starts; 131 073 at 700: more meshes than the one-launch route takes. The last two split the commands by the draws'
    state keys (k_asm_vb, the three-pass scan over the command starts, k_asm_cmd_finish) and carry a UV stream that b's meshes overwrite."""
    import torch
    a, b, b_draw, draws = MS.merge_case(n)
    want = MS.merge_model(a, b, b_draw)
    keys = draws["state_key"][want.meshes["draw"]] if split else None
    st, rcmds, ridx = oracle.assemble(want.meshes, want.idx, max_vb, mesh_keys=keys)
    assert st == 0
    nv = want.pos.shape[0]
    uv = b_uv = white = None
    if uv_bytes:
        uv = torch.zeros((nv + 3, 2), dtype=torch.int16 if uv_bytes == 4 else torch.float32, device=DEV)
        b_uv = MS._u32(np.random.RandomState(n), b.pos.shape[0] * (uv_bytes // 4)).reshape(-1, uv_bytes // 4)
        white = (0x7FFF0001,) if uv_bytes == 4 else (0x3F000000, 0x3E800000)
    out = Out.of(rt, want)
    armed = Armed(ctx, len(rcmds), max_vb, split, uv, white)
    try:
        run_merge(rt, ctx, a, b, b_draw, out, draws if split else None, b_uv)
    finally:
        armed.disarm()
    print("commands:", len(rcmds))
    sizes = assert_frame(out, want, idx=ridx)
    armed.assert_commands(rcmds, sizes)
    if uv_bytes:
        got = uv.cpu().numpy().view(np.uint32).reshape(nv + 3, uv_bytes // 4)
        assert np.array_equal(got[:nv], MS.merge_uv_model(want.order, a, b, b_uv, white, uv_bytes)) and not got[nv:].any()


@pytest.mark.parametrize("short", [0, 1, 2])
def test_merge_nospace(rt, ctx, short):
    a, b, b_draw, _ = MS.merge_case(1025)
    want = MS.merge_model(a, b, b_draw)
    out = Out.of(rt, want, short=short)
    run_merge(rt, ctx, a, b, b_draw, out)
    _, _, _, _, sizes, status = out.read()
    assert status == capi.VGX_E_NOSPACE
    out.assert_untouched()  # the scan finds the need before any kernel writes: nothing past a capacity means nothing at all
    assert (int(sizes[2]), int(sizes[3]), int(sizes[4])) == (1025, want.pos.shape[0], want.idx.shape[0])  # the need


@pytest.mark.parametrize("side", ["a", "b_draw"])
def test_merge_unsorted(rt, ctx, side):
    """An unsorted pair at mesh 1 024 (found by a thread of the fifth workgroup of k_merge_rank): VGX_E_INVALID_ARG."""
    rs = np.random.RandomState(31)
    a, b = MS.make_stream(rs, 1100 if side == "a" else 300, 6, 100), MS.make_stream(rs, 300 if side == "a" else 1100, 6, 100, holes=True)
    a.meshes["draw"] += np.uint32(1)
    b.meshes["draw"] += np.uint32(1)
    b_draw = None
    if side == "a":
        a.meshes["draw"][1024] = a.meshes["draw"][1023] - 1
    else:
        b_draw = b.meshes["draw"].copy()
        b_draw[1024] = b_draw[1023] - 1
    out = Out(rt, a.meshes["num_vertices"].sum() + b.meshes["num_vertices"].sum(), a.meshes["num_indices"].sum() + b.meshes["num_indices"].sum(), 1400)
    run_merge(rt, ctx, a, b, b_draw, out)
    assert out.read()[5] == capi.VGX_E_INVALID_ARG


def test_merge_mesh_too_large(rt, ctx):
    rs = np.random.RandomState(32)
    a = MS.make_stream(rs, 5, 6, 4)
    b = MS.make_stream(rs, 3, 0, 4, num_vertices=[5, 65537, 4])  # the stream really holds the 65 537 vertices
    want = MS.merge_model(a, b)
    out = Out.of(rt, want)
    run_merge(rt, ctx, a, b, None, out)
    assert out.read()[5] == capi.VGX_E_MESH_TOO_LARGE


# ---- vgx_cache_submit --------------------------------------------------------------------------------------------------------------
FRAMES = [n for n, _ in MS.CACHE_FRAMES]


@pytest.fixture
def frame(oracle):
    """cache_frame(ninst) with the oracle built; the oracle leaves no frame out (asserted here as in tests/test_mesh_streams_cpu.py)."""
    def get(ninst):
        assert ninst not in MS.left_out()
        return MS.cache_frame(ninst)
    return get


def run_submit(rt, ctx, cache, inst, out, meshes=True):
    import torch
    dc, di = DevStream(cache), to_dev(inst)
    mo = out.view.out_struct()
    if not meshes:
        mo.meshes, mo.cap_meshes = None, 0
    st = rt.lib().vgx_cache_submit(ctx.handle, C.byref(dc.desc), di.data_ptr(), inst.shape[0], C.byref(mo), out.view.dev_sizes.data_ptr(),
                                   out.view.dev_status.data_ptr(), rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == capi.VGX_OK


@pytest.mark.parametrize("ninst", FRAMES)
def test_submit(rt, ctx, frame, ninst):
    """1 024: the single-workgroup scan over the instances; 1 025 and 131 073: the three-pass one, with the empty instances [250, 520)
    across slice borders (slices of 256 instances at 1 025: the run crosses the borders at 256 and at 512; slices of 512 at 131 073: the
    border at 512), empty instances at both ends, one at first_mesh == num_meshes."""
    cache, inst, ref = frame(ninst)
    out = Out.of(rt, ref)
    run_submit(rt, ctx, cache, inst, out)
    assert_frame(out, ref)


@pytest.mark.parametrize("ninst", FRAMES)
def test_submit_armed(rt, ctx, oracle, frame, ninst):
    """Assembly armed (no draw records at this level: one state): indices per mesh with its base (k_cache_copy_idx_mesh); at 131 073
    instances behind the multi-launch assembly route."""
    cache, inst, ref = frame(ninst)
    st, rcmds, ridx = oracle.assemble(ref.meshes, ref.idx, MS.CACHE_MAX_VB)
    assert st == 0 and len(rcmds) > 1
    out = Out.of(rt, ref)
    armed = Armed(ctx, len(rcmds), MS.CACHE_MAX_VB, False)
    try:
        run_submit(rt, ctx, cache, inst, out)
    finally:
        armed.disarm()
    print("commands:", len(rcmds))
    armed.assert_commands(rcmds, assert_frame(out, ref, idx=ridx))


def test_submit_without_mesh_table(rt, ctx, frame):
    """out->meshes == NULL: the internal table is sized cache->num_meshes * ninst; streams and totals as with a table."""
    cache, inst, ref = frame(1025)
    out = Out.of(rt, ref)
    run_submit(rt, ctx, cache, inst, out, meshes=False)
    pos, color, idx, meshes, sizes, status = out.read()
    assert status == capi.VGX_OK and (int(sizes[2]), int(sizes[3]), int(sizes[4])) == (ref.meshes.shape[0], ref.pos.shape[0], ref.idx.shape[0])
    assert np.array_equal(pos, ref.pos.view(np.uint32)) and np.array_equal(color, ref.color) and np.array_equal(idx, ref.idx)
    assert np.all(meshes.view(np.uint8) == MESH_BYTE)


@pytest.mark.parametrize("short", [0, 1, 2])
def test_submit_nospace(rt, ctx, frame, short):
    cache, inst, ref = frame(1025)
    out = Out.of(rt, ref, short=short)
    run_submit(rt, ctx, cache, inst, out)
    _, _, _, _, sizes, status = out.read()
    assert status == capi.VGX_E_NOSPACE
    out.assert_untouched()  # the scan finds the need before any kernel writes: nothing past a capacity means nothing at all
    assert (int(sizes[2]), int(sizes[3]), int(sizes[4])) == (ref.meshes.shape[0], ref.pos.shape[0], ref.idx.shape[0])


@pytest.mark.parametrize("what", ["leaves_the_cache", "starts_behind_the_cache"])
def test_submit_invalid_range(rt, ctx, frame, what):
    """Instance 1 024 of 1 025 (the last occupied scan slice) names meshes the cache does not have."""
    cache, inst, ref = frame(1025)
    inst = inst.copy()
    if what == "leaves_the_cache":
        inst["first_mesh"][1024], inst["num_meshes"][1024] = MS.CACHE_MESHES - 1, 2
    else:
        inst["first_mesh"][1024], inst["num_meshes"][1024] = MS.CACHE_MESHES + 1, 0
    out = Out.of(rt, ref)
    run_submit(rt, ctx, cache, inst, out)
    assert out.read()[5] == capi.VGX_E_INVALID_ARG


# ---- vgx_cache_localize ------------------------------------------------------------------------------------------------------------
def localize(rt, ctx, draws, s):
    """vgx_cache_localize on the stream's positions between guards; returns them as uint32."""
    import torch
    nv = s.pos.shape[0]
    pos = torch.full((nv + 2 * G, 2), POS_PATTERN, dtype=torch.float32, device=DEV)
    pos[G:G + nv] = torch.from_numpy(s.pos).to(DEV)
    dd, dm = to_dev(draws), to_dev(s.meshes)
    st = rt.lib().vgx_cache_localize(ctx.handle, dd.data_ptr(), draws.shape[0], pos[G:].data_ptr(), dm.data_ptr(), s.meshes.shape[0], rt._stream_ptr())
    torch.cuda.synchronize()
    assert st == capi.VGX_OK
    got = pos.cpu().numpy()
    assert np.all(got[:G] == np.float32(POS_PATTERN)) and np.all(got[G + nv:] == np.float32(POS_PATTERN)), "pos guard"
    return got[G:G + nv].view(np.uint32)


def test_localize_past_the_grid(rt, ctx, oracle):
    """40 000 meshes: more than the 32 768 workgroups of k_cache_localize, so its loop over the meshes runs. Matrices: rotations and
    scales, a singular one, and pairs whose determinants lie just either side of +1e-6 and of -1e-6 (the reference's double-precision
    rule: inside the band the 'inverse' is {1, 0, 1, 0, 0, 0}). Which side each falls on is the oracle's decision."""
    rs = np.random.RandomState(91)
    nd = 500
    s = MS.make_stream(rs, 40000, 6, nd)
    d = np.zeros(nd, dtype=capi.draw_dtype)
    ang, sx, sy = rs.uniform(0, 6.28, size=nd), rs.uniform(0.25, 3.0, size=nd), rs.uniform(0.25, 3.0, size=nd)
    d["mtx"] = np.stack([sx * np.cos(ang), sx * np.sin(ang), -sy * np.sin(ang), sy * np.cos(ang), rs.uniform(-50, 50, size=nd), rs.uniform(-50, 50, size=nd)], axis=1)
    t = np.float32(1e-3)  # t * t = 1.0000001e-6 in double; one step below t brings the product under 1e-6
    below = np.nextafter(t, np.float32(0))
    d["mtx"][7] = [0, 0, 0, 0, 3, 4]
    d["mtx"][100], d["mtx"][101] = [t, 0, 0, t, 5, 6], [t, 0, 0, below, 5, 6]
    d["mtx"][102], d["mtx"][103] = [-t, 0, 0, t, 5, 6], [-t, 0, 0, below, 5, 6]
    want = MS.repack(s, np.arange(40000))
    oracle.cache_localize(d, want)
    rule = {}
    for k in (7, 100, 101, 102, 103):
        m = want.meshes[(want.meshes["draw"] == k) & (want.meshes["num_vertices"] > 0)]
        assert m.shape[0] > 0
        v = np.concatenate([np.arange(int(f), int(f) + int(c)) for f, c in zip(m["first_vertex"], m["num_vertices"])])
        rule[k] = bool(np.all(want.pos[v, 1] == 0))  # the singular rule maps every point to (x + y, 0)
    assert rule == {7: True, 100: False, 101: True, 102: False, 103: True}
    assert np.array_equal(localize(rt, ctx, d, s), want.pos.view(np.uint32))


def test_localize_skips_a_mesh_of_no_draw(rt, ctx):
    """A record with draw >= ndraws is left as it is (the oracle rejects such a record, so it is not asked)."""
    rs = np.random.RandomState(92)
    s = MS.make_stream(rs, 3, 0, 1, num_vertices=[4, 70, 5])
    d = np.zeros(2, dtype=capi.draw_dtype)
    d["mtx"][:] = [2, 0, 0, 4, 1, 1]
    s.meshes["draw"] = [0, 2, 1]
    got = localize(rt, ctx, d, s).view(np.float32)
    assert np.array_equal(got[4:74].view(np.uint32), s.pos[4:74].view(np.uint32))
    moved = np.concatenate([s.pos[:4], s.pos[74:]])
    want = np.stack([np.float32(0.5) * moved[:, 0] + np.float32(-0.5), np.float32(0.25) * moved[:, 1] + np.float32(-0.25)], axis=1)
    assert np.array_equal(np.concatenate([got[:4], got[74:]]), want)  # powers of two: the inverse and the products are exact
