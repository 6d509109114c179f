"""GPU: vgx_merge_uv_stream -- vgx_merge with a UV stream of the caller's beside pos / color -- on the merge inputs of
tests/mesh_streams.py: pos / color / idx / meshes are vgx_merge's (merge_model), out_uv holds b_uv at the merged places of the
vertices of b's meshes and its fill pattern everywhere else, the guards around it included, for both uv_bytes. With draw-command
assembly armed the frame and the commands are the ones vgx_merge gives and the assembly's own UV stream is not written."""
import importlib

import numpy as np
import pytest

import mesh_streams as MS
import test_gpu_mesh_streams as GS

pytestmark = pytest.mark.gpu
capi = MS.capi
G = GS.G
DEV = GS.DEV
UV_WORD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def ctx(rt):
    c = rt.Context(0)
    yield c
    c.close()


def run(rt, ctx, a, b, b_draw, out, b_uv, uv_bytes, draws=None):
    """One vgx_merge_uv_stream call into `out` and a guarded UV stream of exactly out's vertex count; returns that stream as uint32 words
    [G + nv + G, uv_bytes / 4]."""
    import torch
    words = uv_bytes // 4
    nv = out.n[0]
    uv_all = torch.full(((nv + 2 * G) * words,), UV_WORD, dtype=torch.int32, device=DEV)
    da, db = GS.DevStream(a), GS.DevStream(b)
    bd = GS.to_dev(np.ascontiguousarray(b_draw, dtype=np.uint32)) if b_draw is not None else None
    dd = GS.to_dev(draws) if draws is not None else None
    rt.merge_uv_stream(ctx, da.desc, db.desc, bd, GS.to_dev(b_uv), uv_bytes, dd, 0 if draws is None else draws.shape[0], out.view, uv_all[G * words:])
    torch.cuda.synchronize()
    return uv_all.cpu().numpy().view(np.uint32).reshape(nv + 2 * G, words)


def b_uvs(b, uv_bytes, seed):
    return MS._u32(np.random.RandomState(seed), max(b.pos.shape[0], 1) * (uv_bytes // 4)).reshape(-1, uv_bytes // 4)


def assert_uv(got, want_order, a, b, b_uv, uv_bytes):
    nv = got.shape[0] - 2 * G
    assert np.all(got[:G] == UV_WORD) and np.all(got[G + nv:] == UV_WORD), "uv guard"
    want = MS.merge_uv_model(want_order, a, b, b_uv, (UV_WORD, UV_WORD), uv_bytes)
    assert np.array_equal(got[G:G + nv], want)
    assert int((want != UV_WORD).any(axis=1).sum()) > 0 or b.meshes["num_vertices"].sum() == 0


@pytest.mark.parametrize("uv_bytes", [4, 8])
@pytest.mark.parametrize("n", [1025, 40000])
def test_equals_merge_and_writes_only_bs_vertices(rt, ctx, n, uv_bytes):
    """1 025 meshes: the first size of the three-pass scan; 40 000: b has holes, so the source places of its UVs are not packed."""
    a, b, b_draw, _ = MS.merge_case(n)
    want = MS.merge_model(a, b, b_draw)
    b_uv = b_uvs(b, uv_bytes, n)
    out = GS.Out.of(rt, want)
    got = run(rt, ctx, a, b, b_draw, out, b_uv, uv_bytes)
    GS.assert_frame(out, want)
    assert_uv(got, want.order, a, b, b_uv, uv_bytes)
    assert not np.any(b_uv == UV_WORD)  # the pattern is told apart from every UV


def test_b_draw_given(rt, ctx):
    rs = np.random.RandomState(3)
    a, b = MS.make_stream(rs, 300, 6, 50), MS.make_stream(rs, 200, 6, 50, holes=True)
    b_draw = b.meshes["draw"].copy()
    b.meshes["draw"] = MS._u32(rs, 200)
    want = MS.merge_model(a, b, b_draw)
    b_uv = b_uvs(b, 8, 5)
    out = GS.Out.of(rt, want)
    got = run(rt, ctx, a, b, b_draw, out, b_uv, 8)
    GS.assert_frame(out, want)
    assert_uv(got, want.order, a, b, b_uv, 8)


@pytest.mark.parametrize("uv_bytes,asm_uv_bytes", [(4, 8), (8, 4), (8, 8)])
def test_armed_assembly_keeps_its_own_uv_stream(rt, ctx, oracle, uv_bytes, asm_uv_bytes):
    import torch
    n, max_vb = 1025, 256
    a, b, b_draw, draws = MS.merge_case(n)
    want = MS.merge_model(a, b, b_draw)
    st, rcmds, ridx = oracle.assemble(want.meshes, want.idx, max_vb, mesh_keys=draws["state_key"][want.meshes["draw"]])
    assert st == 0
    nv = want.pos.shape[0]
    asm_uv = torch.full((nv + 3, asm_uv_bytes // 4), 0x13572468, dtype=torch.int32, device=DEV)
    b_uv = b_uvs(b, uv_bytes, 9)
    out = GS.Out.of(rt, want)
    armed = GS.Armed(ctx, len(rcmds), max_vb, True, asm_uv.view(torch.int16 if asm_uv_bytes == 4 else torch.float32), (0x7FFF0001, 0x3E800000))
    try:
        got = run(rt, ctx, a, b, b_draw, out, b_uv, uv_bytes, draws)
        sizes = GS.assert_frame(out, want, idx=ridx)
        armed.assert_commands(rcmds, sizes)
        assert_uv(got, want.order, a, b, b_uv, uv_bytes)
        assert np.all(asm_uv.cpu().numpy() == 0x13572468)  # not written by this call
        # vgx_merge_uv under the same assembly still fills it
        out2 = GS.Out.of(rt, want)
        GS.run_merge(rt, ctx, a, b, b_draw, out2, draws, b_uvs(b, asm_uv_bytes, 9))
        GS.assert_frame(out2, want, idx=ridx)
        assert not np.any(asm_uv.cpu().numpy()[:nv] == 0x13572468)
    finally:
        armed.disarm()


def test_refused_calls(rt, ctx):
    import ctypes as C
    a, b, b_draw, _ = MS.merge_case(1025)
    want = MS.merge_model(a, b, b_draw)
    out = GS.Out.of(rt, want)
    da, db = GS.DevStream(a), GS.DevStream(b)
    uv = GS.to_dev(b_uvs(b, 8, 1))
    o = out.view.out_struct()
    lib = rt.lib()

    def call(b_uv, uv_bytes, out_uv):
        return lib.vgx_merge_uv_stream(ctx.handle, C.byref(da.desc), C.byref(db.desc), None, b_uv, uv_bytes, None, 0, C.byref(o), out_uv,
                                       out.view.dev_sizes.data_ptr(), out.view.dev_status.data_ptr(), rt._stream_ptr())

    p = uv.data_ptr()
    bad = capi.VGX_E_INVALID_ARG
    assert call(None, 8, p) == bad and call(p, 8, None) == bad
    assert call(p, 0, p) == bad and call(p, 6, p) == bad and call(p + 2, 4, p) == bad and call(p, 4, p + 1) == bad
    out.assert_untouched()
