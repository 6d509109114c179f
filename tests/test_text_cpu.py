"""CPU: text, pinned without a GPU.
  1. the lane code of vgx_text_quads (csrc/vgx_text.h through libvgx_hosttest.so) against the reference's own
     vgutil::batchTransformTextQuads / vgutil::genQuadIndices_unaligned (oracle/_ref/libvgref.so) and the restated UV loop;
  2. the run matrix against the reference's State (pushState + transformTranslate played on the reference's Context);
  3. vgx_cmdlist_decode_text: Text / TextBox commands as draws + vgx_text_cmd records, against the reference's state at the command;
  4. whole frames (the device pieces played by the hosttest export and the CPU oracles) against what vg::end() hands to bgfx.
tests/test_gpu_text.py runs the kernel and the same frames through the product on the device. Nothing is compared within a tolerance."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cmdlist_util as cu
import frameref as F
import pyvgref as R
import text_frame as T
import test_gpu_concave as TC
from vgscript import Script

f32 = np.float32


@pytest.fixture(scope="module")
def rt():
    return importlib.import_module("vg-renderer_amd.runtime")


@pytest.fixture(scope="module")
def vgutil(oracle):
    if not oracle.available("reference"):
        pytest.skip("oracle/_ref is not built")
    return T.load_vgutil()


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.available("reference") or not R.available():
        pytest.skip("oracle/_ref is not built")
    return TC.load_ref(oracle)


def random_runs(capi, rng, counts):
    """Runs of the given quad counts: matrices with rotation, shear, negative determinant; scales 0.1 .. 8; dx / dy of either sign."""
    n = len(counts)
    runs = np.zeros(n, capi.text_run_dtype)
    runs["num_quads"] = counts
    runs["first_quad"] = np.cumsum(counts) - counts
    ang = rng.uniform(-np.pi, np.pi, n)
    sx, sy, sh = rng.uniform(0.2, 4.0, n), rng.uniform(0.2, 4.0, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-1.0, 1.0, n)
    m = np.zeros((n, 6))
    m[:, 0], m[:, 1] = np.cos(ang) * sx, np.sin(ang) * sx
    m[:, 2], m[:, 3] = -np.sin(ang) * sy + sh * m[:, 0], np.cos(ang) * sy + sh * m[:, 1]
    m[:, 4], m[:, 5] = rng.uniform(-500, 1500, n), rng.uniform(-500, 1000, n)
    runs["mtx"] = m.astype(f32)
    runs["x"], runs["y"] = rng.uniform(-100, 1200, n), rng.uniform(-100, 700, n)
    runs["dx"], runs["dy"] = rng.uniform(-300, 300, n), rng.uniform(-40, 40, n)
    runs["scale"] = np.where(rng.random(n) < 0.5, np.round(rng.uniform(0.1, 8.0, n), 1), rng.uniform(0.1, 8.0, n))
    runs["color"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    runs["draw"] = np.arange(n) * 3 + 1
    nq = int(np.sum(counts))
    quads = np.zeros((nq, 8), f32)
    quads[:, 0], quads[:, 1] = rng.uniform(-50, 2000, nq), rng.uniform(-60, 20, nq)
    quads[:, 2], quads[:, 3] = quads[:, 0] + rng.uniform(0.5, 40, nq).astype(f32), quads[:, 1] + rng.uniform(0.5, 60, nq).astype(f32)
    quads[:, 4:6] = rng.uniform(0, 0.9, (nq, 2))
    quads[:, 6:8] = quads[:, 4:6] + rng.uniform(0, 0.1, (nq, 2)).astype(f32)
    quads[:nq // 50 + 1, 4:8] = rng.choice([0.0, 1.0], (nq // 50 + 1, 4))  # the ends of the range FontStash produces
    return runs, quads


def assert_runs_equal(vgutil, quads, runs, pos, color, uv, idx, what=""):
    """Every run against the reference's own calls: bit patterns of positions, colours, UVs, indices."""
    ub = 0 if uv is None else uv.dtype.itemsize * 2
    for r in runs:
        q0, n, v0, i0 = int(r["first_quad"]), int(r["num_quads"]), int(r["first_vertex"]), int(r["first_index"])
        m = T.ref_matrix(r["mtx"], r["x"], r["y"], r["dx"], r["dy"], r["scale"])
        rp, rc, ru, ri = T.ref_run(vgutil, quads[q0:q0 + n], m, int(r["color"]), ub)
        assert np.array_equal(pos[v0:v0 + 4 * n].view(np.uint32), rp.view(np.uint32)), (what, "pos", q0, n)
        assert np.array_equal(color[v0:v0 + 4 * n], rc), (what, "color", q0, n)
        assert np.array_equal(idx[i0:i0 + 6 * n], ri), (what, "idx", q0, n)
        if uv is not None:
            assert np.array_equal(uv[v0:v0 + 4 * n].view(np.uint8), ru.view(np.uint8)), (what, "uv", q0, n)


# ---- 1. lane code against the reference's own functions ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(6)))
@pytest.mark.parametrize("uv", [4, 8, 0])
def test_lane_code_matches_the_reference_loops(rt, vgutil, seed, uv):
    capi = rt.capi
    rng = np.random.default_rng(1000 + seed)
    counts = np.concatenate([[1, 2, 3, 3000, 2999, 0, 7], rng.integers(1, 3001, 12), rng.integers(1, 40, 30)]).astype(np.int64)
    rng.shuffle(counts)
    runs, quads = random_runs(capi, rng, counts)
    nv, ni = rt.text_runs_dense(runs)
    assert (nv, ni) == (4 * quads.shape[0], 6 * quads.shape[0])
    assert np.array_equal(runs["first_vertex"], 4 * runs["first_quad"]) and np.array_equal(runs["first_index"], 6 * runs["first_quad"])
    pos, color, idx = np.zeros((nv, 2), f32), np.zeros(nv, np.uint32), np.zeros(ni, np.uint16)
    uvs = None if uv == 0 else np.zeros((nv, 2), np.int16 if uv == 4 else f32)
    meshes = np.zeros(runs.shape[0] + 2, capi.mesh_dtype)
    sizes = capi.Sizes()
    assert T.host_text_quads(capi, quads, runs, pos, color, uvs, idx, meshes=meshes, first_mesh=2, sizes=sizes) == 0
    assert_runs_equal(vgutil, quads, runs, pos, color, uvs, idx)
    rec = meshes[2:]
    assert np.array_equal(rec["first_vertex"], runs["first_vertex"]) and np.array_equal(rec["first_index"], runs["first_index"])
    assert np.array_equal(rec["num_vertices"], 4 * runs["num_quads"]) and np.array_equal(rec["num_indices"], 6 * runs["num_quads"])
    assert np.array_equal(rec["draw"], runs["draw"]) and (rec["subpath_kind"] == capi.MESH_TEXT << 28).all()
    assert (sizes.num_meshes, sizes.num_vertices, sizes.num_indices, sizes.num_elements) == (runs.shape[0] + 2, nv, ni, quads.shape[0])


def test_batch_reference_helpers_agree_with_the_per_run_ones(rt, vgutil):
    """tests/text_frame.py's reference_fill / ref_matrix_batch (what the GPU test compares whole buffers with) == ref_run / ref_matrix."""
    capi = rt.capi
    rng = np.random.default_rng(77)
    runs, quads = random_runs(capi, rng, rng.integers(0, 90, 300))
    rt.text_runs_dense(runs, 3, 5)
    runs["first_vertex"] += np.cumsum(rng.integers(0, 5, 300)).astype(np.uint64)
    nv, ni = int(runs["first_vertex"][-1]) + 4 * 90, int(runs["first_index"][-1]) + 6 * 90
    for uvt in (np.int16, f32):
        pos, color, idx, uv = np.zeros((nv, 2), f32), np.zeros(nv, np.uint32), np.zeros(ni, np.uint16), np.zeros((nv, 2), uvt)
        T.reference_fill(vgutil, quads, runs, np.ones(300, bool), pos, color, uv, idx)
        assert_runs_equal(vgutil, quads, runs, pos, color, uv, idx)
        hp, hc, hi, hu = np.zeros((nv, 2), f32), np.zeros(nv, np.uint32), np.zeros(ni, np.uint16), np.zeros((nv, 2), uvt)
        assert T.host_text_quads(capi, quads, runs, hp, hc, hu, hi) == 0
        assert np.array_equal(hp.view(np.uint32), pos.view(np.uint32)) and np.array_equal(hc, color) and np.array_equal(hi, idx) and np.array_equal(hu, uv)


def test_lane_code_statuses(rt):
    capi = rt.capi
    rng = np.random.default_rng(3)
    runs, quads = random_runs(capi, rng, np.asarray([5, 16385, 4]))
    rt.text_runs_dense(runs)
    nv, ni = 4 * quads.shape[0], 6 * quads.shape[0]
    pos, color, idx = np.full((nv, 2), 7.0, f32), np.zeros(nv, np.uint32), np.zeros(ni, np.uint16)
    meshes = np.zeros(3, capi.mesh_dtype)
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes) == capi.VGX_E_MESH_TOO_LARGE
    assert meshes["num_vertices"].tolist() == [20, 0, 16] and (pos[20:20 + 4 * 16385] == 7.0).all() and not (pos[:20] == 7.0).any()
    runs["num_quads"][1] = 16384
    runs["scale"][2] = 0.0
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes) == capi.VGX_E_NONFINITE
    runs["scale"][2] = 1.0
    runs["mtx"][0, 3] = np.inf
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes) == capi.VGX_E_NONFINITE
    runs["mtx"][0, 3] = 1.0
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes) == 0
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes, caps=(nv - 1, ni, 3)) == capi.VGX_E_NOSPACE
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes, caps=(nv, ni - 1, 3)) == capi.VGX_E_NOSPACE
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes, caps=(nv, ni, 2)) == capi.VGX_E_NOSPACE
    runs["first_quad"][2] -= 2  # overlaps its predecessor (which ends one quad short of it since the line above shrank it)
    assert T.host_text_quads(capi, quads, runs, pos, color, None, idx, meshes=meshes) == capi.VGX_E_INVALID_ARG


# ---- 2. the matrix against the reference's State -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(4)))
def test_run_matrix_matches_the_reference_state(rt, ref, seed):
    capi = rt.capi
    rng = np.random.default_rng(50 + seed)
    runs, _ = random_runs(capi, rng, np.ones(40, np.int64))
    lib = T.hosttest()
    lib.vgxt_text_run_matrix.restype = C.c_int
    lib.vgxt_text_run_matrix.argtypes = [C.c_void_p, C.c_void_p]
    with R.RefContext() as rc:
        rc.begin(1280, 720, 1.0)
        for k in range(runs.shape[0]):
            r = runs[k:k + 1]
            m0 = r["mtx"][0]
            scale = f32(r["scale"][0])
            s = Script().identity().mult(m0.tolist(), False).push()
            s.translate(f32(r["x"][0] + f32(r["dx"][0] / scale)), f32(r["y"][0] + f32(r["dy"][0] / scale)))
            s.play(rc, R.IMMEDIATE)
            got_state = rc.state()["mtx"].copy()
            Script().pop().play(rc, R.IMMEDIATE)
            assert np.array_equal(rc.state()["mtx"].view(np.uint32), m0.view(np.uint32))  # the state the run was recorded under
            want = got_state.copy()
            want[:4] = want[:4] * f32(f32(1.0) / scale)
            m = np.zeros(6, f32)
            assert lib.vgxt_text_run_matrix(r.ctypes.data, m.ctypes.data) == 1
            assert np.array_equal(m.view(np.uint32), want.view(np.uint32)), (k, m, want)
            assert np.array_equal(T.ref_matrix(m0, r["x"][0], r["y"][0], r["dx"][0], r["dy"][0], scale).view(np.uint32), want.view(np.uint32))
        rc.end()


# ---- 3. the decoder --------------------------------------------------------------------------------------------------------
def decoder_script():
    """Path segments around Text / TextBox commands; average scales on both sides of the 0.1 quantisation steps."""
    s = T.TextScript()
    s.begin_path().rect(10, 10, 100, 50).fill(0xFF0000FF, T.FILL_AA)
    s.text(b"plain", 10, 20, 20.0, 0xFFFFFFFF)
    for a in (0.949, 0.951, 1.449, 1.451):
        s.push().scale(a, a).rotate(0.2)
        s.text(b"scaled", 30, 40, 10.0, 0xFF00FF00, T.ALIGN_CENTER | T.ALIGN_MIDDLE)
        s.begin_path().circle(50, 50, 20).stroke(0xFFFF0000, 2.0, cu.stroke_flags(0, 0))
        s.pop()
    s.push().scale(2.0, 0.5).translate(5, 6)
    s.text_box(b"a box of text", 1, 2, 150.0, 12.0, 0xC0102030, T.ALIGN_RIGHT | T.ALIGN_TOP, font=3, flags=1)
    s.pop()
    s.global_alpha(0.5)
    s.text(b"half", 1, 2, 20.0, 0xFF445566)
    s.begin_path().rect(200, 10, 10, 10).fill(0xFF0000FF, T.FILL_AA)
    s.global_alpha(0.0)
    s.text(b"gone: alpha", 1, 2, 20.0, 0xFFFFFFFF)                 # early-out: colour alpha 0 after the global alpha
    s.global_alpha(1.0)
    s.text(b"gone: transparent", 1, 2, 20.0, 0x00FFFFFF)
    s.text(b"gone: small", 1, 2, 2.6, 0xFFFFFFFF)                   # early-out: font_size * scale < 4 (dpr 1.5: 3.9)
    s.push().scale(0.3, 0.3)
    s.text(b"gone: small after scaling", 1, 2, 8.0, 0xFFFFFFFF)     # 8 * 0.3 (* 1.5) < 4
    s.text(b"stays", 1, 2, 14.0, 0xFFFFFFFF)                        # 14 * 0.3 >= 4
    s.pop()
    s.set_scissor(10, 20, 300, 200)
    s.text(b"scissored", 50, 60, 16.0, 0xFFFFFFFF)
    s.begin_path().rect(20, 30, 50, 50).fill(0xFF00FFFF, T.FILL_AA)
    s.reset_scissor()
    s.begin_clip(0)
    s.begin_path().rect(0, 0, 400, 400).fill(0xFF000000, T.FILL_AA)
    s.text(b"inside BeginClip .. EndClip", 10, 10, 16.0, 0xFFFFFFFF)
    s.end_clip()
    s.text(b"clipped", 10, 10, 16.0, 0xFFFFFFFF)
    s.begin_path().rect(5, 5, 50, 50).fill(0xFF123456, T.FILL_AA)
    s.reset_clip()
    s.begin_path().move_to(1, 1).line_to(50, 2)
    s.text(b"while a path is being built", 10, 10, 16.0, 0xFFFFFFFF)
    s.line_to(30, 40).close_path().fill(0xFF654321, T.FILL_AA)
    return s


def reference_states(ts, dpr):
    """The reference's State at every Text / TextBox of the script (ordinary calls played in immediate mode)."""
    out = []
    with R.RefContext() as rc:
        data, strings = T.list_bytes(rc, ts)
        rc.begin(1280, 720, dpr)
        st0 = rc.state()
        for kind, v in ts.segments():
            if kind == "ops":
                v.play(rc, R.IMMEDIATE)
            else:
                out.append((v, rc.state()))
        rc.end()
        return data, strings, out, dict(state0=st0, params=rc.params(), white_uv=rc.white_uv(), font_image=rc.font_image(), uv_float=False, dpr=dpr,
                                        bytes=data, strings=strings)


def path_of(ps, p):
    c0, c1 = int(ps.path_cmd_begin[p]), int(ps.path_cmd_begin[p + 1])
    return ps.cmd_type[c0:c1].tobytes(), ps.args[int(ps.cmd_arg_off[c0]):int(ps.cmd_arg_off[c1])].tobytes()


def draw_fields(d):
    return tuple(d[k].tobytes() for k in d.dtype.names if k != "path")


@pytest.mark.parametrize("dpr", [1.0, 1.5])
def test_decoder_text_commands(rt, ref, dpr):
    capi = rt.capi
    ts = decoder_script()
    data, strings, states, refd = reference_states(ts, dpr)
    ntext = len(states)
    # the existing entry: exactly what it gives today -- text is skipped and counted
    ps0, draws0, n0, extra0 = T.decode(rt, refd, text=False)
    assert n0["skipped"] == ntext and not (draws0["fill_flags"] & capi.FILL_TEXT).any()
    ps1, draws1, n1, extra1 = T.decode(rt, refd)
    assert n1["skipped"] == 0
    texts = extra1["texts"]
    is_text = (draws1["fill_flags"] & capi.FILL_TEXT) != 0
    assert (draws1["fill_flags"][is_text] == capi.FILL_TEXT).all() and (draws1["stroke_flags"][is_text] == 0).all()
    # the path draws: the same records at shifted indices, on the same paths
    keep = np.flatnonzero(~is_text)
    assert keep.shape[0] == draws0.shape[0]
    for a, b in zip(keep, range(draws0.shape[0])):
        assert draw_fields(draws1[a]) == draw_fields(draws0[b]), (a, b)
        assert path_of(ps1, int(draws1["path"][a])) == path_of(ps0, int(draws0["path"][b])), (a, b)
        s1, s0 = extra1["draw_state"][a], extra0["draw_state"][b]
        assert all(np.array_equal(s1[k], s0[k]) for k in ("scissor", "clip_rule", "raw_color")), (a, b)
        # the clip region is a range of draw indices: the same Clip draws, at their shifted indices (text inside the range is no Clip draw)
        assert (int(s1["clip_first_draw"]) == 0xFFFFFFFF) == (int(s0["clip_first_draw"]) == 0xFFFFFFFF)
        if int(s0["clip_first_draw"]) != 0xFFFFFFFF:
            r0 = [int(keep[i]) for i in range(int(s0["clip_first_draw"]), int(s0["clip_first_draw"]) + int(s0["clip_num_draws"])) if (int(draws0["state_key"][i]) >> 16) & 3 == 3]
            r1 = [i for i in range(int(s1["clip_first_draw"]), int(s1["clip_first_draw"]) + int(s1["clip_num_draws"])) if (int(draws1["state_key"][i]) >> 16) & 3 == 3]
            assert r0 == r1, (a, b, r0, r1)
    # the survivors, in order, against the reference's state at the command
    want = []
    for j, (v, st) in enumerate(states):
        scale = f32(f32(st["font_scale"]) * f32(dpr))
        c = T.fold_alpha(v["color"], st["global_alpha"])
        if f32(f32(v["font_size"]) * scale) < T.MIN_FONT_SIZE or (c >> 24) == 0:
            continue
        want.append((v, st, scale, c, j))
    assert [w[0]["string"] for w in want] == [b"plain"] + [b"scaled"] * 4 + [b"a box of text", b"half", b"stays", b"scissored", b"inside BeginClip .. EndClip",
                                                                         b"clipped", b"while a path is being built"]
    assert texts.shape[0] == len(want) == int(is_text.sum())
    assert np.array_equal(texts["draw"], np.flatnonzero(is_text))
    # the place of every text draw: behind the path draws of the bytes in front of its command
    off = 0
    prefix_draws = []
    for kind, v in ts.segments():
        if kind == "ops":
            with R.RefContext() as rc:
                off += len(F.record(rc, v)[1])
        else:
            pre = dict(refd, bytes=data[:off])
            prefix_draws.append(T.decode(rt, pre, text=False)[1].shape[0])
            off += len(T.text_command(v, 0))
    seen_scales = set()
    assert len(prefix_draws) == ntext
    for k, (v, st, scale, c, j) in enumerate(want):
        t = texts[k]
        d = int(t["draw"])
        assert d == prefix_draws[j] + k, (k, d)
        assert strings[int(t["string_offset"]):int(t["string_offset"]) + int(t["string_len"])] == v["string"]
        assert np.array_equal(np.asarray(t["scale"], f32).view(np.uint32), np.asarray(scale, f32).view(np.uint32)), (k, t["scale"], scale)
        assert np.array_equal(t["mtx"].view(np.uint32), st["mtx"].view(np.uint32)), k
        assert int(t["color"]) == c and int(draws1["fill_color"][d]) == c
        assert (int(t["kind"]), int(t["font"]), int(t["alignment"]), int(t["textbox_flags"])) == (v["kind"], v["font"], v["alignment"], v["flags"])
        assert (f32(t["font_size"]), f32(t["x"]), f32(t["y"]), f32(t["break_width"])) == (f32(v["font_size"]), f32(v["x"]), f32(v["y"]), f32(v["break_width"]))
        key = int(draws1["state_key"][d])
        assert (key >> 16) & 3 == 0 and key & 0xFFFF == refd["font_image"], (k, hex(key))  # Textured | font image, also inside BeginClip .. EndClip
        assert extra1["draw_state"]["scissor"][d].tolist() == [int(x) for x in st["scissor"].astype(np.uint16)], k
        assert np.array_equal(draws1["mtx"][d].view(np.uint32), st["mtx"].view(np.uint32))
        seen_scales.add(round(float(st["font_scale"]), 3))
    assert {0.9, 1.0, 1.4, 1.5} <= seen_scales  # both sides of two quantisation steps
    # the generation: a text draw merges with its neighbours unless the scissor changed (state_key equal to the fill's in front of "plain")
    assert int(draws1["state_key"][1]) == int(draws1["state_key"][0])
    ds = extra1["draw_state"]
    by = {w[0]["string"]: int(texts["draw"][k]) for k, w in enumerate(want)}
    d = by[b"scissored"]
    assert int(draws1["state_key"][d]) != int(draws1["state_key"][d - 1]) and int(draws1["state_key"][d]) == int(draws1["state_key"][d + 1])
    d = by[b"inside BeginClip .. EndClip"]
    assert (int(draws1["state_key"][d - 1]) >> 16) & 3 == 3 and int(ds["clip_num_draws"][d]) == 0   # the region is still open
    d = by[b"clipped"]
    assert all(int(ds[k][d]) == int(ds[k][d + 1]) for k in ("clip_rule", "clip_first_draw", "clip_num_draws"))
    assert int(ds["clip_first_draw"][d]) != 0xFFFFFFFF and int(ds["clip_num_draws"][d]) >= 1


def test_decoder_text_rules(rt, ref):
    """Global alpha in a Cacheable list, command culling, a bad string range, a too small record array, an empty string."""
    capi = rt.capi
    ts = T.TextScript()
    ts.global_alpha(0.5)
    ts.begin_path().rect(1, 1, 20, 20).fill(0xFF0000FF, T.FILL_AA)
    ts.text(b"folds the alpha", 5, 5, 20.0, 0xFFFFFFFF)
    ts.set_scissor(0, 0, 0, 0)
    ts.begin_path().rect(1, 1, 20, 20).fill(0xFF0000FF, T.FILL_AA)   # culled under the empty scissor
    ts.text(b"not culled", 5, 5, 20.0, 0xFFFFFFFF)
    data, strings, states, refd = reference_states(ts, 1.0)
    _, draws, n, extra = T.decode(rt, refd, flags=capi.CL_CACHEABLE)
    assert draws["fill_flags"].tolist()[1] == capi.FILL_TEXT and int(draws["fill_color"][0]) >> 24 == 0xFF and int(draws["fill_color"][1]) >> 24 == 0x7F
    assert extra["texts"]["color"].tolist() == [0x7FFFFFFF, 0x7FFFFFFF]
    _, draws, n, extra = T.decode(rt, refd, flags=capi.CL_ALLOW_CULLING)
    assert [int(x) for x in draws["fill_flags"]] == [draws["fill_flags"][0], capi.FILL_TEXT, capi.FILL_TEXT] and n["skipped"] == 0
    assert extra["draw_state"]["scissor"][2].tolist() == [0, 0, 0, 0]
    # string ranges
    item = dict(kind=0, string=b"abcdef", x=1.0, y=2.0, font_size=20.0, color=0xFFFFFFFF, alignment=1, font=0, break_width=0.0, flags=0)
    dec = importlib.import_module("vg-renderer_amd.cmdlist").decode
    assert dec(rt, T.text_command(item, 0), text=dict(strings_size=6))[0] == 0
    assert dec(rt, T.text_command(item, 1), text=dict(strings_size=6))[0] == capi.VGX_E_INVALID_ARG
    assert dec(rt, T.text_command(item, 6, 0), text=dict(strings_size=6))[0] == capi.VGX_E_INVALID_ARG  # offset < size, vg.cpp:4512
    assert dec(rt, T.text_command(item, 0), text=dict(strings_size=0))[0] == capi.VGX_E_INVALID_ARG
    box = dict(item, kind=1, break_width=100.0)
    assert dec(rt, T.text_command(box, 3, 4), text=dict(strings_size=6))[0] == capi.VGX_E_INVALID_ARG
    rc, _, draws, n = dec(rt, T.text_command(item, 2, 0) + T.text_command(box, 2, 4), text=dict(strings_size=6))  # an empty string: neither a draw nor skipped
    assert rc == 0 and draws.shape[0] == 1 and n["skipped"] == 0
    assert dec(rt, T.text_command(item, 99))[0] == 0  # the existing entry does not look at text at all
    # min_font_size and the device pixel ratio
    assert dec(rt, T.text_command(item, 0), text=dict(strings_size=6, min_font_size=20.5))[2].shape[0] == 0
    assert dec(rt, T.text_command(item, 0), text=dict(strings_size=6, min_font_size=20.5, device_pixel_ratio=1.1))[2].shape[0] == 1
    # a too small record array
    data = T.text_command(item, 0) + T.text_command(item, 0)
    st = capi.CmdListState()
    st.mtx[0] = st.mtx[3] = 1.0
    st.global_alpha = 1.0; st.tess_tol = 0.25; st.fringe = 1.0; st.canvas_width, st.canvas_height = 1280.0, 720.0
    out, txt = capi.CmdListOut(), capi.CmdListText()
    txt.strings_size, txt.device_pixel_ratio = 6, 1.0
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert rt.lib().vgx_cmdlist_decode_text(buf, len(data), C.byref(st), C.byref(out), C.byref(txt)) == 0
    assert (out.num_draws, txt.num_texts, out.num_paths) == (2, 2, 1)
    draws, pcb, texts = np.zeros(2, capi.draw_dtype), np.zeros(2, np.uint32), np.zeros(2, capi.text_cmd_dtype)
    ct, ao, ar = np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.float32)
    out.cmd_type, out.cmd_arg_off, out.args, out.path_cmd_begin, out.draws = ct.ctypes.data, ao.ctypes.data, ar.ctypes.data, pcb.ctypes.data, draws.ctypes.data
    out.cap_cmds, out.cap_args, out.cap_paths, out.cap_draws = 0, 0, 1, 2
    txt.texts, txt.cap_texts = texts.ctypes.data, 1
    assert rt.lib().vgx_cmdlist_decode_text(buf, len(data), C.byref(st), C.byref(out), C.byref(txt)) == capi.VGX_E_NOSPACE
    txt.texts, txt.cap_texts = None, 2
    assert rt.lib().vgx_cmdlist_decode_text(buf, len(data), C.byref(st), C.byref(out), C.byref(txt)) == capi.VGX_E_NOSPACE
    txt.texts, txt.cap_texts = texts.ctypes.data, 2
    assert rt.lib().vgx_cmdlist_decode_text(buf, len(data), C.byref(st), C.byref(out), C.byref(txt)) == 0
    assert texts["draw"].tolist() == [0, 1] and texts["string_len"].tolist() == [6, 6]


# ---- 4. whole frames on the CPU ------------------------------------------------------------------------------------------------
def cpu_frame(rt, oracle, ref, ts, max_vb, uv_float):
    refd = T.reference_frame(ts, max_vb=max_vb, uv_float=uv_float)
    ps, draws, n, extra = T.decode(rt, refd)
    assert n["skipped"] == 0
    ext, runs = T.external_meshes(rt.capi, draws, extra, refd["strings"], uv_float, T.host_text_fn(rt.capi))
    assert runs.shape[0] == refd["num_runs"]
    pos, col, idx, meshes, cmds, uv = T.compose(oracle, ref, refd, ps, draws, ext, max_vb)
    F.assert_frame_equal(refd["frame"], pos, col, idx, meshes, cmds, draws, extra["draw_state"], max_vb, uv=uv)
    return draws, extra, meshes, cmds, runs


def merged_and_apart(capi, draws, meshes, cmds):
    """(a draw command holds a text mesh AND a mesh of a colour fill / stroke, two consecutive commands differ in nothing but the
    scissor generation with text on one side)."""
    kind = meshes["subpath_kind"] >> 28
    merged = apart = False
    for k, c in enumerate(cmds):
        ks = kind[int(c["first_mesh"]):int(c["first_mesh"]) + int(c["num_meshes"])]
        if (ks == capi.MESH_TEXT).any() and (ks <= capi.MESH_STROKE_AA_THIN).any():
            merged = True
        if k and (int(c["state_key"]) ^ int(cmds[k - 1]["state_key"])) >> 20 and (int(c["state_key"]) & 0xFFFFF) == (int(cmds[k - 1]["state_key"]) & 0xFFFFF) \
                and int(c["vertex_buffer"]) == int(cmds[k - 1]["vertex_buffer"]) and (ks == capi.MESH_TEXT).any():
            apart = True
    return merged, apart


@pytest.mark.parametrize("uv_float", [False, True])
@pytest.mark.parametrize("max_vb", [65536, 512])
def test_text_scenario_cpu(rt, oracle, ref, max_vb, uv_float):
    draws, extra, meshes, cmds, runs = cpu_frame(rt, oracle, ref, T.s_text(uv_float), max_vb, uv_float)
    assert extra["texts"].shape[0] == 11 and runs.shape[0] > extra["texts"].shape[0]  # TextBox rows: several runs per draw
    assert merged_and_apart(rt.capi, draws, meshes, cmds) == (True, True)
    kind = meshes["subpath_kind"] >> 28
    assert kind[0] == rt.capi.MESH_TEXT and kind[-1] == rt.capi.MESH_TEXT   # text as the first and as the last thing in the frame
    if max_vb == 512:  # a vertex-buffer split between two runs of one TextBox draw
        vb = np.zeros(meshes.shape[0], np.int64)
        for c in cmds:
            vb[int(c["first_mesh"]):int(c["first_mesh"]) + int(c["num_meshes"])] = int(c["vertex_buffer"])
        t = np.flatnonzero(kind == rt.capi.MESH_TEXT)
        assert any(meshes["draw"][a] == meshes["draw"][b] and vb[a] != vb[b] for a, b in zip(t[:-1], t[1:]))


@pytest.mark.parametrize("uv_float", [False, True])
def test_frame_of_nothing_but_text_cpu(rt, oracle, ref, uv_float):
    draws, extra, meshes, cmds, runs = cpu_frame(rt, oracle, ref, T.s_text_only(), 65536, uv_float)
    assert ((meshes["subpath_kind"] >> 28) == rt.capi.MESH_TEXT).all() and len(cmds) == 1


@pytest.mark.parametrize("seed", list(range(14)))
def test_random_text_frames_cpu(rt, oracle, ref, seed):
    cpu_frame(rt, oracle, ref, T.s_random(300 + seed, bool(seed & 1)), 65536 if seed % 3 else 768, bool(seed & 1))
