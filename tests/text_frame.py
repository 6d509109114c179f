"""Text in frames (TEST INFRASTRUCTURE): the reference's own text helpers through ctypes, a deterministic stand-in for the
caller's FontStash, scripts with Text / TextBox commands, and both sides of a frame comparison.

What the reference does with a string (ctxText, reference src/vg.cpp:4177-4232; renderTextQuads :5541-5621):
  FontStash shapes it into glyph quads + an alignment offset (dx, dy)                                  [caller's side: `shape` here]
  pushState; transformTranslate(x + dx / scale, y + dy / scale); m[0..3] *= 1 / scale;
  vgutil::batchTransformTextQuads, colour x 4, UVs, vgutil::genQuadIndices_unaligned; popState          [vgx_text_quads]
The oracle libraries have no font entry point (oracle/ref_vg_capi.cpp), but at the level of what vg::end() hands to bgfx a run
is bit for bit what the reference makes of
  pushState; transformTranslate(x + dx / scale, y + dy / scale); transformScale(1 / scale, 1 / scale);
  indexedTriList(quad corners, one colour, quad indices, UVs, invalid image = the font atlas); popState
so whole frames with text are pinned against the reference's unmodified vg.cpp with that sequence in the place of each run."""
import ctypes as C
import importlib
import os
import struct

import numpy as np

import cmdlist_util as cu
import frameref as F
import pyvgref as R
from vgscript import Script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# FONSalign
ALIGN_LEFT, ALIGN_CENTER, ALIGN_RIGHT, ALIGN_TOP, ALIGN_MIDDLE, ALIGN_BOTTOM, ALIGN_BASELINE = 1, 2, 4, 8, 16, 32, 64
MIN_FONT_SIZE = f32(4.0)  # VG_CONFIG_MIN_FONT_SIZE

FILL_AA = cu.fill_flags(aa=True)
FILL_CONCAVE_AA = cu.fill_flags(concave=True, aa=True)


# ---- the reference's own loops (src/vg_util.cpp, compiled where it lies into oracle/_ref/libvgref.so) ---------------------------
def load_vgutil():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(R.__file__)), "_ref", "libvgref.so"))
    bt = getattr(lib, "_ZN6vgutil23batchTransformTextQuadsEPKfjS1_Pf")   # vgutil::batchTransformTextQuads(const float*, unsigned, const float*, float*)
    bt.restype = None
    bt.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    gq = getattr(lib, "_ZN6vgutil24genQuadIndices_unalignedEPtjt")        # vgutil::genQuadIndices_unaligned(uint16_t*, unsigned, uint16_t)
    gq.restype = None
    gq.argtypes = [C.c_void_p, C.c_uint32, C.c_uint16]
    return bt, gq


def ref_matrix(mtx, x, y, dx, dy, scale):
    """The matrix renderTextQuads hands to batchTransformTextQuads, in float32 numpy in the reference's order:
    ctxTransformTranslate(x + dx / scale, y + dy / scale) (vg.cpp:4229, 4058-4059), then m[0..3] * (1.0f / scale) (:5545-5558)."""
    m = np.asarray(mtx, f32).copy()
    x, y, dx, dy, scale = f32(x), f32(y), f32(dx), f32(dy), f32(scale)
    tx = f32(x + f32(dx / scale))
    ty = f32(y + f32(dy / scale))
    m4 = f32(m[4] + f32(f32(m[0] * tx) + f32(m[2] * ty)))
    m5 = f32(m[5] + f32(f32(m[1] * tx) + f32(m[3] * ty)))
    inv = f32(f32(1.0) / scale)
    return np.asarray([m[0] * inv, m[1] * inv, m[2] * inv, m[3] * inv, m4, m5], f32)


def ref_matrix_batch(runs):
    """ref_matrix for an array of vgx_text_run records: [n, 6] float32, the same operations in the same order."""
    m = runs["mtx"].astype(f32)
    x, y, dx, dy, scale = (runs[k].astype(f32) for k in ("x", "y", "dx", "dy", "scale"))
    with np.errstate(all="ignore"):
        tx = x + dx / scale
        ty = y + dy / scale
        out = np.zeros((runs.shape[0], 6), f32)
        out[:, 4] = m[:, 4] + (m[:, 0] * tx + m[:, 2] * ty)
        out[:, 5] = m[:, 5] + (m[:, 1] * tx + m[:, 3] * ty)
        inv = f32(1.0) / scale
        out[:, :4] = m[:, :4] * inv[:, None]
    return out


def reference_fill(vgutil, quads, runs, write, pos, color, uv, idx):
    """The runs with write[r] set, by the reference's own functions, at their places in pos / color / uv / idx (in place; every
    other byte of the arrays stays as it is)."""
    bt, gq = vgutil
    q = np.ascontiguousarray(quads, f32).reshape(-1, 8)
    M = np.ascontiguousarray(ref_matrix_batch(runs))
    uvall = ref_uv(q, uv.dtype.itemsize * 2) if uv is not None else None
    assert pos.flags.c_contiguous and idx.flags.c_contiguous and pos.dtype == f32 and idx.dtype == np.uint16
    for r in np.flatnonzero(write):
        q0, n, v0, i0 = int(runs["first_quad"][r]), int(runs["num_quads"][r]), int(runs["first_vertex"][r]), int(runs["first_index"][r])
        if not n:
            continue
        bt(q.ctypes.data + 32 * q0, n, M.ctypes.data + 24 * int(r), pos.ctypes.data + 8 * v0)
        gq(idx.ctypes.data + 2 * i0, n, 0)
        color[v0:v0 + 4 * n] = runs["color"][r]
        if uv is not None:
            uv[v0:v0 + 4 * n] = uvall[4 * q0:4 * (q0 + n)]


def ref_uv(quads, uv_bytes):
    """vg.cpp:5587-5590 ((int16_t)(s * INT16_MAX), truncation) / :5605-5608 restated: (s0,t0) (s1,t0) (s1,t1) (s0,t1) per quad."""
    q = np.asarray(quads, f32).reshape(-1, 8)
    st = q[:, [4, 5, 6, 5, 6, 7, 4, 7]].reshape(-1, 2)
    if uv_bytes == 8:
        return st.copy()
    return (st * f32(32767)).astype(np.int32).astype(np.int16)  # float -> integer conversion truncates towards zero


def ref_run(vgutil, quads, mtx6, color, uv_bytes):
    """One renderTextQuads call by the reference's own functions: (pos [4n,2], color [4n], uv [4n,2] or None, idx [6n])."""
    bt, gq = vgutil
    q = np.ascontiguousarray(quads, f32).reshape(-1, 8)
    n = q.shape[0]
    pos = np.zeros((4 * n, 2), f32)
    idx = np.zeros(6 * n, np.uint16)
    m = np.ascontiguousarray(mtx6, f32)
    if n:
        bt(q.ctypes.data, n, m.ctypes.data, pos.ctypes.data)
        gq(idx.ctypes.data, n, 0)
    return pos, np.full(4 * n, color, np.uint32), (ref_uv(q, uv_bytes) if uv_bytes else None), idx


# ---- the lane code on the host (vg-renderer_amd/libvgx_hosttest.so: csrc/vgx_text.h driven over whole arrays) ---------------------
def hosttest():
    lib = C.CDLL(os.path.join(ROOT, "vg-renderer_amd", "libvgx_hosttest.so"))
    lib.vgxt_text_quads.restype = C.c_int
    return lib


def host_text_quads(capi, quads, runs, pos, color, uv, idx, meshes=None, first_mesh=0, caps=None, sizes=None):
    """vgxt_text_quads on numpy arrays, written in place. uv: int16 / float32 [nv,2] or None. caps: (vertices, indices, meshes)."""
    lib = hosttest()
    q = np.ascontiguousarray(quads, f32).reshape(-1, 8)
    caps = caps or (pos.shape[0], idx.shape[0], meshes.shape[0] if meshes is not None else 0)
    out = capi.MeshOut(pos.ctypes.data, color.ctypes.data, idx.ctypes.data, meshes.ctypes.data if meshes is not None else None, caps[0], caps[1], caps[2])
    ub = 0 if uv is None else (8 if uv.dtype == np.float32 else 4)
    lib.vgxt_text_quads.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(capi.MeshOut), C.c_void_p, C.c_uint32, C.c_void_p]
    return lib.vgxt_text_quads(q.ctypes.data, q.shape[0], runs.ctypes.data, runs.shape[0], first_mesh, C.byref(out),
                               uv.ctypes.data if uv is not None else None, ub, C.byref(sizes) if sizes is not None else None)


# ---- the caller's FontStash, played by a deterministic stand-in --------------------------------------------------------
def _row(bs, size):
    """Glyph quads of one row of bytes at pen 0 (FONSquad: x0 y0 x1 y1 s0 t0 s1 t1) and the row's width. Blanks advance only."""
    pen = f32(0)
    out = []
    for b in bs:
        adv = f32(size * f32(0.35 + 0.05 * (b % 7)))
        if b != 32:
            s0 = f32((b % 16) / 16.0 + 1 / 64.0)
            t0 = f32(((b // 16) % 16) / 16.0 + 1 / 64.0)
            out.append([pen + f32(size * f32(0.04)), f32(-size * f32(0.75)) + f32(b % 3), pen + adv, f32(size * f32(0.2)),
                        s0, t0, f32(s0 + f32(3 / 64.0)), f32(t0 + f32(3 / 64.0))])
        pen = f32(pen + adv)
    return np.asarray(out, f32).reshape(-1, 8), pen


def _align(a, width, size):
    dx = f32(0) if a & ALIGN_LEFT else (f32(-width * f32(0.5)) if a & ALIGN_CENTER else (f32(-width) if a & ALIGN_RIGHT else f32(0)))
    dy = f32(size * f32(0.75)) if a & ALIGN_TOP else (f32(size * f32(0.25)) if a & ALIGN_MIDDLE else (f32(-size * f32(0.2)) if a & ALIGN_BOTTOM else f32(0)))
    return dx, dy


def shape(kind, string, font_size, scale, alignment, x, y, break_width):
    """string -> [(x, y, dx, dy, quads)]: one run for a Text, one per row for a TextBox with ctxTextBox's per-row x / y and the
    FONS_ALIGN_LEFT | valign alignment (vg.cpp:4245-4267). What it computes does not matter, only that both sides get the same."""
    font_size, scale, x, y, break_width = f32(font_size), f32(scale), f32(x), f32(y), f32(break_width)
    size = f32(font_size * scale)
    bs = list(bytes(string))
    if kind == 0:
        q, w = _row(bs, size)
        dx, dy = _align(alignment, w, size)
        return [(x, y, dx, dy, q)] if q.shape[0] else []
    halign, valign = alignment & 7, alignment & 0x78
    lineh = f32(font_size * f32(1.25))
    rows, cur = [], []
    for b in bs:  # textBreakLines: as many glyphs as fit into break_width, one at least
        if cur and f32(_row(cur + [b], size)[1] / scale) > break_width:
            rows.append(cur)
            cur = []
        cur.append(b)
    if cur:
        rows.append(cur)
    runs = []
    for r in rows:
        q, w = _row(r, size)
        roww = f32(w / scale)
        rx = x if halign & ALIGN_LEFT else (f32(x + f32(f32(break_width - roww) * f32(0.5))) if halign & ALIGN_CENTER else f32(f32(x + break_width) - roww))
        dx, dy = _align(ALIGN_LEFT | valign, w, size)
        if q.shape[0]:
            runs.append((rx, y, dx, dy, q))
        y = f32(y + lineh)
    return runs


def quad_mesh(quads, uv_float):
    """The indexedTriList arguments a run is on the reference's side: corners, quad indices, UVs of the build's uv_t."""
    q = np.asarray(quads, f32).reshape(-1, 8)
    pos = q[:, [0, 1, 2, 1, 2, 3, 0, 3]].reshape(-1, 2).copy()
    b = (4 * np.arange(q.shape[0], dtype=np.uint32))[:, None]
    idx = (b + np.asarray([0, 1, 2, 0, 2, 3], np.uint32)[None, :]).astype(np.uint16).reshape(-1)
    return pos, idx, ref_uv(q, 8 if uv_float else 4)


def fold_alpha(color, global_alpha):
    """colorSetAlpha(color, (uint8_t)(globalAlpha * colorGetAlpha(color))), vg.cpp:5547."""
    a = int(f32(f32(global_alpha) * f32((color >> 24) & 0xFF))) & 0xFF
    return (color & 0x00FFFFFF) | (a << 24)


# ---- scripts with text ----------------------------------------------------------------------------------------------------
class TextScript(Script):
    """A vgscript.Script that may hold Text / TextBox items between its ordinary calls."""

    def text(self, string, x, y, font_size=18.0, color=0xFFFFFFFF, alignment=ALIGN_LEFT | ALIGN_BASELINE, font=0):
        self.ops.append(("TEXT", dict(kind=0, string=bytes(string), x=x, y=y, font_size=font_size, color=color, alignment=alignment, font=font,
                                      break_width=0.0, flags=0)))
        return self

    def text_box(self, string, x, y, break_width, font_size=18.0, color=0xFFFFFFFF, alignment=ALIGN_LEFT | ALIGN_BASELINE, font=0, flags=0):
        self.ops.append(("TEXT", dict(kind=1, string=bytes(string), x=x, y=y, font_size=font_size, color=color, alignment=alignment, font=font,
                                      break_width=break_width, flags=flags)))
        return self

    def segments(self):
        """[("ops", Script) | ("text", item)] in order."""
        out = []
        for op in self.ops:
            if op[0] == "TEXT":
                out.append(("text", op[1]))
            else:
                if not out or out[-1][0] != "ops":
                    out.append(("ops", Script()))
                out[-1][1].ops.append(op)
        return out


def text_command(item, offset, length=None):
    """clText / clTextBox's record (vg.cpp:2914-2957): TextConfig{uint16 font, float size, uint32 alignment, Color}, x, y[, breakWidth],
    string offset, length[, flags], behind the 16-byte header, padded to 16 bytes (clAllocCommand, :5694-5723)."""
    r = cu.Recorder()
    cfg = struct.pack("<HxxfII", item["font"], item["font_size"], item["alignment"], item["color"])
    n = len(item["string"]) if length is None else length
    if item["kind"] == 0:
        r._cmd("Text", cfg + struct.pack("<ffII", item["x"], item["y"], offset, n))
    else:
        r._cmd("TextBox", cfg + struct.pack("<fffIII", item["x"], item["y"], item["break_width"], offset, n, item["flags"]))
    return r.bytes()


def list_bytes(rc, ts):
    """The script as command-list bytes: ordinary calls recorded by the reference's own writers, Text / TextBox commands written
    here and spliced in between (every record is a 16-byte aligned unit, so the concatenation is a valid list). Returns
    (bytes, string buffer)."""
    data, strings = b"", b""
    for kind, v in ts.segments():
        if kind == "ops":
            cl, b = F.record(rc, v)
            data += b
        elif len(v["string"]):  # clText returns before it writes anything for an empty string (:2921-2923)
            data += text_command(v, len(strings))
            strings += v["string"]
    return data, strings


def play_reference(rc, ts, dpr, uv_float):
    """The script on the reference's Context in immediate mode, every run replaced by its push / translate / scale / indexedTriList /
    pop sequence; ctxText's early-outs (vg.cpp:4183-4191, 5547-5550) restated. Returns the number of runs played."""
    nruns = 0
    for kind, v in ts.segments():
        if kind == "ops":
            v.play(rc, R.IMMEDIATE)
            continue
        st = rc.state()
        scale = f32(f32(st["font_scale"]) * f32(dpr))
        if f32(f32(v["font_size"]) * scale) < MIN_FONT_SIZE or not len(v["string"]):
            continue
        c = fold_alpha(v["color"], st["global_alpha"])
        if (c >> 24) == 0:
            continue
        for (x, y, dx, dy, q) in shape(v["kind"], v["string"], v["font_size"], scale, v["alignment"], v["x"], v["y"], v["break_width"]):
            pos, idx, uv = quad_mesh(q, uv_float)
            inv = f32(f32(1.0) / scale)
            s = Script().push().translate(f32(x + f32(dx / scale)), f32(y + f32(dy / scale))).scale(inv, inv)
            s.indexed_tri_list(pos, [c], idx, uv=uv, image=0xFFFF).pop()
            s.play(rc, R.IMMEDIATE)
            nruns += 1
    return nruns


def reference_frame(ts, max_vb=65536, uv_float=False, images=6, dpr=1.0, canvas=(1280, 720)):
    """One frame of the script on the reference + the product's input (bytes, strings). A dict like frameref.reference_frame's."""
    with R.RefContext(max_vb_vertices=max_vb, uv_float=uv_float) as rc:
        img = [rc.create_image(8, 8) for _ in range(images)]
        assert all(h != 0xFFFF for h in img)
        data, strings = list_bytes(rc, ts)
        rc.begin(canvas[0], canvas[1], dpr)
        st0 = rc.state()
        nruns = play_reference(rc, ts, dpr, uv_float)
        fr = rc.end()
        return dict(frame=fr, bytes=data, strings=strings, lists={}, root=None, params=rc.params(), state0=st0, white_uv=rc.white_uv(),
                    font_image=rc.font_image(), uv_float=uv_float, dpr=dpr, num_runs=nruns)


def decode(rt, refd, canvas=(1280, 720), flags=0, text=True):
    """vgx_cmdlist_decode_text (text=False: vgx_cmdlist_decode) of the frame's bytes under the state the reference had."""
    st0 = refd["state0"]
    extra = {}
    rc, ps, draws, n = cu.decode(rt, refd["bytes"], mtx=st0["mtx"].tolist(), global_alpha=st0["global_alpha"], tess_tol=refd["params"]["tess_tol"],
                                 fringe=refd["params"]["fringe"], canvas=(float(canvas[0]), float(canvas[1])), flags=flags, extra=extra,
                                 white_uv=refd["white_uv"][0], font_image=refd["font_image"], uv_float=refd["uv_float"],
                                 text=dict(strings_size=len(refd["strings"]), device_pixel_ratio=refd["dpr"]) if text else None)
    assert rc == 0, rc
    return ps, draws, n, extra


def external_meshes(capi, draws, extra, strings, uv_float, text_fn):
    """The frame's ONE sequence of external meshes, sorted by draw: the decoder's user meshes copied to their places, the text
    runs (shaped from the vgx_text_cmd records) written at theirs by text_fn(quads, runs, pos, color, uv, idx). Returns the
    sequence in the shape of the decoder's tri_* arrays + the runs."""
    tri, texts = extra["tri"], extra["texts"]
    items = [(int(m["draw"]), 0, k, None) for k, m in enumerate(tri["meshes"])]
    for t in texts:
        assert int(draws["fill_flags"][int(t["draw"])]) == capi.FILL_TEXT
        s = strings[int(t["string_offset"]):int(t["string_offset"]) + int(t["string_len"])]
        for run in shape(int(t["kind"]), s, t["font_size"], t["scale"], int(t["alignment"]), t["x"], t["y"], t["break_width"]):
            items.append((int(t["draw"]), 1, t, run))
    items.sort(key=lambda it: it[0])  # stable: the runs of one TextBox keep their order
    meshes = np.zeros(len(items), capi.mesh_dtype)
    runs, quads = [], []
    v = i = nq = 0
    for k, (d, what, a, run) in enumerate(items):
        if what == 0:
            nv, ni, kindbits = int(tri["meshes"]["num_vertices"][a]), int(tri["meshes"]["num_indices"][a]), capi.MESH_TRILIST << 28
        else:
            n = run[4].shape[0]
            nv, ni, kindbits = 4 * n, 6 * n, capi.MESH_TEXT << 28
            r = np.zeros(1, capi.text_run_dtype)
            r["first_quad"], r["num_quads"], r["color"], r["mtx"], r["scale"], r["draw"] = nq, n, a["color"], a["mtx"], a["scale"], d
            r["x"], r["y"], r["dx"], r["dy"] = run[0], run[1], run[2], run[3]
            r["first_vertex"], r["first_index"] = v, i
            runs.append(r)
            quads.append(run[4])
            nq += n
        meshes[k] = (v, i, nv, ni, d, kindbits)
        v += nv
        i += ni
    uvt = np.float32 if uv_float else np.int16
    pos, color, uv, idx = np.zeros((v, 2), f32), np.zeros(v, np.uint32), np.zeros((v, 2), uvt), np.zeros(i, np.uint16)
    for k, (d, what, a, run) in enumerate(items):
        if what == 0:
            m, o = tri["meshes"][a], meshes[k]
            sv, si = slice(int(m["first_vertex"]), int(m["first_vertex"]) + int(m["num_vertices"])), slice(int(m["first_index"]), int(m["first_index"]) + int(m["num_indices"]))
            dv, di = slice(int(o["first_vertex"]), int(o["first_vertex"]) + int(o["num_vertices"])), slice(int(o["first_index"]), int(o["first_index"]) + int(o["num_indices"]))
            pos[dv], color[dv], uv[dv], idx[di] = tri["pos"][sv], tri["color"][sv], tri["uv"][sv], tri["idx"][si]
    runs = np.concatenate(runs) if runs else np.zeros(0, capi.text_run_dtype)
    quads = np.concatenate(quads) if quads else np.zeros((0, 8), f32)
    if runs.shape[0]:
        pos, color, uv, idx = text_fn(quads, runs, pos, color, uv, idx)
    return dict(pos=pos, color=color, uv=uv, idx=idx, meshes=meshes), runs


def host_text_fn(capi):
    def fn(quads, runs, pos, color, uv, idx):
        assert host_text_quads(capi, quads, runs, pos, color, uv, idx) == 0
        return pos, color, uv, idx
    return fn


def gpu_text_fn(rt, ctx):
    """vgx_text_quads into device buffers that already hold the user meshes at their places."""
    def fn(quads, runs, pos, color, uv, idx):
        import torch
        dev = torch.device("cuda", 0)
        bufs = rt.MeshBuffers(dev, pos.shape[0], idx.shape[0], runs.shape[0])
        bufs.pos[:pos.shape[0]] = torch.from_numpy(pos).to(dev)
        bufs.color[:color.shape[0]] = torch.from_numpy(color.view(np.int32)).to(dev)
        bufs.idx[:idx.shape[0]] = torch.from_numpy(idx.view(np.int16)).to(dev)
        uvd = torch.from_numpy(uv).to(dev)
        qd = torch.from_numpy(np.ascontiguousarray(quads)).to(dev)
        rd = torch.from_numpy(runs.view(np.uint8).copy()).to(dev)
        rt.text_quads(ctx, qd, quads.shape[0], rd, runs.shape[0], bufs, uv_dev=uvd, uv_bytes=uv.dtype.itemsize * 2)
        torch.cuda.synchronize()
        assert int(bufs.dev_status.item()) == 0, int(bufs.dev_status.item())
        rec = bufs.meshes[:runs.shape[0] * 32].cpu().numpy().view(rt.capi.mesh_dtype)
        assert np.array_equal(rec["first_vertex"], runs["first_vertex"]) and np.array_equal(rec["num_indices"], 6 * runs["num_quads"])
        assert np.array_equal(rec["draw"], runs["draw"]) and (rec["subpath_kind"] == rt.capi.MESH_TEXT << 28).all()
        return (bufs.pos[:pos.shape[0]].cpu().numpy(), bufs.color[:color.shape[0]].cpu().numpy().view(np.uint32), uvd.cpu().numpy(),
                bufs.idx[:idx.shape[0]].cpu().numpy().view(np.uint16))
    return fn


def compose(oracle, ref, refd, ps, draws, ext, max_vb):
    """The CPU frame: sequence A (oracle tessellation) + concave fills (reference stroker + libtess2) + the external sequence, merged
    by draw and assembled by the oracle's assembler (as tests/test_trilist_frame_cpu.py composes its frames)."""
    import concave_frame as CF
    import test_gpu_concave as TC
    capi = importlib.import_module("vg-renderer_amd.runtime").capi
    A = oracle.tessellate(ps, draws)
    seq = []
    for m in A.meshes:
        v0, nv, i0, ni = int(m["first_vertex"]), int(m["num_vertices"]), int(m["first_index"]), int(m["num_indices"])
        seq.append((int(m["draw"]), 0, A.pos[v0:v0 + nv], A.color[v0:v0 + nv], A.idx[i0:i0 + ni], int(m["subpath_kind"]), None))
    cidx = np.flatnonzero((draws["fill_flags"] & capi.FILL_CONCAVE) != 0)
    if cidx.shape[0]:
        fl = oracle.flatten(ps, draws[cidx], apply_transform=True)
        for k, di in enumerate(cidx):
            info = fl.draw_info[k]
            subs = fl.subpaths[int(info["first_subpath"]):int(info["first_subpath"]) + int(info["num_subpaths"])]
            if subs.shape[0] == 0 or (subs["num_vertices"] < 3).any():
                continue
            contours = [fl.poly[int(s["first_vertex"]):int(s["first_vertex"]) + int(s["num_vertices"])] for s in subs]
            ff = int(draws["fill_flags"][di])
            eo = 1 if ff & capi.FILL_EVEN_ODD else 0
            col = int(draws["fill_color"][di])
            if ff & capi.FILL_AA:
                pos, c, idx = TC._reference_mesh(ref, contours, col, float(draws["fringe"][di]), eo)
            else:
                pos, idx = CF._polygons(ref, contours, eo)
                c = np.full(pos.shape[0], col, np.uint32)
            seq.append((int(di), 1, pos, c, idx, capi.MESH_CONCAVE_FILL_AA << 28, None))
    for k, m in enumerate(ext["meshes"]):
        v0, nv, i0, ni = int(m["first_vertex"]), int(m["num_vertices"]), int(m["first_index"]), int(m["num_indices"])
        seq.append((int(m["draw"]), 2 + k, ext["pos"][v0:v0 + nv], ext["color"][v0:v0 + nv], ext["idx"][i0:i0 + ni], int(m["subpath_kind"]), ext["uv"][v0:v0 + nv]))
    seq.sort(key=lambda t: (t[0], t[1]))
    meshes = np.zeros(len(seq), dtype=capi.mesh_dtype)
    v = i = 0
    for k, t in enumerate(seq):
        meshes[k] = (v, i, t[2].shape[0], t[4].shape[0], t[0], t[5])
        v += t[2].shape[0]
        i += t[4].shape[0]
    pos = np.concatenate([t[2] for t in seq]) if seq else np.zeros((0, 2), f32)
    col = np.concatenate([t[3] for t in seq]) if seq else np.zeros(0, np.uint32)
    idx = np.concatenate([t[4] for t in seq]) if seq else np.zeros(0, np.uint16)
    white, nb = refd["white_uv"]
    uv = np.zeros((pos.shape[0], 2), ext["uv"].dtype)
    uv[:] = np.frombuffer(white.tobytes()[:nb], dtype=ext["uv"].dtype)
    for k, t in enumerate(seq):
        if t[6] is not None:
            uv[int(meshes["first_vertex"][k]):int(meshes["first_vertex"][k]) + t[6].shape[0]] = t[6]
    st, cmds, idx2 = oracle.assemble(meshes, idx, max_vb, mesh_keys=draws["state_key"][meshes["draw"]])
    assert st == 0
    return pos, col, idx2, meshes, cmds, uv


# ---- frames -----------------------------------------------------------------------------------------------------------
def _grid(nx, ny, x0, y0, step, rng):
    import trilist_frame as TF
    return TF.grid(nx, ny, x0, y0, step, rng)


def s_text(uv_float=False, image=3, seed=5):
    """Labels around fills, strokes and user meshes: text first and last, a label that joins its neighbour fill's draw command, one
    that a scissor change keeps apart, rotated / non-uniformly scaled / saved states, a TextBox of several rows (several runs, one
    draw), the early-outs (too small, transparent), a blank string, text while a path is being built."""
    import trilist_frame as TF
    rng = np.random.default_rng(seed)
    s = TextScript()
    s.text(b"First thing in the frame", 20, 30, 20.0, 0xFFE0E0E0)
    s.begin_path().rect(10, 40, 200, 60).fill(0xFF2040F0, FILL_AA)
    s.text(b"joins the fill", 20, 80, 16.0, 0xFFFFFFFF)                       # same draw command as the rect
    s.begin_path().rounded_rect(10, 120, 200, 60, 6.0).fill(0xFF20F040, FILL_AA)
    s.set_scissor(0, 0, 640, 480)
    s.text(b"kept apart by a scissor", 20, 160, 16.0, 0xFF00FFFF, ALIGN_CENTER | ALIGN_MIDDLE)
    s.reset_scissor()
    s.begin_path().circle(400, 200, 40).stroke(0xFF00FF00, 3.0, cu.stroke_flags(0, 0))
    s.push().translate(300, 300).rotate(0.35).scale(1.7, 0.8)
    s.text(b"rotated, stretched", 0, 0, 14.0, 0x80FF8040, ALIGN_RIGHT | ALIGN_TOP)
    gp, gi, gc = TF.grid(5, 3, 0, 0, 12.0, rng)
    s.indexed_tri_list(gp, gc, gi, uv=TF.uv_of(gp, uv_float, rng), image=image)
    s.text_box(b"A text box that is broken into several rows by the caller's shaper, one run per row, one draw.", 10, 40, 180.0, 15.0, 0xFFFFFFFF,
               ALIGN_CENTER | ALIGN_BASELINE)
    s.global_alpha(0.5)
    s.text(b"half", 5, 5, 30.0, 0xFF102030, ALIGN_LEFT | ALIGN_BOTTOM)
    s.global_alpha(0.0)
    s.text(b"invisible", 5, 50, 30.0, 0xFFFFFFFF)                             # colour alpha 0 after the global alpha
    s.pop()
    s.text(b"too small", 500, 20, 3.0, 0xFFFFFFFF)                            # font_size * scale < 4
    s.text(b"    ", 500, 40, 20.0, 0xFFFFFFFF)                                # nothing to bake
    p, i = TF.quad(600, 20, 50, 40)
    s.indexed_tri_list(p, [0xFFFFFFFF], i)                                    # a user mesh on the font atlas next to text
    s.text(b"after a user mesh", 600, 80, 12.0, 0xFFFF00FF)
    s.begin_path().move_to(700, 50).line_to(800, 60)
    s.text(b"while a path is built", 700, 200, 18.0, 0xFF8080FF, ALIGN_RIGHT | ALIGN_BASELINE)
    s.line_to(780, 150).close_path().fill(0xFF808080, FILL_AA)
    s.begin_path().move_to(900, 100).line_to(1000, 100).line_to(920, 180).line_to(960, 60).line_to(1000, 180).close_path().fill(0xFF00FFFF, FILL_CONCAVE_AA)
    s.text_box(b"right aligned rows of a second box, long enough for a small vertex buffer to split inside it " * 2, 900, 300, 240.0, 13.0, 0xFFC0C0C0,
               ALIGN_RIGHT | ALIGN_TOP)
    s.text(b"Last thing in the frame", 20, 700, 20.0, 0xFFE0E0E0)
    return s


def s_text_only():
    """Nothing but text: no path in the whole list."""
    s = TextScript()
    for k in range(6):
        s.translate(3.0, 2.0).scale(1.07, 1.02)
        s.text(b"label %d of a frame of labels" % k, 20.0, 40.0 + 30.0 * k, 12.0 + 2 * k, 0xFF000000 | (0x203040 * (k + 1)), [65, 66, 68, 9, 18, 36][k])
    s.text_box(b"and a box of rows " * 8, 400, 100, 200.0, 14.0, 0xFFFFFFFF, ALIGN_LEFT | ALIGN_TOP)
    return s


def s_random(seed, uv_float=False):
    import trilist_frame as TF
    rng = np.random.default_rng(seed)
    s = TextScript()
    words = [b"alpha", b"beta gamma", b"The quick brown fox", b"jumps over", b"0123456789", b"lazy dog!", b"x", b"vg-renderer text"]
    depth = 0
    for k in range(int(rng.integers(10, 26))):
        r = rng.random()
        col = int(rng.integers(0, 2 ** 32)) | (0xFF000000 if rng.random() < 0.7 else 0x40000000)
        if r < 0.30:
            w = b" ".join(words[int(j)] for j in rng.integers(0, len(words), int(rng.integers(1, 4))))
            s.text(w, float(rng.uniform(0, 900)), float(rng.uniform(20, 600)), float(rng.uniform(8, 40)), col,
                   int(rng.choice([1, 2, 4])) | int(rng.choice([8, 16, 32, 64])))
        elif r < 0.40:
            w = b" ".join(words[int(j)] for j in rng.integers(0, len(words), int(rng.integers(4, 14))))
            s.text_box(w, float(rng.uniform(0, 700)), float(rng.uniform(20, 400)), float(rng.uniform(80, 300)), float(rng.uniform(9, 24)), col,
                       int(rng.choice([1, 2, 4])) | int(rng.choice([8, 16, 32, 64])))
        elif r < 0.50:
            nx, ny = int(rng.integers(1, 8)), int(rng.integers(1, 8))
            gp, gi, gc = TF.grid(nx, ny, float(rng.uniform(0, 800)), float(rng.uniform(0, 500)), float(rng.uniform(2, 20)), rng)
            s.indexed_tri_list(gp, gc[:1] if rng.random() < 0.4 else gc, gi, uv=TF.uv_of(gp, uv_float, rng) if rng.random() < 0.5 else None,
                               image=int(rng.choice([0xFFFF, 0xFFFF, 1, 2, 3])))
        elif r < 0.53:
            cx, cy, rad = float(rng.uniform(100, 800)), float(rng.uniform(100, 500)), float(rng.uniform(20, 80))
            s.begin_path().move_to(cx - rad, cy - rad * 0.4).line_to(cx + rad, cy - rad * 0.4).line_to(cx - rad * 0.6, cy + rad).line_to(cx, cy - rad)
            s.line_to(cx + rad * 0.6, cy + rad).close_path().fill(col | 0xFF000000, FILL_CONCAVE_AA)
        elif r < 0.66:
            s.begin_path().rounded_rect(float(rng.uniform(0, 800)), float(rng.uniform(0, 500)), float(rng.uniform(5, 90)), float(rng.uniform(5, 90)), 4.0)
            s.fill(col | 0xFF000000, FILL_AA)
        elif r < 0.76:
            s.begin_path().circle(float(rng.uniform(0, 800)), float(rng.uniform(0, 500)), float(rng.uniform(3, 60)))
            s.stroke(col | 0xFF000000, float(rng.uniform(0.5, 6)), cu.stroke_flags(int(rng.integers(0, 3)), int(rng.integers(0, 3))))
        elif r < 0.84:
            s.translate(float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))).rotate(float(rng.uniform(-0.3, 0.3))).scale(float(rng.uniform(0.7, 1.5)), float(rng.uniform(0.7, 1.5)))
        elif r < 0.89:
            s.push()
            depth += 1
        elif r < 0.94 and depth:
            s.pop()
            depth -= 1
        elif r < 0.97:
            s.global_alpha(float(rng.choice([1.0, 0.5, 0.25])))
        else:
            s.set_scissor(float(rng.uniform(0, 100)), float(rng.uniform(0, 100)), float(rng.uniform(300, 900)), float(rng.uniform(300, 600)))
    for _ in range(depth):
        s.pop()
    return s
