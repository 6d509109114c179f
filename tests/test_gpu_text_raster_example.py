"""examples/vgx_text_raster_example.cpp: command-list bytes with a shape, a Text command and an IndexedTriList, from C++ to a PPM --
vgx_cmdlist_decode_text, a stand-in shaper over an atlas made up on the spot, vgx_text_quads, vgx_merge_uv_stream,
vgx_raster_textured. The example prints a digest of the pixels and, asked to, dumps its streams, draws and images; the numpy model of
the specification (tests/raster_textured_model.py) renders those and must arrive at the same digest and the same picture, in which the
shape, the glyphs and the user mesh all show."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_model as R
import raster_textured_model as T
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = R.capi


def test_cpp_text_raster_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_text_raster_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_text_raster_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, nd, aw, _ = np.frombuffer(raw, dtype="<u8", count=8).tolist()
    at = [64]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a

    pos, color, uv = take("<f4", 2 * nv).reshape(-1, 2), take("<u4", nv), take("<i2", 2 * nv).reshape(-1, 2)
    idx, meshes = take("<u2", ni), take(capi.mesh_dtype, nm)
    draws, dstate = take(capi.draw_dtype, nd), take(capi.draw_state_dtype, nd)
    atlas, checker = take("<u4", aw * aw).reshape(aw, aw), take("<u4", 64).reshape(8, 8)
    assert at[0] == len(raw) and (w, h, aw) == (256, 128, 128) and nd == 3
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFFFFFFF)
    f = R.make("example", pos, color, idx, meshes, tgt)
    f.draws, f.dstate, f.uv = draws.copy(), dstate.copy(), np.ascontiguousarray(uv)
    f.images = [T.Image(atlas, aw, 0), T.Image(checker, 8, T.NEAREST)]
    kinds = (meshes["subpath_kind"] >> 28).tolist()
    assert kinds.count(R.TEXT) == 1 and kinds.count(R.TRILIST) == 1 and kinds.index(R.TEXT) < kinds.index(R.TRILIST) and nm >= 3
    st = T.Stats(tgt)
    want = T.render(f, tgt, np.zeros((h, w), dtype=np.uint32), stats=st)
    for m in range(nm):  # the shape, the glyphs and the user mesh all show
        assert m in st.per_mesh and int((st.per_mesh[m] > 0).sum()) > 200, m
    text = kinds.index(R.TEXT)
    others = [m for m in range(nm) if m != text]
    glyph_px = want != T.render(f, tgt, np.zeros((h, w), dtype=np.uint32), only=others)
    cols, rows = np.nonzero(glyph_px.any(axis=0))[0], np.nonzero(glyph_px.any(axis=1))[0]
    assert cols[-1] - cols[0] > 150 and int(glyph_px.sum()) > 300
    assert glyph_px[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].mean() < 0.95  # patterns with gaps between them, not one filled box
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
