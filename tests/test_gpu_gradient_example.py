"""examples/vgx_gradient_example.cpp: command-list bytes with a linear, a box and a radial gradient and an image pattern, from C++ to a
PPM -- vgx_cmdlist_decode, vgx_paint_tables, the tessellator, vgx_raster_painted. The example prints a digest of the pixels and, asked
to, dumps its streams, draws, paints and image; the numpy model of the specification (tests/raster_painted_model.py) renders those and
must arrive at the same digest and the same picture, in which every one of the four paints shows as a paint, not as a flat colour."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_model as R
import raster_painted_model as P
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = R.capi


def test_cpp_gradient_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_gradient_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_gradient_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, nd, npaints, side = np.frombuffer(raw, dtype="<u8", count=8).tolist()
    at = [64]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a

    pos, color = take("<f4", 2 * nv).reshape(-1, 2), take("<u4", nv)
    idx, meshes = take("<u2", ni), take(capi.mesh_dtype, nm)
    draws, dstate = take(capi.draw_dtype, nd), take(capi.draw_state_dtype, nd)
    paints, tile = take(capi.paint_dtype, npaints), take("<u4", side * side).reshape(side, side)
    assert at[0] == len(raw) and (w, h, side) == (256, 128, 8) and nd == 4 and npaints == 4
    assert paints["type"].tolist() == [1, 1, 1, 2] and ((draws["state_key"] >> 16) & 0xF).tolist() == [1, 1, 1, 2]
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFE8E0D8)
    f = R.make("example", pos, color, idx, meshes, tgt)
    f.draws, f.dstate, f.uv = draws.copy(), dstate.copy(), np.zeros((nv, 2), dtype=np.int16)
    f.images = [P.Image(tile, side, 0)]
    f.gradients, f.patterns = P.scatter(paints)
    st = P.Stats(tgt)
    want = P.render(f, tgt, np.zeros((h, w), dtype=np.uint32), stats=st)
    for d in range(nd):  # every paint shows, and as a paint: many colours, where its vertex colours would give one
        ms = [m for m in range(nm) if int(meshes["draw"][m]) == d]
        hit = sum(st.per_mesh[m] for m in ms if m in st.per_mesh) > 0
        assert int(hit.sum()) > 400, d
        others = [m for m in range(nm) if m not in ms]
        mine = want != P.render(f, tgt, np.zeros((h, w), dtype=np.uint32), only=others)
        assert np.unique(want[mine]).size > 12, d
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
