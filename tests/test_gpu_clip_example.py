"""examples/vgx_clip_example.cpp: a command list with a scissor change, an In region and an Out region, recorded, decoded, tessellated
and drawn by vgx_raster_frame from C++, written as a binary PPM. The example prints a digest of the pixels and, asked to, dumps its mesh
streams and draw state; the numpy model of the specification (tests/raster_frame_model.py) renders those and must arrive at the same
digest and the same picture -- which is not the picture without the state."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_frame_model as M
import raster_model as R
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_clip_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_clip_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_clip_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, nd = np.frombuffer(raw, dtype="<u8", count=6).tolist()
    at = 48
    parts = []
    for dtype, count in (("<f4", 2 * nv), ("<u4", nv), ("<u2", ni), (R.capi.mesh_dtype, nm), (R.capi.draw_dtype, nd), (R.capi.draw_state_dtype, nd)):
        parts.append(np.frombuffer(raw, dtype=dtype, count=count, offset=at))
        at += parts[-1].nbytes
    assert at == len(raw) and (w, h) == (256, 192) and nm > 20
    pos, color, idx, meshes, draws, dstate = parts
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFFFFFFF)
    f = R.make("example", pos.reshape(-1, 2), color, idx, meshes, tgt)
    f.draws, f.dstate = draws, dstate
    types = (draws["state_key"] >> 16) & 0xF
    tested = (dstate["clip_first_draw"] != M.NONE) & (dstate["clip_num_draws"] != 0) & (types != M.CLIP)
    assert int((types == M.CLIP).sum()) == 3 and {0, 1} <= {int(r) for r in dstate["clip_rule"][tested]}
    assert len({tuple(int(v) for v in s) for s in dstate["scissor"]}) >= 4
    want = M.render(f, tgt, np.zeros((h, w), dtype=np.uint32))
    plain = M.render(f, tgt, np.zeros((h, w), dtype=np.uint32), ignore_clips=True)
    assert int((want != plain).sum()) > 1000
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
