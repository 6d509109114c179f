"""examples/vgx_commands_example.cpp: a command list with a scissor change and an In clip region, decoded, tessellated under an armed
draw-command assembly (VGX_ASM_SPLIT_STATE, vertex buffers of 512), turned into a command table by vgx_raster_cmds_from_assembly and drawn
by vgx_raster_commands from C++, written as a binary PPM. The example prints a digest of the pixels and, asked to, dumps its streams and
its table; the numpy model (tests/raster_commands_model.py) renders those and must arrive at the same digest and the same picture."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_commands_model as CM
import raster_model as R
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_commands_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_commands_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_commands_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nv, ni, nc, w, h = np.frombuffer(raw, dtype="<u8", count=5).tolist()
    at = 40
    parts = []
    for dtype, count in (("<f4", 2 * nv), ("<u4", nv), ("<i2", 2 * nv), ("<u2", ni), (R.capi.raster_cmd_dtype, nc)):
        parts.append(np.frombuffer(raw, dtype=dtype, count=count, offset=at))
        at += parts[-1].nbytes
    assert at == len(raw) and (w, h) == (256, 192)
    pos, color, uv, idx, cmds = parts
    tested = (cmds["type"] != CM.CLIP) & (cmds["clip_first_cmd"] != CM.NONE) & (cmds["clip_num_cmds"] != 0)
    assert int((cmds["type"] == CM.CLIP).sum()) >= 1 and tested.any() and nv > 512 and nc > 4
    assert len({tuple(int(v) for v in s) for s in cmds["scissor"]}) >= 2
    assert (cmds["first_vertex"][1:] > 0).all() and (cmds["num_vertices"] <= 512).all()  # command-relative indices, small vertex buffers
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFFFFFFF)
    sc = CM.Scene("example", pos.reshape(-1, 2), color, idx, cmds, tgt, uv=uv.reshape(-1, 2), images=[CM.white_image()])
    assert CM.status(sc) == R.capi.VGX_OK
    want = CM.render(sc, tgt, np.zeros((h, w), dtype=np.uint32))
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
