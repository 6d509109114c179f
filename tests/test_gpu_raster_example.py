"""examples/vgx_raster_example.cpp: a frame rendered from C++ -- one tiger-like drawing tessellated, drawn into a 256 x 256 image by
vgx_raster, written as a binary PPM. The example prints a digest of the pixels and, asked to, dumps its mesh streams; the numpy model
of the specification (tests/raster_model.py) renders those streams and must arrive at the same digest and the same picture."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_model as R
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_raster_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_raster_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_raster_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, _ = np.frombuffer(raw, dtype="<u8", count=6).tolist()
    at = 48
    pos = np.frombuffer(raw, dtype="<f4", count=2 * nv, offset=at).reshape(-1, 2)
    at += 8 * nv
    color = np.frombuffer(raw, dtype="<u4", count=nv, offset=at)
    at += 4 * nv
    idx = np.frombuffer(raw, dtype="<u2", count=ni, offset=at)
    at += 2 * ni
    meshes = np.frombuffer(raw, dtype=R.capi.mesh_dtype, count=nm, offset=at)
    assert at + 32 * nm == len(raw) and (w, h) == (256, 256) and nm > 60
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFFFFFFF)
    want = R.render(R.make("example", pos, color, idx, meshes, tgt), tgt, np.zeros((h, w), dtype=np.uint32))
    assert int((want != 0xFFFFFFFF).sum()) > 10000
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
