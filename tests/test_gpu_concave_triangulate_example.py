"""examples/vgx_concave_triangulate_example.cpp: command-list bytes with a star, an anti-aliased L and a bow-tie, from C++ to a PPM --
vgx_cmdlist_decode, the tessellator, vgx_flatten, vgx_concave_triangulate, vgx_merge under an armed assembly,
vgx_raster_cmds_from_assembly, vgx_raster_commands; no libtess2. The example prints the routes; the picture shows the two triangulated
fills and leaves the refused one to the contour route."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_concave_triangulate_example_runs(tmp_path):
    exe, ppm = str(tmp_path / "vgx_concave_triangulate_example"), str(tmp_path / "out.ppm")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_concave_triangulate_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm], text=True, timeout=300)
    assert re.findall(r"draw (\d): (.*)", out) == [("0", "no mesh"), ("1", "triangles"), ("2", "triangles"), ("3", "refused: not simple")], out
    # the backdrop's two triangles, the star's 8, the L's fringe (12) and interior (4)
    assert re.search(r"assembled frame: 3 meshes, (\d+) vertices, (\d+) indices", out).groups() == (str(4 + 10 + 18), str(6 + 24 + 36 + 12)), out
    assert re.search(r"digest [0-9a-f]{16}", out)
    pic = open(ppm, "rb").read()
    head = b"P6\n128 96\n255\n"
    assert pic[:len(head)] == head
    rgb = np.frombuffer(pic[len(head):], dtype=np.uint8).reshape(96, 128, 3)
    backdrop = rgb[2, 2].tolist()
    assert backdrop == [0x20, 0x28, 0x30]
    assert rgb[32, 34].tolist() != backdrop and rgb[40, 80].tolist() != backdrop and rgb[16, 110].tolist() != backdrop   # the star, both arms of the L
    assert rgb[40, 105].tolist() == backdrop and rgb[70, 20].tolist() == backdrop and rgb[84, 52].tolist() == backdrop     # the L's notch; the bow-tie is not drawn
