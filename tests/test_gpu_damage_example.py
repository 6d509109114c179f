"""examples/vgx_damage_example.cpp: the damage redraw from C++ -- a grid of cached drawings rendered, one drawing dragged and another
recoloured through mark -> vgx_cache_update -> mark -> vgx_raster_damaged on one stream; the example itself compares the image with a full
vgx_raster_concave of the edited frame and exits non-zero unless they are equal."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_damage_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_damage_example")
    ppm = str(tmp_path / "damage.ppm")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_damage_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm], text=True, timeout=300)
    m = re.search(r"damage: (\d+) of (\d+) tiles marked; 0 pixels differ from a full redraw", out)
    assert m and 0 < int(m.group(1)) < int(m.group(2)) // 4, out   # two drawings of thirty: a small part of the image
    with open(ppm, "rb") as f:
        assert f.read(15) == b"P6\n512 416\n255\n"
    assert os.path.getsize(ppm) == 15 + 512 * 416 * 3
