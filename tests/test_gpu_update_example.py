"""examples/vgx_update_example.cpp: the incremental update from C++ -- a frame of overlapping cached drawings submitted, the drawing under a
cursor picked, moved and recoloured through vgx_cache_update, picked again at the old and the new position; every answer checked against
a host loop over the downloaded frame, the frame and its boxes against a fresh submit."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_update_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_update_example")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_update_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=300)
    m = re.search(r"update: at the old cursor instance (\d+) answers, at the new one instance (\d+); 0 answers differ from the host loop, "
                  r"0 words differ from a fresh submit", out)
    assert m and m.group(1) != m.group(2), out
    assert re.search(r"cursor \(.*\): instance %s, under it instance %s" % (m.group(2), m.group(1)), out), out
