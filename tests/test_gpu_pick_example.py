"""examples/vgx_pick_example.cpp: hit testing from C++ -- one frame of overlapping cached drawings submitted, a handful of cursor
positions picked, the drawing under each hit found through mesh_end, every answer checked against a host loop over the downloaded frame."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_pick_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_pick_example")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_pick_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=300)
    assert "8 cursors picked" in out and "0 answers differ from the host loop" in out and "under it instance" in out, out
