"""examples/vgx_dashed_frame_example.cpp: a frame of filled and dashed draws through vgx_tessellate_dashed from C++ -- the first frame
reaches VGX_OK within four calls, the steady one takes one, and every dash is one stroke mesh at its draw's place."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_dashed_frame_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_dashed_frame_example")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_dashed_frame_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=300)
    assert "frame 0: 96 draws (64 dashed)" in out and "frame 1: 96 draws (64 dashed)" in out and "INCONSISTENT" not in out, out
    assert "the steady frame took one call; every dash is one stroke mesh at its draw's place" in out, out
    assert "(OK)" in out  # the steady frame: one call
