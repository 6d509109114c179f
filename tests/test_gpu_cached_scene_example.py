"""examples/vgx_cached_scene.cpp: a grid of cached drawings under a moving camera from C++ -- vgx_cache_cull then vgx_cache_submit per frame,
nothing read back in between; every frame submits exactly the kept instances' vertices and never the whole grid."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_cached_scene_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_cached_scene")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_cached_scene.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, "12"], text=True, timeout=300)
    assert "12 frames culled and submitted" in out and "of 576 instances kept" in out, out
