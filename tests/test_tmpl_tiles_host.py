"""CPU: template mode's tile boundaries (vg-renderer_amd/csrc/vgx_tmpl_plan.h -- snap limit, stride, nominal boundary, snap decision:
the lines the build kernels run) on random lists of mesh lengths, as a stand-alone host program: tests/native/tmpl_tiles_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tmpl_tile_boundaries_partition_and_avoid_short_meshes(tmp_path):
    exe = str(tmp_path / "tmpl_tiles_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "vg-renderer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "tmpl_tiles_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
