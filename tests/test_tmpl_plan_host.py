"""CPU: template mode's host decisions (vg-renderer_amd/csrc/vgx_tmpl_plan.h -- kernel kind and tile size, class grouping, per-class
sizes, the batch plan and its tables) as a stand-alone host program: tests/native/tmpl_plan_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tmpl_plan_kernel_classes_sizes_and_tables(tmp_path):
    exe = str(tmp_path / "tmpl_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "vg-renderer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "tmpl_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
