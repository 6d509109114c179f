"""CPU: the sort window of the damaged raster calls (vg-renderer_amd/csrc/vgx_damage.h -- what a landed mirror teaches, and the window
vgx_raster_damaged and vgx_raster_commands_damaged sort) as a stand-alone host program: tests/native/damage_window_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vg-renderer_amd", "csrc")
TEST = os.path.join(ROOT, "tests", "native", "damage_window_test.cpp")


def test_damage_window_sequences_and_clips(tmp_path):
    exe = str(tmp_path / "damage_window_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, TEST, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
