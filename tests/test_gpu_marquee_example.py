"""examples/vgx_marquee_example.cpp: pick tolerance and marquee selection from C++ -- a grid of cached drawings and a hairline submitted,
the hairline picked with a +-2-unit square where the point pick misses, one marquee as a crossing and as a window selection by instance,
the selected instances recoloured through vgx_cache_update, the image written as a PPM; every selection checked against a host loop."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_marquee_example_runs(tmp_path):
    exe = str(tmp_path / "vgx_marquee_example")
    ppm = str(tmp_path / "marquee.ppm")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_marquee_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm], text=True, timeout=300)
    assert "the point pick finds nothing, the +-2 square instance 64 (1 entry)" in out, out
    assert "12 instances crossed, 2 wholly inside" in out and "0 answers differ from the host loop" in out, out
    header = b"P6\n1125 1000\n255\n"
    assert open(ppm, "rb").read(len(header)) == header and os.path.getsize(ppm) == len(header) + 3 * 1125 * 1000
