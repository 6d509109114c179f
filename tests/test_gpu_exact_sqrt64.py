"""The binary64 square root the gradient rule of vgx_raster_painted calls (vgx_raster_sqrt, csrc/vgx_raster.h) on the device against
the same function on the host, bit for bit, over about 2^26 inputs: sums of two squares as the rule forms them, every binade, perfect
squares and their neighbours. tests/native/exact_sqrt64_test.hip is the program; __graft_entry__.build() compiles it."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_sqrt64_equals_the_hosts():
    exe = os.path.join(ROOT, "tests", "native", "exact_sqrt64_test.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", exe,
                               os.path.join(ROOT, "tests", "native", "exact_sqrt64_test.hip")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [l for l in r.stdout.splitlines() if "mismatches=" in l]
    assert r.returncode == 0 and len(lines) == 5, r.stdout
    for l in lines:
        assert "mismatches=0 of " in l, r.stdout
    total = int(lines[-1].split(" of ")[1])
    assert lines[-1].startswith("mismatches=") and total > 60_000_000, lines[-1]
