"""CPU: the ordinary pipeline's host decisions (vg-renderer_amd/csrc/vgx_route_plan.h -- batch tag, period decoding, heap and one-walk
sizing, the route choice of the count and of the immediate call, the options table) as a stand-alone host program:
tests/native/route_plan_test.cpp."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vg-renderer_amd", "csrc")
TEST = os.path.join(ROOT, "tests", "native", "route_plan_test.cpp")


def _defines(path):
    return {m.group(1): m.group(2) for m in re.finditer(r"^#define (VGX_\w+) +(\w+)", open(path).read(), re.M)}


def test_route_plan_rules_choice_and_options(tmp_path):
    exe = str(tmp_path / "route_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, TEST, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_route_plan_test_uses_the_library_constants():
    """The program defines the constants the header takes from its includer; they are the library's."""
    mine = _defines(TEST)
    theirs = {}
    for h in ("vgx_internal.h", "vgx_inst.h", "vgx_tmpl_plan.h"):
        theirs.update(_defines(os.path.join(CSRC, h)))
    assert len(mine) == 7
    for k, v in mine.items():
        assert theirs[k] == v, k
