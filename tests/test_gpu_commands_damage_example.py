"""examples/vgx_commands_damage_example.cpp: a grid of cached drawings submitted under an armed assembly, turned into a command table,
boxed by vgx_command_bounds and rendered; one drawing picked with vgx_pick_commands_boxed, dragged with vgx_cache_update between two
vgx_damage_instances, the touched commands' boxes refreshed and the marked tiles redrawn by vgx_raster_commands_damaged, from C++. The
example itself compares its image with a full redraw and returns 0 only when no pixel differs; the test checks what it printed and the PPM."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_commands_damage_example_runs(tmp_path):
    exe, ppm = str(tmp_path / "vgx_commands_damage_example"), str(tmp_path / "out.ppm")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_commands_damage_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm], text=True, timeout=300)
    ncmd = int(re.search(r"in (\d+) draw commands", out).group(1))
    assert ncmd >= 4, out   # several vertex buffers: the drawing's commands are a few of many
    assert re.search(r"-> drawing 8\n", out), out
    m = re.search(r"damage: commands \[(\d+), (\d+)\) of (\d+) refreshed; (\d+) of (\d+) tiles marked; (\d+) pixels differ", out)
    a, b, n, marked, tiles, differ = (int(v) for v in m.groups())
    assert n == ncmd and 0 <= a < b <= n and b - a < n and tiles == 32 * 26 and 1 <= marked < tiles // 8 and differ == 0, out
    head = b"P6\n512 416\n255\n"
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head and len(pic) == len(head) + 512 * 416 * 3
    assert len(set(pic[len(head):len(head) + 512 * 3 * 100:3])) > 8   # not a flat picture
