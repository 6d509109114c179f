"""examples/vgx_concave_nested_example.cpp: command-list bytes with the word "oBioBio" as one path of sixteen outlines and a target of five
nested squares, from C++ to a PPM -- vgx_cmdlist_decode, the tessellator, vgx_flatten, vgx_concave_triangulate_nested, vgx_pick, vgx_merge
under an armed assembly, vgx_raster_cmds_from_assembly, vgx_raster_commands; no libtess2. The example prints the routes and the picks; its
picture is, pixel for pixel, the one runtime.concave_triangulate_nested gives for the same list."""
import os
import re
import subprocess

import numpy as np
import pytest

import cmdlist_util as cu
import raster_painted_model as P
import test_gpu_concave_nested as GN
from raster_harness import rt  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rect(x, y, w, h, hole=False):
    p = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
    return p[::-1] if hole else p


def list_bytes():
    """The example's list, written with the tests' recorder."""
    r = P.Rec()

    def path(rings):
        r.begin_path()
        for pts in rings:
            r.move_to(*pts[0])
            for p in pts[1:]:
                r.line_to(*p)
            r.close_path()

    r.begin_path(); r.rect(0, 0, 160, 64); r.fill_path(0xFF302820, cu.fill_flags(aa=False))
    word = []
    for k, ch in enumerate("oBioBio"):
        x = 2.0 + 13.0 * k
        if ch == "o":
            word += [rect(x, 10, 10, 10), rect(x + 2.5, 12.5, 5, 5, True)]
        elif ch == "B":
            word += [rect(x, 10, 10, 14), rect(x + 2, 12, 3.5, 3.5, True), rect(x + 2, 18, 3.5, 3.5, True)]
        else:
            word += [rect(x + 3, 15, 4, 10), rect(x + 3, 9, 4, 4)]
    path(word); r.fill_path(0xC020C0FF, cu.fill_flags(concave=True, aa=False))
    path([rect(100 + 4 * k, 4 + 4 * k, 56 - 8 * k, 56 - 8 * k, bool(k & 1)) for k in range(5)]); r.fill_path(0xC0FF8020, cu.fill_flags(concave=True, aa=True))
    return r.bytes()


def test_cpp_concave_nested_example_runs(rt, tmp_path):
    exe, ppm = str(tmp_path / "vgx_concave_nested_example"), str(tmp_path / "out.ppm")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_concave_nested_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm], text=True, timeout=300)
    assert re.findall(r"draw (\d): (.*)", out) == [("0", "no mesh"), ("1", "triangles"), ("2", "triangles")], out
    assert "on the dot of the i: mesh 0 of draw 1" in out and "in the counter of the o: nothing" in out and "on the innermost square: mesh 1 of draw 2" in out, out
    # the backdrop (4 vertices, 6 indices); the word: V = 64, S = 16, G = 9; the target: V = 20, S = 5, G = 3 behind a fringe
    nv = 4 + 64 + 3 * 20
    ni = 6 + 3 * (64 + 32 - 36) + (6 * 20 + 3 * (20 + 10 - 12))
    assert re.search(r"assembled frame: 3 meshes, (\d+) vertices, (\d+) indices", out).groups() == (str(nv), str(ni)), out
    assert re.search(r"digest [0-9a-f]{16}", out)
    pic = open(ppm, "rb").read()
    head = b"P6\n160 64\n255\n"
    assert pic[:len(head)] == head
    rgb = np.frombuffer(pic[len(head):], dtype=np.uint8).reshape(64, 160, 3)
    backdrop = rgb[2, 2].tolist()
    assert backdrop == [0x20, 0x28, 0x30]
    assert rgb[11, 33].tolist() != backdrop and rgb[15, 7].tolist() == backdrop and rgb[15, 13].tolist() == backdrop   # the dot of the i, the counter of the o, the gap
    assert rgb[32, 128].tolist() != backdrop and rgb[32, 106].tolist() == backdrop and rgb[32, 102].tolist() != backdrop   # the target: innermost square, second ring, rim
    # the same list through the runtime call: the same routes, sizes and picture
    routes, image, sizes = GN.assembled_image(rt, list_bytes(), 160, 64, 0xFFE8E0D8)
    assert routes == [0, GN.TM.TRIANGLES, GN.TM.TRIANGLES] and sizes == (3, nv, ni)
    want = np.stack([image & 255, (image >> 8) & 255, (image >> 16) & 255], axis=-1).astype(np.uint8)
    assert np.array_equal(rgb, want), np.argwhere((rgb != want).any(axis=-1))[:5]
