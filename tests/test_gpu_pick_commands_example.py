"""examples/vgx_pick_commands_example.cpp: a backdrop and four discs that overlap under the cursor, decoded, tessellated under an armed
draw-command assembly into ONE draw command, turned into a command table by vgx_raster_cmds_from_assembly and hit-tested by
vgx_pick_commands with the frame's mesh table as owners, from C++. The example prints the hit under the cursor and two steps down the
stack (cmd_end / tri_end) and, asked to, dumps its streams and tables; the numpy model (tests/pick_commands_model.py) must give the same
hits for the same limits, and the walk must name the draws 4, 3, 2."""
import os
import re
import subprocess

import numpy as np
import pytest

import pick_commands_model as PC
import raster_commands_model as CM
import raster_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = R.capi


def test_cpp_pick_commands_example_runs(tmp_path):
    exe, dump = str(tmp_path / "vgx_pick_commands_example"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_pick_commands_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, dump], text=True, timeout=300)  # exit status 0: the walk named the draws 4, 3, 2
    lines = re.findall(r"^(cursor|below ) \(([\d.]+), ([\d.]+)\) limit \((-?\d+), (\d+)\): command (\d+) triangle (\d+) mesh (\d+) draw (\d+)$", out, flags=re.M)
    assert len(lines) == 3 and [l[0] for l in lines] == ["cursor", "below ", "below "], out
    assert [int(l[8]) for l in lines] == [4, 3, 2], out
    assert re.search(r"5 draws -> 5 meshes in 1 draw command,", out), out
    raw = open(dump, "rb").read()
    nv, ni, nc, nm, w, h = np.frombuffer(raw, dtype="<u8", count=6).tolist()
    at = 48
    parts = []
    for dtype, count in (("<f4", 2 * nv), ("<u4", nv), ("<u2", ni), (capi.raster_cmd_dtype, nc), (capi.mesh_dtype, nm)):
        parts.append(np.frombuffer(raw, dtype=dtype, count=count, offset=at))
        at += parts[-1].nbytes
    assert at == len(raw) and (w, h) == (256, 192) and nc == 1 and nm == 5
    pos, color, idx, cmds, meshes = parts
    sc = CM.Scene("example", pos.reshape(-1, 2), color, idx, cmds, R.Target(w, h, w, 0, 0))
    q = PC.queries([(float(l[1]), float(l[2])) for l in lines])
    q["cmd_end"] = [int(l[3]) & 0xFFFFFFFF for l in lines]
    q["tri_end"] = [int(l[4]) for l in lines]
    want = PC.pick(sc, q, meshes)
    assert want.status == capi.VGX_OK
    got = np.array([tuple(int(v) for v in l[5:9]) for l in lines], dtype=capi.pick_cmd_hit_dtype)
    assert np.array_equal(got.view(np.uint32), want.hits.view(np.uint32)), (got, want.hits)
    # every step's limit is the first triangle of the mesh hit before
    for k in (1, 2):
        m = int(lines[k - 1][7])
        assert int(lines[k][3]) == int(lines[k - 1][5]) and int(lines[k][4]) == (int(meshes["first_index"][m]) - int(cmds["first_index"][0])) // 3
