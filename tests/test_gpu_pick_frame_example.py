"""examples/vgx_pick_frame_example.cpp: command-list bytes with a square under a scissor, a bar under an In region, a bar under an Out
region and a concave star, from C++ to hit records -- vgx_cmdlist_decode, the tessellator, vgx_flatten, vgx_concave_contours, vgx_merge,
vgx_raster_concave (the ID image) and vgx_pick / vgx_pick_frame. The example compares vgx_pick_frame with its own ID image at every pixel
centre and exits non-zero on a disagreement; asked to, it dumps its streams, draws and the ID image, and the numpy model of the
specification (tests/pick_frame_model.py) must say the same at every pixel centre."""
import os
import re
import subprocess

import numpy as np
import pytest

import pick_frame_model as PF
import raster_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = R.capi


def test_cpp_pick_frame_example_runs(tmp_path):
    exe, dump = str(tmp_path / "vgx_pick_frame_example"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_pick_frame_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, dump], text=True, timeout=300)  # exit status 0: no pixel centre disagrees with the ID image
    assert re.search(r"6144 pixel centres checked against the ID image: 0 disagree", out), out
    differ = int(re.search(r"(\d+) of 10 named points differ", out).group(1))
    assert differ >= 4, out
    lines = [l for l in out.splitlines() if l.startswith("point")]
    assert len(lines) == 10
    star = [l for l in lines if "middle of the star" in l][0]
    assert re.search(r"vgx_pick: draw +0 mesh +0 +vgx_pick_frame: draw +6", star), star   # vgx_pick never hits a contour mesh
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, nd, _, _ = np.frombuffer(raw, dtype="<u8", count=8).tolist()
    at = [64]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a

    pos, color = take("<f4", 2 * nv).reshape(-1, 2), take("<u4", nv)
    idx, meshes = take("<u2", ni), take(capi.mesh_dtype, nm)
    draws, dstate = take(capi.draw_dtype, nd), take(capi.draw_state_dtype, nd)
    ids = take("<u4", w * h).reshape(h, w)
    assert at[0] == len(raw) and (w, h) == (96, 64) and nd == 7
    assert int(((meshes["subpath_kind"] >> 28) == capi.MESH_CONTOURS).sum()) == 1
    tgt = R.Target(w, h, w, 0, 0)
    f = R.make("example", pos, color, idx, meshes, tgt)
    f.draws, f.dstate = draws.copy(), dstate.copy()
    a = PF.pick(f, PF.centre_queries(tgt))
    mesh = np.where(a.hits["mesh"] == PF.NONE, -1, a.hits["mesh"].astype(np.int64)).reshape(h, w)
    assert np.array_equal(mesh, PF.decode_ids(ids, tgt))
    assert a.passed_in.any() and a.refused_in.any() and a.passed_out.any() and a.cut.any() and a.contour.any()
