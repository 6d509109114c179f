"""examples/vgx_concave_raster_example.cpp: command-list bytes with a star under both fill rules, a ring with a hole, an AA concave shape
under a linear gradient and a concave clip region, from C++ to a PPM -- vgx_cmdlist_decode, the tessellator, vgx_flatten,
vgx_concave_contours, vgx_merge, vgx_raster_concave; no libtess2. The example prints a digest of the pixels and, asked to, dumps its
streams, draws and paints; the numpy model of the specification (tests/raster_concave_model.py) renders those and must arrive at the
same digest and the same picture, in which every concave fill shows."""
import os
import re
import subprocess

import numpy as np
import pytest

import raster_concave_model as K
import raster_model as R
import raster_painted_model as P
from hashutil import fnv1a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = R.capi


def test_cpp_concave_raster_example_runs(tmp_path):
    exe, ppm, dump = str(tmp_path / "vgx_concave_raster_example"), str(tmp_path / "out.ppm"), str(tmp_path / "frame.bin")
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_concave_raster_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, ppm, dump], text=True, timeout=300)
    digest = int(re.search(r"digest ([0-9a-f]{16})", out).group(1), 16)
    raw = open(dump, "rb").read()
    nm, nv, ni, w, h, nd, npaints, _ = np.frombuffer(raw, dtype="<u8", count=8).tolist()
    at = [64]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a

    pos, color = take("<f4", 2 * nv).reshape(-1, 2), take("<u4", nv)
    idx, meshes = take("<u2", ni), take(capi.mesh_dtype, nm)
    draws, dstate = take(capi.draw_dtype, nd), take(capi.draw_state_dtype, nd)
    paints = take(capi.paint_dtype, npaints)
    assert at[0] == len(raw) and (w, h) == (192, 128) and nd == 7 and npaints == 1
    kinds = meshes["subpath_kind"] >> 28
    cm = np.flatnonzero(kinds == capi.MESH_CONTOURS)
    assert cm.size == 5 and int((kinds == capi.MESH_CONCAVE_FILL_AA).sum()) == 2                    # two of the five fills are anti-aliased
    assert sorted((meshes["subpath_kind"][cm] & capi.CONTOUR_EVEN_ODD).tolist()) == [0, 0, 0, 1, 1]   # both rules
    assert (np.diff(meshes["draw"].astype(np.int64)) >= 0).all()
    tgt = R.Target(w, h, w, 0, 0, clear=0xFFE8E0D8)
    f = R.make("example", pos, color, idx, meshes, tgt)
    f.draws, f.dstate, f.uv, f.images = draws.copy(), dstate.copy(), np.zeros((nv, 2), dtype=np.int16), []
    f.gradients, f.patterns = P.scatter(paints)
    st = P.Stats(tgt)
    want = K.render(f, tgt, np.zeros((h, w), dtype=np.uint32), stats=st)
    for m in cm:
        clip = ((int(draws["state_key"][int(meshes["draw"][m])]) >> 16) & 0xF) == P.CLIP
        assert clip or int(st.per_mesh[int(m)].sum()) > 300, m   # every concave fill shows
    assert st.stamped.sum() > 300                                 # ... and the concave clip region stamps
    bar = [m for m in range(nm) if int(meshes["draw"][m]) == nd - 1]
    hit = sum(st.per_mesh[m] for m in bar) > 0
    assert 0 < int(hit.sum()) < 84 * 24 and not (hit & ~st.stamped).any()   # the bar shows inside the region only
    pent = [int(m) for m in cm[:2]]
    assert int(st.per_mesh[pent[0]].sum()) > int(st.per_mesh[pent[1]].sum()) + 100   # EvenOdd leaves the pentagram's centre out
    assert digest == fnv1a(want), out
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pic = open(ppm, "rb").read()
    assert pic[:len(head)] == head
    rgb = np.stack([(want >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    assert pic[len(head):] == rgb.tobytes()
