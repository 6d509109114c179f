"""CPU: examples/vgx_marquee_example.cpp compiles and links against the C-ABI here, without a GPU: it needs vgx_pick_rect and its types in
include/vgx.h and the symbol in libvgx.so (tests/test_gpu_marquee_example.py runs it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marquee_example_compiles_and_links(tmp_path):
    pkg = os.path.join(ROOT, "vg-renderer_amd")
    if not os.path.exists(os.path.join(pkg, "libvgx.so")):
        import __graft_entry__ as g
        g.build()
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "vgx_marquee_example.cpp"),
                           "-L", pkg, "-lvgx", "-Wl,-rpath," + pkg, "-o", str(tmp_path / "vgx_marquee_example")])
