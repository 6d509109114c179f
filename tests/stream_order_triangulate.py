"""The row of vgx_concave_triangulate in the table of tests/stream_order.py, and its maker. The table's file is shared by every entry and
is left as it is: this module appends the row to stream_order.CASES when it is imported, once. The test files of
vgx_concave_triangulate import it, and pytest imports every test file before it runs a test, so the table is complete when
tests/test_stream_order_table_cpu.py reads it and when tests/test_gpu_stream_order.py (collected after them) takes its parameters."""
import ctypes as C

import numpy as np

import stream_order as SO

F = np.float32
ENTRY = "vgx_concave_triangulate"


def make_concave_triangulate(env, ctx):
    import concave_triangulate_model as TM
    import raster_harness as H
    move = np.array([8.0, -5.0], dtype=F)   # every coordinate below is a multiple of 0.25: the moved rings are the same rings, exactly
    rings = [TM.L_SHAPE, TM.COMB, TM.BOWTIE, TM.DART, TM.FLAT3, TM.COLLINEAR]
    assert all(np.array_equal((r + move) - move, r) and TM.ring_route(r)[0] == TM.ring_route(r + move)[0] for r in rings)
    specs = [([r], TM.CONCAVE, TM.COLOR, 1.0) for r in rings]
    specs.insert(2, ([TM.SQUARE, TM.SQUARE[::-1] * F(0.5) + F(10.0)], TM.CONCAVE | TM.AA, 0x80FF8040, 1.5))   # MULTI whatever its geometry
    specs.insert(4, ([TM.SQUARE], TM.ENABLE | TM.AA, 0xFF112233, 1.0))                                         # makes nothing
    fl = H.Flat(specs)
    nv = sum(sum(len(c) for c in s[0]) * (3 if s[1] & TM.AA else 1) for s in specs if TM.makes(s))
    ni = sum(sum(len(c) for c in s[0]) * 8 for s in specs if TM.makes(s))   # a bound: 3 (V - 2) < 8 V
    p = SO.Plan()
    poly = p.new_inp(fl.poly, (fl.poly + move).astype(F))
    draws = p.new_inp(fl.draws, SO._recoloured(fl.draws))
    subs, info = SO.to_dev(fl.subs), SO.to_dev(fl.info)
    p.keep += [subs, info]
    b = SO.mesh_out(p, env, nv, ni, len(specs) + 1)
    routes = p.out(env.torch.zeros(len(specs) + 16, dtype=env.torch.int32, device="cuda:0"), used=len(specs) * 4)
    out = b.out_struct()

    def call():
        env.rt._check(env.lib.vgx_concave_triangulate(ctx.handle, poly.data_ptr(), subs.data_ptr(), info.data_ptr(), draws.data_ptr(), len(fl.specs), C.byref(out),
                                                      routes.data_ptr(), b.dev_sizes.data_ptr(), b.dev_status.data_ptr(), env.rt._stream_ptr()), "vgx_concave_triangulate")
    p.call = call
    return p


if not any(r.entry == ENTRY for r in SO.CASES):
    SO.CASES.append(SO.Row(ENTRY, make_concave_triangulate, header="stream-ordered with no host round trip"))
