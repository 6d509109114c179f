"""The row of vgx_concave_triangulate_nested in the table of tests/stream_order.py, and its maker: appended to stream_order.CASES when this
module is imported, once, the way tests/stream_order_rings.py does it. The test files of the entry import it."""
import ctypes as C

import numpy as np

import stream_order as SO

F = np.float32
ENTRY = "vgx_concave_triangulate_nested"


def make_concave_triangulate_nested(env, ctx):
    import concave_nested_model as NM
    import concave_rings_model as RM
    import concave_triangulate_model as TM
    import raster_harness as H
    move = np.array([8.0, -5.0], dtype=F)   # every coordinate below is a multiple of 0.25: the moved rings are the same rings, exactly
    names = ["island", "word_eo_aa", "bullseye", "island_touches_hole", "two_donuts_interleaved", "donut_same_nz", "word"]
    specs = [NM.draw_spec(n) for n in names] + [RM.draw_spec("comb")]   # one group: the rings rule
    for rings, flags, _, _ in specs:
        moved = [r + move for r in rings]
        assert all(np.array_equal(m - move, r) for m, r in zip(moved, rings))
        if not flags & RM.AA:
            assert NM.nested_route(rings, bool(flags & RM.EO))[0] == NM.nested_route(moved, bool(flags & RM.EO))[0]
    specs.insert(2, ([TM.L_SHAPE], TM.CONCAVE, TM.COLOR, 1.0))                 # one ring: the single-ring rule
    specs.insert(4, ([TM.SQUARE], TM.ENABLE | TM.AA, 0xFF112233, 1.0))         # makes nothing
    fl = H.Flat(specs)
    nv = sum(sum(len(c) for c in s[0]) * (3 if s[1] & TM.AA else 1) for s in specs if TM.makes(s))
    ni = sum(sum(len(c) for c in s[0]) * 11 for s in specs if TM.makes(s))   # a bound: 6 V + 3 (V + 2 H - 2) < 11 V, and 8 V for contours
    p = SO.Plan()
    poly = p.new_inp(fl.poly, (fl.poly + move).astype(F))
    draws = p.new_inp(fl.draws, SO._recoloured(fl.draws))
    subs, info = SO.to_dev(fl.subs), SO.to_dev(fl.info)
    p.keep += [subs, info]
    b = SO.mesh_out(p, env, nv, ni, 2 * len(specs) + 1)
    routes = p.out(env.torch.zeros(len(specs) + 16, dtype=env.torch.int32, device="cuda:0"), used=len(specs) * 4)
    out = b.out_struct()

    def call():
        env.rt._check(env.lib.vgx_concave_triangulate_nested(ctx.handle, poly.data_ptr(), subs.data_ptr(), info.data_ptr(), draws.data_ptr(), len(fl.specs), C.byref(out),
                                                            routes.data_ptr(), b.dev_sizes.data_ptr(), b.dev_status.data_ptr(), env.rt._stream_ptr()),
                      "vgx_concave_triangulate_nested")
    p.call = call
    return p


if not any(r.entry == ENTRY for r in SO.CASES):
    SO.CASES.append(SO.Row(ENTRY, make_concave_triangulate_nested, header="stream-ordered with no host round trip"))
