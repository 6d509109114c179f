"""vgx_concave_triangulate_nested beside vgx_concave_triangulate_rings and vgx_concave_contours: one job on one box, warmed up, the
variants alternating; host clock around `call; synchronise`, buffers and scratch sized before the clock starts; medians and ranges of
--rounds rounds. There is no threshold.
  holes_*      (1) --draws draws of a 48-vertex star with two 8-vertex holes through this entry and through the rings entry: the same
                   work, the outputs asserted equal -- the price for draws the rings entry accepts
  word_*       (2) --draws draws of the word "oBioBio" (16 sub-paths, 9 groups, 64 vertices): this entry and vgx_concave_contours;
  raster_*         downstream, vgx_raster_concave of the triangulated frame and of the contour frame into a --size image, images equal
  islands_*, grid_* (3) one draw each: a square with 144 seven-vertex holes and a triangle in every hole (145 groups) through this
                   entry; the square with its holes alone through the rings entry
  max_*        (4) one draw of 819 rings in 4096 slots (818 triangles and a hexagon), this entry and vgx_concave_contours
  old_*, oldrings_* (5) with --parent-lib: vgx_concave_triangulate on single-ring stars and vgx_concave_triangulate_rings on the holed
                   stars of (1), this build against the library given, in child processes that alternate (each: warm-up, then --rounds
                   samples; two children per library). The yardstick is the parent library's own run-to-run range

python profiles/concave_nested_timing.py [--rounds R] [--draws N] [--size S] [--parent-lib libvgx.so] [--out FILE]   (prints one JSON object)"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF
WIDE = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--draws", type=int, default=10000)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-lib", default=None, help="internal: time the two older entries of this library and print the samples")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concave_nested_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    capi = rt.capi
    if args.child_lib:
        rt.LIB_PATH = args.child_lib
        if not hasattr(C.CDLL(args.child_lib), "vgx_concave_triangulate_nested"):
            capi.VGX_SYMBOLS.pop("vgx_concave_triangulate_nested")
    dev = torch.device("cuda", 0)
    F = np.float32
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "draws": args.draws, "size": args.size, "cap": capi.TRIANGULATE_MAX_VERTICES}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def alternate(calls):
        names = sorted(calls)
        for _ in range(3):
            for k in names:
                calls[k]()
        t = {k: [] for k in names}
        for r in range(args.rounds):
            for k in names[r % len(names):] + names[:r % len(names)]:
                t[k].append(sample(calls[k]))
        for k in names:
            v = sorted(t[k])
            res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = v[len(v) // 2], v[0], v[-1]
        return t

    def star(cx, cy, r0, r1, points, phase):
        a = phase + np.arange(2 * points) * (np.pi / points)
        rad = np.where(np.arange(2 * points) % 2 == 0, r0, r1)
        return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], axis=1).astype(F)

    def flat(draw_rings, colors):
        """What vgx_flatten leaves for one concave draw per entry of draw_rings (a list of rings each)."""
        n = len(draw_rings)
        rings = [r for d in draw_rings for r in d]
        per = np.array([len(d) for d in draw_rings], dtype=np.uint64)
        counts = np.array([len(r) for r in rings], dtype=np.uint64)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        subs = np.zeros(len(rings), dtype=capi.subpath_dtype)
        subs["first_vertex"], subs["num_vertices"], subs["flags"] = first, counts, 1
        first_sub = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.uint64)
        verts = np.add.reduceat(counts, first_sub.astype(np.int64))
        info = np.zeros(n, dtype=capi.draw_info_dtype)
        info["first_poly_vertex"], info["first_subpath"], info["num_poly_vertices"], info["num_subpaths"] = first[first_sub.astype(np.int64)], first_sub, verts, per
        draws = np.zeros(n, dtype=capi.draw_dtype)
        draws["fill_flags"], draws["fill_color"], draws["fringe"], draws["scale"], draws["tess_tol"] = capi.FILL_CONCAVE, colors, 1.0, 1.0, 0.25
        return [up(np.concatenate(rings)), up(subs), up(info), up(draws)], n, int(counts.sum())

    ctx = rt.Context(0)
    lib = rt.lib()

    def entry(name, tensors, n, b, routes):
        fn = getattr(lib, name)

        def call():
            out = b.out_struct()
            if routes is None:
                rt._check(fn(ctx.handle, *[t.data_ptr() for t in tensors], n, C.byref(out), b.dev_sizes.data_ptr(), b.dev_status.data_ptr(), rt._stream_ptr()), name)
            else:
                rt._check(fn(ctx.handle, *[t.data_ptr() for t in tensors], n, C.byref(out), routes.data_ptr(), b.dev_sizes.data_ptr(), b.dev_status.data_ptr(),
                             rt._stream_ptr()), name)
        return call

    def compare(tensors, n, V, prefix, variants):
        """variants: key -> entry name. Every triangulating variant must triangulate every draw."""
        bufs = {k: rt.MeshBuffers(dev, V, 5 * V, n) for k in variants}
        routes = {k: (None if e == "vgx_concave_contours" else torch.zeros(n, dtype=torch.int32, device=dev)) for k, e in variants.items()}
        alternate({prefix + "_" + k: entry(e, tensors, n, bufs[k], routes[k]) for k, e in variants.items()})
        torch.cuda.synchronize()
        for k in variants:
            assert int(bufs[k].dev_status.item()) == 0, (prefix, k)
            assert routes[k] is None or bool((routes[k] == capi.TRI_ROUTE_TRIANGLES).all()), "a draw of the timing input fell back"
        return bufs

    side = int(np.ceil(np.sqrt(args.draws)))
    pitch = args.size / side
    rs = np.random.RandomState(5)
    centres = [((k % side + 0.5) * pitch, (k // side + 0.5) * pitch) for k in range(args.draws)]
    phases = rs.uniform(0, 6.28, args.draws)
    colors = (0x80 << 24) | rs.randint(0, 1 << 24, args.draws).astype(np.uint32)
    holes = [[star(x, y, 0.62 * pitch, 0.40 * pitch, 24, p), star(x - 0.14 * pitch, y, 0.09 * pitch, 0.05 * pitch, 4, 0.3)[::-1].copy(),
              star(x + 0.14 * pitch, y, 0.09 * pitch, 0.05 * pitch, 4, 0.8)[::-1].copy()] for (x, y), p in zip(centres, phases)]
    t1, n1, V1 = flat(holes, colors)
    if args.child_lib:
        ts, ns, Vs = flat([[star(x, y, 0.62 * pitch, 0.27 * pitch, 32, p)] for (x, y), p in zip(centres, phases)], colors)
        b, b1 = rt.MeshBuffers(dev, Vs, 5 * Vs, ns), rt.MeshBuffers(dev, V1, 5 * V1, n1)
        t = alternate({"old": entry("vgx_concave_triangulate", ts, ns, b, torch.zeros(ns, dtype=torch.int32, device=dev)),
                       "oldrings": entry("vgx_concave_triangulate_rings", t1, n1, b1, torch.zeros(n1, dtype=torch.int32, device=dev))})
        print(json.dumps(t))
        ctx.close()
        return

    # ---- (1) a 48-vertex star with two 8-vertex holes per draw: this entry and the rings entry ----
    res["holes_vertices"] = V1
    a = compare(t1, n1, V1, "holes", {"nested": "vgx_concave_triangulate_nested", "rings": "vgx_concave_triangulate_rings"})
    nv, ni = (int(v) for v in a["rings"].dev_sizes.cpu().numpy()[3:5])
    assert all(torch.equal(getattr(a["nested"], f)[:k], getattr(a["rings"], f)[:k]) for f, k in (("pos", nv), ("color", nv), ("idx", ni))), "the two entries differ on one group"
    res["holes_difference_ms"] = res["holes_nested_ms_median"] - res["holes_rings_ms_median"]
    res["holes_rings_range_ms"] = res["holes_rings_ms_max"] - res["holes_rings_ms_min"]
    res["holes_difference_exceeds_rings_range"] = abs(res["holes_difference_ms"]) > res["holes_rings_range_ms"]

    # ---- (2) the word "oBioBio" per draw, scaled into its cell ----
    def sq(x, y, w, h, hole=False):
        p = np.array([(x, y), (x + w, y), (x + w, y + h), (x, y + h)], dtype=np.float64)
        return p[::-1].copy() if hole else p

    word = []
    for k, ch in enumerate("oBioBio"):
        x = 2.0 + 13.0 * k
        if ch == "o":
            word += [sq(x, 10, 10, 10), sq(x + 2.5, 12.5, 5, 5, True)]
        elif ch == "B":
            word += [sq(x, 10, 10, 14), sq(x + 2, 12, 3.5, 3.5, True), sq(x + 2, 18, 3.5, 3.5, True)]
        else:
            word += [sq(x + 3, 15, 4, 10), sq(x + 3, 9, 4, 4)]
    word = [word[k] for k in np.random.RandomState(5).permutation(len(word))]
    scale = pitch / 96.0
    words = [[((r - (46.0, 17.0)) * scale + (x, y)).astype(F) for r in word] for (x, y) in centres]
    t2, n2, V2 = flat(words, colors)
    res["word_vertices"] = V2
    hb = compare(t2, n2, V2, "word", {"nested": "vgx_concave_triangulate_nested", "contours": "vgx_concave_contours"})
    res["word_cost_ms"] = res["word_nested_ms_median"] - res["word_contours_ms_median"]

    # ---- (3) the grid with an island in every hole against the grid alone, one draw each ----
    grid = [np.array([(0, 0), (200, 0), (200, 200), (0, 200)], dtype=F)]
    islands = []
    for iy in range(12):
        for ix in range(12):
            ang = 0.1 * ix + np.arange(7) * (2 * np.pi / 7)
            rad = np.array([6.0, 3.0, 6.0, 3.0, 6.0, 3.0, 4.5])
            cx, cy = 12.0 + 16 * ix, 12.0 + 16 * iy
            grid.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).astype(F)[::-1].copy())
            islands.append(np.array([(cx + 0.75, cy), (cx - 0.5, cy + 0.75), (cx - 0.5, cy - 0.75)], dtype=F))
    one = np.array([0x80FF8040], dtype=np.uint32)
    t3, n3, V3 = flat([grid + islands], one)
    compare(t3, n3, V3, "islands", {"nested": "vgx_concave_triangulate_nested"})
    t3b, n3b, V3b = flat([grid], one)
    compare(t3b, n3b, V3b, "grid", {"rings": "vgx_concave_triangulate_rings", "nested": "vgx_concave_triangulate_nested"})

    # ---- (4) 819 rings in 4096 slots ----
    cap = capi.TRIANGULATE_MAX_VERTICES
    many = []
    for k in range(819):
        x, y = 3.0 * (k % 32), 3.0 * (k // 32)
        pts = [(x, y), (x + 2, y), (x, y + 2)] if k < 818 else [(x, y), (x + 1, y), (x + 2, y), (x + 2, y + 1), (x + 1, y + 2), (x, y + 2)]
        many.append(np.array(pts, dtype=F))
    t4, n4, V4 = flat([many], one)
    assert V4 + 2 * 818 == cap
    compare(t4, n4, V4, "max", {"nested": "vgx_concave_triangulate_nested", "contours": "vgx_concave_contours"})

    # ---- (2, downstream) the two frames of the words through vgx_raster_concave ----
    dtab = np.zeros(n2, dtype=capi.draw_dtype)
    stab = np.zeros(n2, dtype=capi.draw_state_dtype)
    stab["scissor"], stab["clip_first_draw"] = (0, 0, WIDE, WIDE), NONE
    dd, ds = up(dtab), up(stab)
    uv = torch.zeros((V2, 2), dtype=torch.int16, device=dev)
    rt.raster_reserve(ctx, n2, 1 << 22)
    images = {}

    def raster_of(kind):
        b = hb[kind]
        nm, nv, ni = (int(v) for v in b.dev_sizes.cpu().numpy()[2:5])
        desc = rt.mesh_seq(b, nv, ni, nm)
        image = torch.zeros((args.size, args.size), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def call():
            rt.raster_concave(ctx, desc, dd, ds, n2, uv, 4, None, 0, None, 0, None, 0, args.size, args.size, clear_color=0xFF202020, image=image, dev_status=status)

        for _ in range(4):   # a first call may end with VGX_E_GROWN: grow before the clock starts
            call()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                break
        assert int(status.item()) == 0, int(status.item())
        images[kind] = (image, status)
        return call

    alternate({"raster_triangles": raster_of("nested"), "raster_contours": raster_of("contours")})
    torch.cuda.synchronize()
    x, y = images["nested"][0].cpu().numpy(), images["contours"][0].cpu().numpy()
    assert int(images["nested"][1].item()) == 0 and int(images["contours"][1].item()) == 0
    assert np.array_equal(x, y), "the triangulated frame and the contour frame differ"
    res["raster_pixels_covered"] = int((x.view(np.uint32) != 0xFF202020).sum())
    res["raster_images_equal"] = True
    res["raster_cost_ms"] = res["raster_triangles_ms_median"] - res["raster_contours_ms_median"]
    res["scratch_bytes"] = int(ctx.scratch_bytes())
    ctx.close()

    # ---- (5) the two older entries, this build against the parent's library: processes alternating ----
    if args.parent_lib:
        samples = {"this": {"old": [], "oldrings": []}, "parent": {"old": [], "oldrings": []}}
        for k in ("this", "parent", "parent", "this"):
            path = rt.LIB_PATH if k == "this" else os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-lib", path, "--rounds", str(args.rounds), "--draws", str(args.draws), "--size", str(args.size)],
                                 check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            got = json.loads(out.strip().splitlines()[-1])
            for e in got:
                samples[k][e] += got[e]
        for e in ("old", "oldrings"):
            for k in ("this", "parent"):
                v = sorted(samples[k][e])
                res[e + "_" + k + "_ms_median"], res[e + "_" + k + "_ms_min"], res[e + "_" + k + "_ms_max"] = v[len(v) // 2], v[0], v[-1]
            res[e + "_difference_ms"] = res[e + "_this_ms_median"] - res[e + "_parent_ms_median"]
            res[e + "_parent_range_ms"] = res[e + "_parent_ms_max"] - res[e + "_parent_ms_min"]
            res[e + "_difference_exceeds_parent_range"] = abs(res[e + "_difference_ms"]) > res[e + "_parent_range_ms"]
    text = json.dumps(res, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
