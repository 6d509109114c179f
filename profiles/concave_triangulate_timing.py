"""vgx_concave_triangulate beside vgx_concave_contours: one job on one box, warmed up, the variants alternating; host clock around `call;
synchronise`, buffers and scratch sized before the clock starts; medians and ranges of --rounds rounds.
  stars_*      --stars translucent 64-edge stars (one draw each, no AA) on a grid: both calls on the same flatten output
  cap_*        ONE ring of VGX_TRIANGULATE_MAX_VERTICES vertices: the O(V^2) edge-pair test and the one-wave clipping loop at their largest
  raster_*     downstream: vgx_raster_concave of the stars' triangulated frame and of their contour frame into a --size image; the two
               images are asserted equal
There is no threshold. `*_cost_ms` = median(triangulate) - median(contours).

python profiles/concave_triangulate_timing.py [--rounds R] [--stars N] [--size S] [--out FILE]   (prints one JSON object)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF
WIDE = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--stars", type=int, default=10000)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "concave_triangulate_timing.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    F = np.float32
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "stars": args.stars, "size": args.size, "cap": capi.TRIANGULATE_MAX_VERTICES}

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

    def star(cx, cy, r0, r1, points, phase):
        a = phase + np.arange(2 * points) * (np.pi / points)
        rad = np.where(np.arange(2 * points) % 2 == 0, r0, r1)
        return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], axis=1).astype(F)

    def flat(rings, colors):
        """What vgx_flatten leaves for one single-ring concave draw per ring."""
        n = len(rings)
        counts = np.array([len(r) for r in rings], dtype=np.uint64)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        subs = np.zeros(n, dtype=capi.subpath_dtype)
        subs["first_vertex"], subs["num_vertices"], subs["flags"] = first, counts, 1
        info = np.zeros(n, dtype=capi.draw_info_dtype)
        info["first_poly_vertex"], info["first_subpath"], info["num_poly_vertices"], info["num_subpaths"] = first, np.arange(n), counts, 1
        draws = np.zeros(n, dtype=capi.draw_dtype)
        draws["fill_flags"], draws["fill_color"], draws["fringe"], draws["scale"], draws["tess_tol"] = capi.FILL_CONCAVE, colors, 1.0, 1.0, 0.25
        return [up(np.concatenate(rings)), up(subs), up(info), up(draws)], n, int(counts.sum())

    ctx = rt.Context(0)
    lib = rt.lib()

    def calls_for(tensors, n, V, prefix):
        bufs = {k: rt.MeshBuffers(dev, V, 3 * V, n) for k in ("triangulate", "contours")}
        routes = torch.zeros(n, dtype=torch.int32, device=dev)

        def tri():
            b = bufs["triangulate"]
            out = b.out_struct()
            rt._check(lib.vgx_concave_triangulate(ctx.handle, *[t.data_ptr() for t in tensors], n, C.byref(out), routes.data_ptr(), b.dev_sizes.data_ptr(),
                                                  b.dev_status.data_ptr(), rt._stream_ptr()), "vgx_concave_triangulate")

        def con():
            b = bufs["contours"]
            out = b.out_struct()
            rt._check(lib.vgx_concave_contours(ctx.handle, *[t.data_ptr() for t in tensors], n, C.byref(out), b.dev_sizes.data_ptr(), b.dev_status.data_ptr(),
                                               rt._stream_ptr()), "vgx_concave_contours")

        alternate({prefix + "_triangulate": tri, prefix + "_contours": con})
        torch.cuda.synchronize()
        assert int(bufs["triangulate"].dev_status.item()) == 0 and int(bufs["contours"].dev_status.item()) == 0
        assert bool((routes == capi.TRI_ROUTE_TRIANGLES).all()), "a ring of the timing input fell back"
        res[prefix + "_cost_ms"] = res[prefix + "_triangulate_ms_median"] - res[prefix + "_contours_ms_median"]
        return bufs

    # ---- the stars ----
    side = int(np.ceil(np.sqrt(args.stars)))
    pitch = args.size / side
    rs = np.random.RandomState(5)
    rings = [star((k % side + 0.5) * pitch, (k // side + 0.5) * pitch, 0.62 * pitch, 0.27 * pitch, 32, rs.uniform(0, 6.28)) for k in range(args.stars)]
    colors = (0x80 << 24) | rs.randint(0, 1 << 24, args.stars).astype(np.uint32)
    tensors, n, V = flat(rings, colors)
    res["stars_vertices"] = V
    sb = calls_for(tensors, n, V, "stars")

    # ---- one ring at the cap ----
    cap = capi.TRIANGULATE_MAX_VERTICES
    t1, n1, V1 = flat([star(1000.0, 1000.0, 900.0, 780.0, cap // 2, 0.003)], np.array([0x80FF8040], dtype=np.uint32))
    calls_for(t1, n1, V1, "cap")

    # ---- downstream: the two frames of the stars through vgx_raster_concave ----
    dtab = np.zeros(n, dtype=capi.draw_dtype)
    stab = np.zeros(n, dtype=capi.draw_state_dtype)
    stab["scissor"], stab["clip_first_draw"] = (0, 0, WIDE, WIDE), NONE
    dd, ds = up(dtab), up(stab)
    uv = torch.zeros((V, 2), dtype=torch.int16, device=dev)
    rt.raster_reserve(ctx, n, 1 << 22)
    images = {}

    def raster_of(kind):
        b = sb[kind]
        nm, nv, ni = (int(v) for v in b.dev_sizes.cpu().numpy()[2:5])
        desc = rt.mesh_seq(b, nv, ni, nm)
        image = torch.zeros((args.size, args.size), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def call():
            rt.raster_concave(ctx, desc, dd, ds, n, uv, 4, None, 0, None, 0, None, 0, args.size, args.size, clear_color=0xFF202020, image=image, dev_status=status)

        for _ in range(4):   # a first call may end with VGX_E_GROWN: grow before the clock starts
            call()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                break
        assert int(status.item()) == 0, int(status.item())
        images[kind] = (image, status)
        return call

    alternate({"raster_triangles": raster_of("triangulate"), "raster_contours": raster_of("contours")})
    torch.cuda.synchronize()
    a, b = images["triangulate"][0].cpu().numpy(), images["contours"][0].cpu().numpy()
    assert int(images["triangulate"][1].item()) == 0 and int(images["contours"][1].item()) == 0
    assert np.array_equal(a, b), "the triangulated frame and the contour frame differ"
    res["raster_pixels_covered"] = int((a.view(np.uint32) != 0xFF202020).sum())
    res["raster_images_equal"] = True
    res["raster_cost_ms"] = res["raster_triangles_ms_median"] - res["raster_contours_ms_median"]
    res["scratch_bytes"] = int(ctx.scratch_bytes())
    ctx.close()
    text = json.dumps(res, indent=1, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
