"""View culling of cached drawings, one job on one box, warmed up, the variants alternating. A 100 x 100 grid of cached Tigers (10 000
drawings, the benchmark's size), once as one instance per DRAW (2.4 M instances of 1-3 meshes) and once as one instance per DRAWING
(10 000 instances of 435 meshes):
  (a) baseline: vgx_cache_submit of all instances (the behaviour before culling existed; that code is unchanged);
  (b) culled:   vgx_cache_cull + vgx_cache_submit, the view showing 1/16, 1/4 and all of the grid ("all" = the overhead of the pass);
  (c) kernels:  vgx_mesh_bounds over the all-instances frame, and vgx_cache_cull alone (out of place, no boxes, no list; a call of a 10 000-instance pass is mostly launch + synchronise) for both range
                shapes (keys *_cull_lane_*: one lane per range; the *_cull_wave32_* keys of the recorded cache_cull_timing.json are
                the wave-reduced form that was removed), as bytes
                read + written per second beside a plain device-to-device copy of 1 GiB timed in the same job.
Every sample is a host clock around `call(s); synchronise`. Buffers and scratch are sized before the clock starts.

python profiles/cache_cull_timing.py [--rounds R] [--drawings-side S] [--out FILE]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--drawings-side", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    S = args.drawings_side
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "drawings": S * S}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(name, v):
        v = sorted(v)
        res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = v[len(v) // 2], v[0], v[-1]

    def make_cache(ctx):
        ps, d = wl.tiger(1)
        pset = rt.PathSet(ctx, ps)
        dd = rt.upload_draws(d)
        sizes = rt.tessellate_count(ctx, pset, dd, d.shape[0])
        bufs = rt.MeshBuffers(dev, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
        rt.tessellate_emit(ctx, pset, dd, d.shape[0], bufs)
        cache = rt.MeshCache(ctx, bufs, sizes, dd, d.shape[0])
        torch.cuda.synchronize()
        pset.close()
        return cache

    ctx = rt.Context(0)
    cache = make_cache(ctx)
    mb = cache.bounds
    box = mb.cpu().numpy()
    lo, hi = box[:, :2].min(axis=0), box[:, 2:].max(axis=0)
    pitch = 1.25 * float(max(hi - lo))
    meshes = cache.bufs.meshes[:cache.nm * 32].cpu().numpy().view(capi.mesh_dtype)
    # the meshes of one draw are consecutive: one range per draw
    draw_first = np.flatnonzero(np.r_[True, meshes["draw"][1:] != meshes["draw"][:-1]])
    draw_count = np.diff(np.r_[draw_first, cache.nm])
    res["cache_meshes"], res["cache_vertices"], res["cache_draw_ranges"] = cache.nm, cache.nv, int(draw_first.shape[0])

    def instances(per_draw):
        k = draw_first.shape[0] if per_draw else 1
        inst = np.zeros(S * S * k, dtype=capi.cache_instance_dtype)
        cell = np.repeat(np.arange(S * S), k)
        inst["first_mesh"] = np.tile(draw_first, S * S) if per_draw else 0
        inst["num_meshes"] = np.tile(draw_count, S * S) if per_draw else cache.nm
        inst["color"] = 0xFFFFFFFF
        inst["mtx"][:, 0] = inst["mtx"][:, 3] = 1.0
        inst["mtx"][:, 4] = (cell % S) * pitch - lo[0]
        inst["mtx"][:, 5] = (cell // S) * pitch - lo[1]
        return inst

    def view_of(fraction_side):
        """The view that shows fraction_side x fraction_side of the grid, from its origin."""
        e = (S * fraction_side - 0.1) * pitch  # a drawing fills 0.8 of its cell: the last shown column ends inside, the next starts outside
        return np.array([[0.0, 0.0, e, e]], dtype=np.float32)

    nv_all, ni_all, nm_all = cache.nv * S * S, cache.ni * S * S, cache.nm * S * S
    out = rt.MeshBuffers(dev, nv_all, ni_all, nm_all)
    # the ruler: a plain copy
    a1 = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    a2 = torch.empty_like(a1)
    for _ in range(3):
        a2.copy_(a1)
    v = sorted(sample(lambda: a2.copy_(a1)) for _ in range(args.rounds))
    res["copy_ms_median"], res["copy_TBps"] = v[len(v) // 2], 2 * a1.numel() * 4 / v[len(v) // 2] / 1e9
    del a1, a2

    for shape in ("per_draw", "per_drawing"):
        inst = instances(shape == "per_draw")
        n = inst.shape[0]
        src = up(inst)
        views = {k: torch.from_numpy(view_of(f)).to(dev) for k, f in (("sixteenth", 0.25), ("quarter", 0.5), ("all", 1.0))}
        nk = {}

        def baseline():
            rt.cache_submit(ctx, cache, src, n, out)

        keep = rt.cache_cull(ctx, cache, mb, src, n, views["all"], want_bounds=False, want_kept=False)  # the output array, allocated once

        def culled(vd):
            def run():
                r = rt.cache_cull(ctx, cache, mb, src, n, vd, reuse=keep)
                rt.cache_submit(ctx, cache, r.inst, n, out)
            return run
        calls = {"a_all": baseline}
        for k, vd in views.items():
            calls["b_" + k] = culled(vd)
            r = rt.cache_cull(ctx, cache, mb, src, n, vd, want_bounds=False)
            nk[k] = int(r.num_kept.item())
            res["%s_kept_%s" % (shape, k)] = nk[k]
        names = sorted(calls)
        for _ in range(2):
            for k in names:
                calls[k]()
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        t = {k: [] for k in names}
        for r in range(args.rounds):
            for k in names[r % len(names):] + names[:r % len(names)]:
                t[k].append(sample(calls[k]))
        res[shape + "_instances"] = n
        for k in names:
            stats("%s_%s" % (shape, k), t[k])
        for k in views:
            res["%s_b_%s_over_a" % (shape, k)] = res["%s_b_%s_ms_median" % (shape, k)] / res["%s_a_all_ms_median" % shape]
        # (c) the cull pass alone
        vd = views["quarter"]

        def cull_only():  # out of place into the array allocated above: every record read and written once, nothing to restore
            rt.cache_cull(ctx, cache, mb, src, n, vd, reuse=keep)
        for _ in range(3):
            cull_only()
        stats("%s_cull_lane" % shape, [sample(cull_only) for _ in range(args.rounds)])
        ms = res["%s_cull_lane_ms_median" % shape]
        moved = 2 * n * 40 + int(inst["num_meshes"].astype(np.int64).sum()) * 16  # records in and out, the boxes of every range (L2)
        res["%s_cull_lane_bytes" % shape] = moved
        res["%s_cull_lane_TBps" % shape] = moved / ms / 1e9
        del src

    # (c) vgx_mesh_bounds over the all-instances frame (what the per-drawing baseline left in `out`)
    inst = instances(False)
    rt.cache_submit(ctx, cache, up(inst), inst.shape[0], out)
    torch.cuda.synchronize()
    for _ in range(3):
        b = rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)
    v = sorted(sample(lambda: rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)) for _ in range(args.rounds))
    ms = v[len(v) // 2]
    moved = nv_all * 8 + nm_all * (32 + 64)  # positions, mesh records, the table: init, store, decode read + write
    res["mesh_bounds_meshes"], res["mesh_bounds_vertices"] = nm_all, nv_all
    res["mesh_bounds_ms_median"], res["mesh_bounds_ms_min"], res["mesh_bounds_ms_max"] = ms, v[0], v[-1]
    res["mesh_bounds_bytes"], res["mesh_bounds_TBps"] = moved, moved / ms / 1e9
    res["mesh_bounds_vs_copy"] = res["mesh_bounds_TBps"] / res["copy_TBps"]
    # spot check: the first drawing's boxes of the frame are the cache's boxes moved by its translation (m1 = m2 = 0)
    got = b[:cache.nm].cpu().numpy()
    want = box + np.array([inst["mtx"][0][4], inst["mtx"][0][5]] * 2, dtype=np.float32)
    res["mesh_bounds_first_drawing_matches"] = bool(np.array_equal(got, want))
    ctx.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
