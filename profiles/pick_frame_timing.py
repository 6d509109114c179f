"""vgx_pick_frame beside vgx_pick: one job on one box, warmed up, the variants alternating; host clock around `call; synchronise`, buffers
and scratch sized before the clock starts; medians and ranges of --rounds rounds.
  grid_*      the grid of cached Tigers of profiles/pick_timing.py (one instance per drawing, boxes taken once by vgx_mesh_bounds), 1 / 16 /
              256 cursor positions through vgx_pick_frame under an all-PLAIN draw table (one draw per instance, type 0, no region, a scissor
              that cuts nothing) and through vgx_pick on the same frame and queries. The grid is scaled to fit the largest draw scissor
              (65 535 frame pixels), so its numbers are NOT those of pick_timing.json
  region_*    the Tiger frame of profiles/raster_frame_timing.py under one In region over the left half of a 1024 window (a clip quad in
              front of the frame's meshes), 256 positions over the window: vgx_pick_frame, and vgx_pick on the same streams
  stacked_*   the worst case of pick_timing.py: 1 000 Tigers under ONE transform, 1 and 256 positions inside the drawing
Per section `*_cost_ms` = median(vgx_pick_frame) - median(vgx_pick), `*_pick_range_ms` = max - min of vgx_pick in that job, and whether the
cost exceeds that range. Where the two calls must agree (the grid and the stack: PLAIN, no contour mesh, random points off every edge) the
hit records are compared.
`--trace-only` runs the 256-position grid and stacked calls a few times and nothing else: the program of a rocprofv3 --kernel-trace
--stats run, which says which kernel carries a cost.

python profiles/pick_frame_timing.py [--rounds R] [--drawings-side S] [--stacked N] [--out FILE]   (prints one JSON object)"""
import argparse
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
    ap.add_argument("--drawings-side", type=int, default=100)
    ap.add_argument("--stacked", type=int, default=1000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    S = args.drawings_side
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "drawings": S * S, "stacked_drawings": args.stacked}

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

    def compare(section, new, old):
        res[section + "_cost_ms"] = res[new + "_ms_median"] - res[old + "_ms_median"]
        res[section + "_pick_range_ms"] = res[old + "_ms_max"] - res[old + "_ms_min"]
        res[section + "_cost_exceeds_pick_range"] = bool(res[section + "_cost_ms"] > res[section + "_pick_range_ms"])

    def plain_table(nd):
        draws = np.zeros(nd, dtype=capi.draw_dtype)
        st = np.zeros(nd, dtype=capi.draw_state_dtype)
        st["scissor"] = (0, 0, WIDE, WIDE)
        st["clip_first_draw"] = NONE
        return up(draws), up(st), nd

    def queries(pts):
        q = np.zeros(len(pts), dtype=capi.pick_query_dtype)
        q["x"], q["y"], q["mesh_end"] = [p[0] for p in pts], [p[1] for p in pts], NONE
        return q

    ctx = rt.Context(0)
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(ctx, pset, dd, d.shape[0])
    cb = rt.MeshBuffers(dev, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(ctx, pset, dd, d.shape[0], cb)
    cache = rt.MeshCache(ctx, cb, sizes, dd, d.shape[0])
    torch.cuda.synchronize()
    box = cache.bounds.cpu().numpy()
    lo, hi = box[:, :2].min(axis=0), box[:, 2:].max(axis=0)
    pitch = 1.25 * float(max(hi - lo))
    res["cache_meshes"] = cache.nm

    def submit(inst):
        n = inst.shape[0]
        out = rt.MeshBuffers(dev, cache.nv * n, cache.ni * n, cache.nm * n)
        rt.cache_submit(ctx, cache, up(inst), n, out)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        return out, capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), cache.nm * n, cache.nv * n, cache.ni * n)

    hd = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 256)}
    hf = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 256)}
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    # ---- the grid, scaled so that every drawing lies inside the largest draw scissor --------------------------------------------
    k = min(1.0, 65000.0 / (S * pitch))
    inst = np.zeros(S * S, dtype=capi.cache_instance_dtype)
    cell = np.arange(S * S)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:, 0] = inst["mtx"][:, 3] = k
    inst["mtx"][:, 4], inst["mtx"][:, 5] = k * ((cell % S) * pitch - lo[0]), k * ((cell // S) * pitch - lo[1])
    out, desc = submit(inst)
    nm_all = cache.nm * S * S
    rs = np.random.RandomState(4)
    qcell = rs.randint(0, S * S, 256)
    pts = [(k * ((c % S) * pitch + rs.uniform(0.3, 0.7) * (hi[0] - lo[0])), k * ((c // S) * pitch + rs.uniform(0.3, 0.7) * (hi[1] - lo[1]))) for c in qcell]
    q = queries(pts)
    mb = rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)
    qd = {n: up(q[:n]) for n in (1, 16, 256)}
    dt = plain_table(S * S)
    res["grid_scale"], res["grid_meshes"] = k, nm_all

    def grid_frame(n):
        rt.pick_frame(ctx, desc, dt[0], dt[1], dt[2], qd[n], n, mb, hits_dev=hf[n], dev_status=status)

    if args.trace_only:
        for _ in range(6):
            grid_frame(256)
            rt.pick(ctx, desc, qd[256], 256, mb, hd[256])
        torch.cuda.synchronize()
    else:
        calls = {}
        for n in (1, 16, 256):
            calls["grid_q%d_pick_frame" % n] = (lambda n=n: grid_frame(n))
            calls["grid_q%d_pick" % n] = (lambda n=n: rt.pick(ctx, desc, qd[n], n, mb, hd[n]))
        alternate(calls)
        for n in (1, 16, 256):
            compare("grid_q%d" % n, "grid_q%d_pick_frame" % n, "grid_q%d_pick" % n)
        torch.cuda.synchronize()
        res["grid_status"] = int(status.item())
        res["grid_q256_hits"] = int((hf[256].cpu().numpy().view(capi.pick_hit_dtype)["mesh"] != NONE).sum())
        res["grid_q256_equals_pick"] = bool(torch.equal(hf[256], hd[256]))
        res["scratch_bytes_after_grid"] = ctx.scratch_bytes()
    del out, mb, dt

    # ---- the stack ---------------------------------------------------------------------------------------------------------------
    N = args.stacked
    inst = np.zeros(N, dtype=capi.cache_instance_dtype)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:] = [1.0, 0.0, 0.0, 1.0, 100.0 - lo[0], 50.0 - lo[1]]
    out, desc = submit(inst)
    pts = [(100.0 + rs.uniform(0.3, 0.7) * (hi[0] - lo[0]), 50.0 + rs.uniform(0.3, 0.7) * (hi[1] - lo[1])) for _ in range(256)]
    q = queries(pts)
    mb = rt.mesh_bounds(ctx, out.pos, out.meshes, cache.nm * N)
    qs = {n: up(q[:n]) for n in (1, 256)}
    dt = plain_table(N)

    def stacked_frame(n):
        rt.pick_frame(ctx, desc, dt[0], dt[1], dt[2], qs[n], n, mb, hits_dev=hf[n], dev_status=status)

    if args.trace_only:
        for _ in range(6):
            stacked_frame(256)
            rt.pick(ctx, desc, qs[256], 256, mb, hd[256])
        torch.cuda.synchronize()
        ctx.close()
        return
    calls = {}
    for n in (1, 256):
        calls["stacked_q%d_pick_frame" % n] = (lambda n=n: stacked_frame(n))
        calls["stacked_q%d_pick" % n] = (lambda n=n: rt.pick(ctx, desc, qs[n], n, mb, hd[n]))
    alternate(calls)
    for n in (1, 256):
        compare("stacked_q%d" % n, "stacked_q%d_pick_frame" % n, "stacked_q%d_pick" % n)
    torch.cuda.synchronize()
    hits = hf[256].cpu().numpy().view(capi.pick_hit_dtype)
    res["stacked_q256_hits"] = int((hits["mesh"] != NONE).sum())
    res["stacked_hits_in_the_top_copy"] = bool(np.all(hits["draw"][hits["mesh"] != NONE] == N - 1))
    res["stacked_q256_equals_pick"] = bool(torch.equal(hf[256], hd[256]))
    del out, mb, dt

    # ---- one Tiger under one In region over the left half of the window ------------------------------------------------------------
    size = args.size
    probe = rt.tessellate(ctx, pset, dd, d.shape[0])
    plo = np.floor(probe.pos.reshape(-1, 2).min(axis=0))
    d2 = d.copy()
    d2["mtx"][:, 4] -= np.float32(plo[0])  # the drawing's corner to the frame's origin: a draw scissor is unsigned
    d2["mtx"][:, 5] -= np.float32(plo[1])
    got = rt.tessellate(ctx, pset, rt.upload_draws(d2), d2.shape[0])
    pset.close()
    nd = d2.shape[0]
    pos = got.pos.reshape(-1, 2)
    nm = got.meshes.shape[0]
    quad = np.array([(0, 0), (size // 2, 0), (size // 2, size), (0, size)], dtype=np.float32)
    tab = np.zeros(nm + 1, dtype=capi.mesh_dtype)
    tab[1:] = got.meshes
    tab["first_vertex"][1:] += 4
    tab["first_index"][1:] += 6
    tab["num_vertices"][0], tab["num_indices"][0], tab["draw"][0] = 4, 6, nd
    keep = [up(np.concatenate([quad, pos]).astype(np.float32)), up(np.concatenate([np.full(4, 0xFFFFFFFF, dtype=np.uint32), got.color])),
            up(np.concatenate([np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), got.idx])), up(tab)]
    desc = capi.CacheDesc(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), nm + 1, pos.shape[0] + 4, got.idx.shape[0] + 6)
    draws = np.zeros(nd + 1, dtype=capi.draw_dtype)
    st = np.zeros(nd + 1, dtype=capi.draw_state_dtype)
    st["scissor"] = (0, 0, size, size)
    st["clip_first_draw"] = NONE
    st["clip_first_draw"][:nd], st["clip_num_draws"][:nd], st["clip_rule"][:nd] = nd, 1, 0
    draws["state_key"][nd] = 3 << 16
    dr = (up(draws), up(st), nd + 1)
    ext = pos.max(axis=0)
    q = queries([(rs.uniform(0, min(size, ext[0])), rs.uniform(0, min(size, ext[1]))) for _ in range(256)])
    qr = up(q)
    mb = rt.mesh_bounds(ctx, keep[0].view(torch.float32), keep[3], nm + 1)
    alternate({"region_q256_pick_frame": lambda: rt.pick_frame(ctx, desc, dr[0], dr[1], dr[2], qr, 256, mb, hits_dev=hf[256], dev_status=status),
               "region_q256_pick": lambda: rt.pick(ctx, desc, qr, 256, mb, hd[256])})
    compare("region_q256", "region_q256_pick_frame", "region_q256_pick")
    torch.cuda.synchronize()
    hits, old = hf[256].cpu().numpy().view(capi.pick_hit_dtype), hd[256].cpu().numpy().view(capi.pick_hit_dtype)
    left = q["x"] < size // 2
    res["region_meshes"] = nm + 1
    res["region_hits_left_half"], res["region_hits_right_half"] = int((hits["mesh"][left] != NONE).sum()), int((hits["mesh"][~left] != NONE).sum())
    res["region_pick_hits_right_half"] = int((old["mesh"][~left] != NONE).sum())
    res["region_pick_reports_the_clip_quad"] = int((old["mesh"] == 0).sum())
    res["scratch_bytes"] = ctx.scratch_bytes()
    ctx.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
