"""vgx_pick_rect, one job on one box, every shape warmed up, the variants alternating; host clock around `call; synchronise`, buffers and
scratch sized before the clock starts; medians and ranges of --rounds rounds. On the 100 x 100 grid of cached Tigers submitted whole (one
instance per drawing: 4.35 M meshes), with the caller's boxes (vgx_mesh_bounds taken once):
  point_q*    (a) 1 / 16 / 64 degenerate rectangles against vgx_pick on the same positions: the yardstick. The ratio is reported beside
              vgx_pick's own run-to-run range; the expectation to confirm or refute is "one more plane of words, same traversal". The two
              calls must give the same four words (checked)
  marquee_*   (b) one marquee over 1/256, 1/16 and all of the grid, crossing and window, by mesh and VGX_PICK_RECT_BY_DRAW, list_cap 64,
              with the counts returned. By instance the counts are checked against the instances' boxes (the drawings do not overlap)
  stacked_*   (c) the worst case of profiles/pick_timing.py: 1 000 Tigers under one transform, a +-2-unit square and the whole drawing
Beside them the ruler of the other timing files: a plain device-to-device copy (1 GiB, as TB/s).

python profiles/pick_rect_timing.py [--rounds R] [--drawings-side S] [--stacked N] [--out FILE]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--drawings-side", type=int, default=100)
    ap.add_argument("--stacked", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    S = args.drawings_side
    CAP = 64
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "drawings": S * S, "stacked_drawings": args.stacked, "list_cap": CAP}

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

    def alternate(calls):
        names = sorted(calls)
        for _ in range(2):
            for k in names:
                calls[k]()
        t = {k: [] for k in names}
        for r in range(args.rounds):
            for k in names[r % len(names):] + names[:r % len(names)]:
                t[k].append(sample(calls[k]))
        for k in names:
            stats(k, t[k])

    ctx = rt.Context(0)
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(ctx, pset, dd, d.shape[0])
    cb = rt.MeshBuffers(dev, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(ctx, pset, dd, d.shape[0], cb)
    cache = rt.MeshCache(ctx, cb, sizes, dd, d.shape[0])
    torch.cuda.synchronize()
    pset.close()
    box = cache.bounds.cpu().numpy()
    lo, hi = box[:, :2].min(axis=0), box[:, 2:].max(axis=0)
    ext = hi - lo
    pitch = 1.25 * float(max(ext))

    def submit(inst):
        n = inst.shape[0]
        out = rt.MeshBuffers(dev, cache.nv * n, cache.ni * n, cache.nm * n)
        rt.cache_submit(ctx, cache, up(inst), n, out)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        return out, capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), cache.nm * n, cache.nv * n, cache.ni * n)

    def rects(rows, flags=0):
        q = np.zeros(len(rows), dtype=capi.pick_rect_query_dtype)
        for k, name in enumerate(("x0", "y0", "x1", "y1")):
            q[name] = [r[k] for r in rows]
        q["mesh_end"], q["flags"] = NONE, flags
        return q

    a1 = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    a2 = torch.empty_like(a1)
    for _ in range(3):
        a2.copy_(a1)
    v = sorted(sample(lambda: a2.copy_(a1)) for _ in range(args.rounds))
    res["copy_ms_median"], res["copy_TBps"] = v[len(v) // 2], 2 * a1.numel() * 4 / v[len(v) // 2] / 1e9
    del a1, a2

    # ---- the grid ------------------------------------------------------------------------------------------------------
    inst = np.zeros(S * S, dtype=capi.cache_instance_dtype)
    cell = np.arange(S * S)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:, 0] = inst["mtx"][:, 3] = 1.0
    inst["mtx"][:, 4], inst["mtx"][:, 5] = (cell % S) * pitch - lo[0], (cell // S) * pitch - lo[1]
    out, desc = submit(inst)
    nm_all = cache.nm * S * S
    res["grid_meshes"], res["grid_vertices"], res["grid_indices"] = nm_all, cache.nv * S * S, cache.ni * S * S
    mb = rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)
    rs = np.random.RandomState(4)
    qcell = rs.randint(0, S * S, 64)
    pts = [((c % S) * pitch + rs.uniform(0.3, 0.7) * ext[0], (c // S) * pitch + rs.uniform(0.3, 0.7) * ext[1]) for c in qcell]
    pq = np.zeros(64, dtype=capi.pick_query_dtype)
    pq["x"], pq["y"], pq["mesh_end"] = [p[0] for p in pts], [p[1] for p in pts], NONE
    rq = rects([(x, y, x, y) for x, y in zip(pq["x"], pq["y"])])
    pd, rd = {n: up(pq[:n]) for n in (1, 16, 64)}, {n: up(rq[:n]) for n in (1, 16, 64)}
    hd = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 64)}
    last = {}

    def rect_call(name, qdev, n, frame=None, bounds=None, top=True):
        def fn():
            last[name] = rt.pick_rect(ctx, frame or desc, qdev, n, list_cap=CAP, bounds_dev=mb if bounds is None else bounds, want_top=top)
        return fn

    # (a) the yardstick
    calls = {}
    for n in (1, 16, 64):
        calls["point_q%d_pick" % n] = (lambda n=n: rt.pick(ctx, desc, pd[n], n, mb, hd[n]))
        calls["point_q%d_rect" % n] = rect_call("point_q%d_rect" % n, rd[n], n)
    alternate(calls)
    for n in (1, 16, 64):
        p, r = "point_q%d_pick" % n, "point_q%d_rect" % n
        res["point_q%d_rect_over_pick" % n] = res[r + "_ms_median"] / res[p + "_ms_median"]
        res["point_q%d_pick_max_over_min" % n] = res[p + "_ms_max"] / res[p + "_ms_min"]
    res["point_q64_same_words_as_vgx_pick"] = bool(np.array_equal(last["point_q64_rect"].top.cpu().numpy()[:64 * 16], hd[64].cpu().numpy()))
    res["point_q64_hits"] = int((hd[64].cpu().numpy().view(capi.pick_hit_dtype)["mesh"] != NONE).sum())

    # (b) one marquee over 1/256, 1/16 and all of the grid
    whole = (0.0, 0.0, (S - 1) * pitch + float(ext[0]), (S - 1) * pitch + float(ext[1]))
    inst_box = np.stack([(cell % S) * pitch, (cell // S) * pitch, (cell % S) * pitch + ext[0], (cell // S) * pitch + ext[1]], axis=1)
    calls, marquees = {}, {}
    for part, side in (("256th", 1 / 16.0), ("16th", 1 / 4.0), ("all", 1.0)):
        w, h = whole[2] * side, whole[3] * side
        x0, y0 = (whole[2] - w) * 0.37, (whole[3] - h) * 0.41
        r = (x0 - 1.0, y0 - 1.0, x0 + w + 1.0, y0 + h + 1.0) if side == 1.0 else (x0, y0, x0 + w, y0 + h)
        marquees[part] = r
        for mode, fl in (("crossing_mesh", 0), ("window_mesh", capi.PICK_RECT_WINDOW), ("crossing_draw", capi.PICK_RECT_BY_DRAW),
                         ("window_draw", capi.PICK_RECT_WINDOW | capi.PICK_RECT_BY_DRAW)):
            name = "marquee_%s_%s" % (part, mode)
            calls[name] = rect_call(name, up(rects([r], fl)), 1)
    alternate(calls)
    torch.cuda.synchronize()
    wrong = 0
    for name in calls:
        res[name + "_count"] = int(last[name].count.cpu().numpy().view(np.uint32)[0])
    for part, r in marquees.items():
        F = np.float32
        b = inst_box.astype(F)
        meets = (F(r[2]) >= b[:, 0]) & (F(r[0]) <= b[:, 2]) & (F(r[3]) >= b[:, 1]) & (F(r[1]) <= b[:, 3])
        within = (b[:, 0] >= F(r[0])) & (b[:, 2] <= F(r[2])) & (b[:, 1] >= F(r[1])) & (b[:, 3] <= F(r[3]))
        # an instance wholly inside is selected either way; one that is crossed is at most one whose box meets the rectangle
        wrong += not (int(within.sum()) <= res["marquee_%s_window_draw_count" % part] <= res["marquee_%s_crossing_draw_count" % part] <= int(meets.sum()))
        res["marquee_%s_instance_boxes_inside" % part], res["marquee_%s_instance_boxes_met" % part] = int(within.sum()), int(meets.sum())
    res["marquee_counts_outside_the_box_bounds"] = wrong
    del out, mb

    # (c) the stack
    N = args.stacked
    inst = np.zeros(N, dtype=capi.cache_instance_dtype)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:] = [1.0, 0.0, 0.0, 1.0, 100.0, 50.0]
    out, sdesc = submit(inst)
    smb = rt.mesh_bounds(ctx, out.pos, out.meshes, cache.nm * N)
    # a position inside the drawing that hits it: the first of a few random ones (vgx_pick decides, before any clock runs)
    cand = np.zeros(64, dtype=capi.pick_query_dtype)
    cand["x"], cand["y"], cand["mesh_end"] = 100.0 + lo[0] + rs.uniform(0.3, 0.7, 64) * ext[0], 50.0 + lo[1] + rs.uniform(0.3, 0.7, 64) * ext[1], NONE
    found = rt.pick(ctx, sdesc, up(cand), 64, smb, hd[64]).cpu().numpy().view(capi.pick_hit_dtype)["mesh"] != NONE
    sp = cand[np.nonzero(found)[0][:1]]
    assert sp.shape[0] == 1, "no position of the stack hits"
    x, y = float(sp["x"][0]), float(sp["y"][0])
    spd = up(sp)
    calls = {"stacked_point_pick": lambda: rt.pick(ctx, sdesc, spd, 1, smb, hd[1]),
             "stacked_point_rect": rect_call("stacked_point_rect", up(rects([(sp["x"][0], sp["y"][0], sp["x"][0], sp["y"][0])])), 1, sdesc, smb),
             "stacked_square_rect": rect_call("stacked_square_rect", up(rects([(x - 2, y - 2, x + 2, y + 2)], capi.PICK_RECT_BY_DRAW)), 1, sdesc, smb),
             "stacked_all_window_draw": rect_call("stacked_all_window_draw", up(rects([(100.0 + lo[0] - 1, 50.0 + lo[1] - 1, 100.0 + hi[0] + 1, 50.0 + hi[1] + 1)],
                                                                                    capi.PICK_RECT_BY_DRAW | capi.PICK_RECT_WINDOW)), 1, sdesc, smb)}
    alternate(calls)
    torch.cuda.synchronize()
    for name in ("stacked_point_rect", "stacked_square_rect", "stacked_all_window_draw"):
        res[name + "_count"] = int(last[name].count.cpu().numpy().view(np.uint32)[0])
    res["stacked_point_rect_over_pick"] = res["stacked_point_rect_ms_median"] / res["stacked_point_pick_ms_median"]
    res["stacked_point_same_words_as_vgx_pick"] = bool(np.array_equal(last["stacked_point_rect"].top.cpu().numpy()[:16], hd[1].cpu().numpy()))
    res["stacked_all_selects_every_copy"] = res["stacked_all_window_draw_count"] == N
    ctx.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
