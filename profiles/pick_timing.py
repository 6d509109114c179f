"""vgx_pick, one job on one box, warmed up, the variants alternating; host clock around `call; synchronise`, buffers and scratch sized
before the clock starts.
  grid_*      a 100 x 100 grid of cached Tigers submitted whole (one instance per drawing: 4.35 M meshes), 1 / 16 / 256 cursor positions
              spread over the grid, with the caller's boxes (vgx_mesh_bounds taken once) and with NULL (the call computes them)
  stacked_*   1 000 Tigers under ONE transform, 1 and 256 positions inside the drawing: every copy's meshes are candidates, the
              triangle stage reads whole index and position streams
  frame316_*  a 316-draw frame written by vgx_tessellate, one position
Beside each the two rulers of the other timing files: a plain device-to-device copy (1 GiB, as TB/s, and the time it would need for the
bytes the stage reads) and vgx_mesh_bounds over the same frame. The answers at full size are checked on a sample: the hit drawing is
downloaded and searched on the host with the rule of include/vgx.h (the grid's drawings do not overlap, so its answer is the frame's).
`--trace-only` runs the 256-position grid pick a few times and nothing else: the program of the rocprofv3 --kernel-trace --stats run.
`--stats-db DB --out FILE` adds the kernels' shares of that run to FILE.

python profiles/pick_timing.py [--rounds R] [--drawings-side S] [--stacked N] [--out FILE]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF


def host_pick(np, pos, idx, meshes, x, y):
    """The rule of include/vgx.h over one downloaded range of meshes: (mesh within the range, triangle) or None."""
    best = None
    F, D = np.float32, np.float64
    for m in range(meshes.shape[0]):
        fv, fi, nv, ni = (int(meshes[k][m]) for k in ("first_vertex", "first_index", "num_vertices", "num_indices"))
        tri = idx[fi:fi + ni // 3 * 3].reshape(-1, 3).astype(np.int64)
        ok = (tri < nv).all(axis=1)
        p = pos[fv:fv + nv]
        t = np.where(ok[:, None], tri, 0)
        a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        box = ok & (F(x) >= lo[:, 0]) & (F(x) <= hi[:, 0]) & (F(y) >= lo[:, 1]) & (F(y) <= hi[:, 1])
        a, b, c, px, py = a.astype(D), b.astype(D), c.astype(D), D(F(x)), D(F(y))
        A = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        e0 = (b[:, 0] - a[:, 0]) * (py - a[:, 1]) - (b[:, 1] - a[:, 1]) * (px - a[:, 0])
        e1 = (c[:, 0] - b[:, 0]) * (py - b[:, 1]) - (c[:, 1] - b[:, 1]) * (px - b[:, 0])
        e2 = (a[:, 0] - c[:, 0]) * (py - c[:, 1]) - (a[:, 1] - c[:, 1]) * (px - c[:, 0])
        hit = box & (((A > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((A < 0) & (e0 <= 0) & (e1 <= 0) & (e2 <= 0)))
        w = np.nonzero(hit)[0]
        if w.size:
            best = (m, int(w[-1]))
    return best


def kernel_key(name):
    """k_pick_tris, k_scan_apply<OpPickCand>, ... from rocprofv3's demangled names."""
    import re
    k = re.search(r"k_\w+", name).group(0)
    op = re.search(r"Op\w+", name)
    return k + ("<%s>" % op.group(0) if op else "")


def add_stats(db, out):
    import sqlite3
    rows = sqlite3.connect(db).cursor().execute("select name,total_calls,total_duration,average from top_kernels").fetchall()
    mine = [r for r in rows if "k_pick_" in r[0] or "OpPickCand" in r[0] or "k_bounds_" in r[0]]
    with open(out) as f:
        res = json.loads(f.read())
    res["trace_grid_q256_null_boxes"] = trace_record([(kernel_key(r[0]), r[1], r[3]) for r in mine])
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res["trace_grid_q256_null_boxes"]))


def trace_record(rows):
    """rows: (kernel, calls, average us). Per call of vgx_pick: every kernel's average time and its share of their sum."""
    avg = {k: a for k, _, a in rows}
    total = sum(avg.values())
    pick = sum(a for k, a in avg.items() if "k_bounds_" not in k)
    return {"avg_us": avg, "share_of_the_call": {k: a / total for k, a in avg.items()}, "sum_us": total, "sum_without_the_box_pass_us": pick,
            "k_pick_tris_share_of_the_call": avg.get("k_pick_tris", 0.0) / total, "k_pick_tris_share_without_the_box_pass": avg.get("k_pick_tris", 0.0) / pick}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--drawings-side", type=int, default=100)
    ap.add_argument("--stacked", type=int, default=1000)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--stats-db", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats_db:
        return add_stats(args.stats_db, args.out)
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
    pitch = 1.25 * float(max(hi - lo))
    res["cache_meshes"], res["cache_vertices"], res["cache_indices"] = cache.nm, cache.nv, cache.ni

    def submit(inst):
        n = inst.shape[0]
        out = rt.MeshBuffers(dev, cache.nv * n, cache.ni * n, cache.nm * n)
        rt.cache_submit(ctx, cache, up(inst), n, out)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        return out, capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), cache.nm * n, cache.nv * n, cache.ni * n)

    def queries(pts):
        q = np.zeros(len(pts), dtype=capi.pick_query_dtype)
        q["x"], q["y"], q["mesh_end"] = [p[0] for p in pts], [p[1] for p in pts], NONE
        return q

    def check(out, desc, inst, q, hits, cells):
        """The sample: the answer inside the query's own drawing, searched on the host."""
        bad = 0
        for k, cell in cells:
            a = cell * cache.nm
            meshes = out.meshes[a * 32:(a + cache.nm) * 32].cpu().numpy().view(capi.mesh_dtype).copy()
            v0, i0 = int(meshes["first_vertex"][0]), int(meshes["first_index"][0])
            pos = out.pos[v0:v0 + cache.nv].cpu().numpy()
            idx = out.idx[i0:i0 + cache.ni].cpu().numpy().view(np.uint16)
            meshes["first_vertex"] -= v0
            meshes["first_index"] -= i0
            want = host_pick(np, pos, idx, meshes, q["x"][k], q["y"][k])
            got = None if hits["mesh"][k] == NONE else (int(hits["mesh"][k]) - a, int(hits["triangle"][k]))
            bad += want != got
        return bad

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
    nm_all, nv_all, ni_all = cache.nm * S * S, cache.nv * S * S, cache.ni * S * S
    rs = np.random.RandomState(4)
    # cursor positions: in the middle region of a random drawing each
    qcell = rs.randint(0, S * S, 256)
    pts = [((c % S) * pitch + rs.uniform(0.3, 0.7) * (hi[0] - lo[0]), (c // S) * pitch + rs.uniform(0.3, 0.7) * (hi[1] - lo[1])) for c in qcell]
    q = queries(pts)
    mb = rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)
    qd = {n: up(q[:n]) for n in (1, 16, 256)}
    hd = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 256)}
    if args.trace_only:
        for _ in range(8):
            rt.pick(ctx, desc, qd[256], 256, None, hd[256])
        torch.cuda.synchronize()
        ctx.close()
        return
    calls = {}
    for n in (1, 16, 256):
        calls["grid_q%d_boxes" % n] = (lambda n=n: rt.pick(ctx, desc, qd[n], n, mb, hd[n]))
        calls["grid_q%d_null" % n] = (lambda n=n: rt.pick(ctx, desc, qd[n], n, None, hd[n]))
    calls["grid_mesh_bounds"] = lambda: rt.mesh_bounds(ctx, out.pos, out.meshes, nm_all)
    alternate(calls)
    hits = hd[256].cpu().numpy().view(capi.pick_hit_dtype)
    res["grid_meshes"], res["grid_vertices"], res["grid_indices"] = nm_all, nv_all, ni_all
    res["grid_q256_hits"] = int((hits["mesh"] != NONE).sum())
    res["grid_sample_checked"], res["grid_sample_wrong"] = 8, check(out, desc, inst, q, hits, [(k, int(qcell[k])) for k in range(8)])
    res["grid_draw_is_the_instance"] = bool(np.all(hits["draw"][hits["mesh"] != NONE] == qcell[hits["mesh"] != NONE]))
    rt.pick(ctx, desc, qd[256], 256, mb, hd[256])
    torch.cuda.synchronize()
    res["grid_boxes_equal_null"] = bool(np.array_equal(hd[256].cpu().numpy(), hits.view(np.uint8)))
    res["grid_box_stage_bytes"] = nm_all * (16 + 32 + 4 + 4)  # box, mesh record, candidate count out, and in again by the scan
    res["grid_box_stage_copy_ms"] = res["grid_box_stage_bytes"] / res["copy_TBps"] / 1e9
    del out, mb

    # ---- the stack -----------------------------------------------------------------------------------------------------
    N = args.stacked
    inst = np.zeros(N, dtype=capi.cache_instance_dtype)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:] = [1.0, 0.0, 0.0, 1.0, 100.0, 50.0]
    out, desc = submit(inst)
    pts = [(100.0 + lo[0] + rs.uniform(0.3, 0.7) * (hi[0] - lo[0]), 50.0 + lo[1] + rs.uniform(0.3, 0.7) * (hi[1] - lo[1])) for _ in range(256)]
    q = queries(pts)
    mb = rt.mesh_bounds(ctx, out.pos, out.meshes, cache.nm * N)
    qd = {n: up(q[:n]) for n in (1, 256)}
    calls = {}
    for n in (1, 256):
        calls["stacked_q%d_boxes" % n] = (lambda n=n: rt.pick(ctx, desc, qd[n], n, mb, hd[n]))
    calls["stacked_mesh_bounds"] = lambda: rt.mesh_bounds(ctx, out.pos, out.meshes, cache.nm * N)
    alternate(calls)
    hits = hd[256].cpu().numpy().view(capi.pick_hit_dtype)
    res["stacked_q256_hits"] = int((hits["mesh"] != NONE).sum())
    res["stacked_hits_in_the_top_copy"] = bool(np.all(hits["draw"][hits["mesh"] != NONE] == N - 1))
    res["stacked_sample_checked"], res["stacked_sample_wrong"] = 8, check(out, desc, inst, q, hits, [(k, N - 1) for k in range(8)])
    res["stacked_stream_bytes"] = cache.ni * N * 2 + cache.nv * N * 8 + cache.nm * N * (16 + 32 + 4 + 4 + 32)
    res["stacked_stream_copy_ms"] = res["stacked_stream_bytes"] / res["copy_TBps"] / 1e9
    del out, mb

    # ---- a 316-draw frame ------------------------------------------------------------------------------------------------
    fps, fd = wl.tiger(2)
    fd = fd[:316]
    fset = rt.PathSet(ctx, fps)
    dfr = rt.upload_draws(fd)
    sz = rt.tessellate_count(ctx, fset, dfr, 316)
    fb = rt.MeshBuffers(dev, sz["num_vertices"], sz["num_indices"], sz["num_meshes"])
    rt.tessellate_emit(ctx, fset, dfr, 316, fb)
    torch.cuda.synchronize()
    fdesc = capi.CacheDesc(fb.pos.data_ptr(), fb.color.data_ptr(), fb.idx.data_ptr(), fb.meshes.data_ptr(), sz["num_meshes"], sz["num_vertices"], sz["num_indices"])
    fpos = fb.pos[:sz["num_vertices"]].cpu().numpy()
    q = queries([tuple(fpos[sz["num_vertices"] // 2])])
    q1 = up(q)
    fmb = rt.mesh_bounds(ctx, fb.pos, fb.meshes, sz["num_meshes"])
    alternate({"frame316_q1_boxes": lambda: rt.pick(ctx, fdesc, q1, 1, fmb, hd[1]), "frame316_q1_null": lambda: rt.pick(ctx, fdesc, q1, 1, None, hd[1]),
               "frame316_mesh_bounds": lambda: rt.mesh_bounds(ctx, fb.pos, fb.meshes, sz["num_meshes"])})
    h = hd[1].cpu().numpy().view(capi.pick_hit_dtype)[0]
    fm = fb.meshes[:sz["num_meshes"] * 32].cpu().numpy().view(capi.mesh_dtype)
    res["frame316_meshes"], res["frame316_vertices"] = sz["num_meshes"], sz["num_vertices"]
    want = host_pick(np, fpos, fb.idx[:sz["num_indices"]].cpu().numpy().view(np.uint16), fm, q["x"][0], q["y"][0])
    res["frame316_matches_host"] = bool(want == (None if h["mesh"] == NONE else (int(h["mesh"]), int(h["triangle"]))))
    fset.close()
    ctx.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
