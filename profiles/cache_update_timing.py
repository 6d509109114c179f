"""Incremental update of a submitted frame, one job on one box, warmed up, the variants alternating. A 100 x 100 grid of cached Tigers
(10 000 drawings, the benchmark's size), once as one instance per DRAWING (10 000 instances of 435 meshes) and once as one instance per
DRAW (2.4 M instances of 1-3 meshes). For each shape, in one alternating loop:
  submit          vgx_cache_submit of all instances: what showing an edit cost before (that code is unchanged)
  submit_bounds   the same + vgx_mesh_bounds over the whole frame: what keeping vgx_pick's boxes current cost before
  layout          vgx_cache_layout alone
  update_K[_b]    vgx_cache_update of K listed instances (per drawing: 1, 100, all; per draw: 1 000, 240 000, all), without and with
                  (_b) frame->mesh_bounds. The list is a seeded random choice without repetition, unsorted.
Every sample is a host clock around `call(s); synchronise`; buffers, lists and scratch exist before the clock starts. Beside each update:
the vertices and meshes it rewrote, the bytes that makes (8 read + 8 written per vertex, 4 more per vertex of a mesh that takes the
instance's colour, 32 read + 16 written per mesh with boxes; the boxes' second read of the cached positions stays in L2 and is not
counted) and the TB/s this gives, next to a plain device-to-device copy of 1 GiB timed in the same job.

python profiles/cache_update_timing.py [--rounds R] [--drawings-side S] [--out FILE]   (prints one JSON object)"""
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

    ctx = rt.Context(0)
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    sizes = rt.tessellate_count(ctx, pset, dd, d.shape[0])
    cbufs = rt.MeshBuffers(dev, sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"])
    rt.tessellate_emit(ctx, pset, dd, d.shape[0], cbufs)
    cache = rt.MeshCache(ctx, cbufs, sizes, dd, d.shape[0])
    torch.cuda.synchronize()
    pset.close()
    box = cache.bounds.cpu().numpy()
    lo, hi = box[:, :2].min(axis=0), box[:, 2:].max(axis=0)
    pitch = 1.25 * float(max(hi - lo))
    meshes = cache.bufs.meshes[:cache.nm * 32].cpu().numpy().view(capi.mesh_dtype)
    draw_first = np.flatnonzero(np.r_[True, meshes["draw"][1:] != meshes["draw"][:-1]])
    draw_count = np.diff(np.r_[draw_first, cache.nm])
    first_vertex = np.r_[meshes["first_vertex"].astype(np.int64), cache.nv]
    uniform = np.isin(meshes["subpath_kind"] >> 28, (capi.MESH_FILL, capi.MESH_STROKE))
    uni_prefix = np.r_[0, np.cumsum(np.where(uniform, meshes["num_vertices"], 0).astype(np.int64))]
    res["cache_meshes"], res["cache_vertices"], res["cache_draw_ranges"] = cache.nm, cache.nv, int(draw_first.shape[0])

    def instances(per_draw, moved):
        k = draw_first.shape[0] if per_draw else 1
        inst = np.zeros(S * S * k, dtype=capi.cache_instance_dtype)
        cell = np.repeat(np.arange(S * S), k)
        inst["first_mesh"] = np.tile(draw_first, S * S) if per_draw else 0
        inst["num_meshes"] = np.tile(draw_count, S * S) if per_draw else cache.nm
        inst["color"] = 0xFF00FF00 if moved else 0xFFFFFFFF
        inst["mtx"][:, 0] = inst["mtx"][:, 3] = 1.0
        inst["mtx"][:, 4] = (cell % S) * pitch - lo[0] + (3.5 if moved else 0.0)
        inst["mtx"][:, 5] = (cell // S) * pitch - lo[1] + (1.25 if moved else 0.0)
        return inst

    nv_all, ni_all, nm_all = cache.nv * S * S, cache.ni * S * S, cache.nm * S * S
    out = rt.MeshBuffers(dev, nv_all, ni_all, nm_all)
    bounds = torch.empty((nm_all, 4), dtype=torch.float32, device=dev)
    # the ruler: a plain copy
    a1 = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    a2 = torch.empty_like(a1)
    for _ in range(3):
        a2.copy_(a1)
    v = sorted(sample(lambda: a2.copy_(a1)) for _ in range(args.rounds))
    res["copy_ms_median"], res["copy_TBps"] = v[len(v) // 2], 2 * a1.numel() * 4 / v[len(v) // 2] / 1e9
    del a1, a2

    def bounds_into(table):
        st = rt.lib().vgx_mesh_bounds(ctx.handle, out.pos.data_ptr(), out.meshes.data_ptr(), nm_all, table.data_ptr(), rt._stream_ptr())
        assert st == 0

    for shape, counts in (("per_drawing", (1, 100, None)), ("per_draw", (1000, 240000, None))):
        inst0, inst1 = instances(shape == "per_draw", False), instances(shape == "per_draw", True)
        n = inst0.shape[0]
        src0, src1 = up(inst0), up(inst1)
        slots, lstat = rt.cache_layout(ctx, cache, src0, n)
        rt.cache_submit(ctx, cache, src0, n, out)
        bounds_into(bounds)
        torch.cuda.synchronize()
        assert int(lstat.item()) == 0 and int(out.dev_status.item()) == 0
        a, k = inst0["first_mesh"].astype(np.int64), inst0["num_meshes"].astype(np.int64)
        inst_vertices = first_vertex[a + k] - first_vertex[a]
        inst_uniform = uni_prefix[a + k] - uni_prefix[a]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        perm = np.random.RandomState(11).permutation(n).astype(np.uint32)
        calls = {"submit": lambda: rt.cache_submit(ctx, cache, src0, n, out),
                 "submit_bounds": lambda: (rt.cache_submit(ctx, cache, src0, n, out), bounds_into(bounds)),
                 "layout": lambda: rt.cache_layout(ctx, cache, src0, n, slots_dev=slots)}
        moved = {}

        def updater(dirty_dev, nd, with_bounds):
            def run():
                rt.cache_update(ctx, cache, src1, n, slots, dirty_dev, nd, out.pos, out.color, nv_all, nm_all,
                                mesh_bounds=bounds if with_bounds else None, dev_status=status)
            return run
        keep = []
        for cnt in counts:
            lst = perm[:cnt] if cnt else perm
            nd = int(lst.shape[0])
            dirty_dev = up(lst)
            keep.append(dirty_dev)
            li = lst.astype(np.int64)
            for wb in (False, True):
                name = "update_%s%s" % ("all" if cnt is None else cnt, "_b" if wb else "")
                calls[name] = updater(dirty_dev, nd, wb)
                V, Vu, M = int(inst_vertices[li].sum()), int(inst_uniform[li].sum()), int(k[li].sum())
                moved[name] = (nd, V, M, 16 * V + 4 * Vu + (48 * M if wb else 0))
        names = sorted(calls)
        for _ in range(2):
            for nm in names:
                calls[nm]()
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and int(out.dev_status.item()) == 0
        t = {nm: [] for nm in names}
        for r in range(args.rounds):
            for nm in names[r % len(names):] + names[:r % len(names)]:
                t[nm].append(sample(calls[nm]))
        res[shape + "_instances"] = n
        for nm in names:
            stats("%s_%s" % (shape, nm), t[nm])
        for nm, (nd, V, M, nbytes) in moved.items():
            ms = res["%s_%s_ms_median" % (shape, nm)]
            key = "%s_%s" % (shape, nm)
            res[key + "_listed"], res[key + "_vertices"], res[key + "_meshes"], res[key + "_bytes"] = nd, V, M, nbytes
            res[key + "_bytes_per_vertex"] = nbytes / max(V, 1)
            res[key + "_TBps"] = nbytes / ms / 1e9
            res[key + "_vs_copy"] = res[key + "_TBps"] / res["copy_TBps"]
            base = "submit_bounds" if nm.endswith("_b") else "submit"
            res[key + "_over_" + base] = ms / res["%s_%s_ms_median" % (shape, base)]
        # spot check: the frame and the boxes after an all-instances update == a fresh submit + vgx_mesh_bounds of the edited array
        calls["update_all_b"]()
        torch.cuda.synchronize()
        pos_u, col_u, box_u = out.pos.clone(), out.color.clone(), bounds.clone()
        rt.cache_submit(ctx, cache, src1, n, out)
        bounds_into(bounds)
        torch.cuda.synchronize()
        res[shape + "_update_all_equals_fresh_submit"] = bool(torch.equal(pos_u.view(torch.int32), out.pos.view(torch.int32)) and torch.equal(col_u, out.color)
                                                              and torch.equal(box_u.view(torch.int32), bounds.view(torch.int32)))
        del pos_u, col_u, box_u, src0, src1, slots, keep
    ctx.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
