"""vgx_raster, one job on one box, warmed up, the variants alternating; host clock around `call; synchronise`, buffers and scratch sized
before the clock starts (vgx_raster_reserve, and one untimed call that checks dev_status).
  tiger1_*    ONE Tiger (vgx_tessellate's frame, scaled to fill the image) into 1024 x 1024 and 4096 x 4096
  grid_*      a 100 x 100 grid of cached Tigers submitted whole (4.35 M meshes), scaled so that the grid fills the image, into the same
              two targets; with the caller's boxes (vgx_mesh_bounds taken once) and with NULL (the call computes them)
Beside each the two rulers: a kernel that only STORES the image (a fill of width x height words: what the last pass cannot beat) and a
plain device-to-device copy (1 GiB, as TB/s, and the time it would need for the bytes the call must read: the four streams of the
frame and the boxes). The two costs to look at first are the binning sort (rocprim radix sort over the bin entries) and the per-pixel
loop of k_raster_tiles; `--trace-only` runs the grid into 4096 x 4096 a few times and nothing else: the program of a
rocprofv3 --kernel-trace --stats run, which splits the call into its kernels.

python profiles/raster_timing.py [--rounds R] [--drawings-side S] [--out profiles/raster_timing.json]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1024, 4096)
CLEAR = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--drawings-side", type=int, default=100)
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
    extent = float(max(hi - lo))
    pitch = 1.25 * extent
    res["cache_meshes"], res["cache_vertices"], res["cache_indices"] = cache.nm, cache.nv, cache.ni

    def submit(inst):
        n = inst.shape[0]
        out = rt.MeshBuffers(dev, cache.nv * n, cache.ni * n, cache.nm * n)
        rt.cache_submit(ctx, cache, up(inst), n, out)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        return out, capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), cache.nm * n, cache.nv * n, cache.ni * n)

    def frame(side, size):
        """side x side drawings scaled so that the grid fills a size x size image."""
        s = size / (side * pitch)
        inst = np.zeros(side * side, dtype=capi.cache_instance_dtype)
        cell = np.arange(side * side)
        inst["num_meshes"], inst["color"] = cache.nm, 0xC0FFFFFF
        inst["mtx"][:, 0] = inst["mtx"][:, 3] = s
        inst["mtx"][:, 4], inst["mtx"][:, 5] = ((cell % side) * pitch - lo[0]) * s, ((cell // side) * pitch - lo[1]) * s
        return submit(inst)

    def prepared(out, desc, size, mb):
        """The image, the status word, the scratch: one untimed call that must end with VGX_OK."""
        img = torch.zeros((size, size), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(3):
            rt.raster(ctx, desc, size, size, clear_color=CLEAR, bounds_dev=mb, image=img, dev_status=status)
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return img, status
        raise RuntimeError("vgx_raster did not reach VGX_OK: %d" % int(status.item()))

    a1 = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    a2 = torch.empty_like(a1)
    for _ in range(3):
        a2.copy_(a1)
    v = sorted(sample(lambda: a2.copy_(a1)) for _ in range(args.rounds))
    res["copy_ms_median"], res["copy_TBps"] = v[len(v) // 2], 2 * a1.numel() * 4 / v[len(v) // 2] / 1e9
    del a1, a2

    for side, tag in ((1, "tiger1"), (S, "grid")):
        for size in SIZES:
            if args.trace_only and not (tag == "grid" and size == SIZES[-1]):
                continue
            out, desc = frame(side, size)
            nm = cache.nm * side * side
            mb = rt.mesh_bounds(ctx, out.pos, out.meshes, nm)
            img, status = prepared(out, desc, size, None)
            prepared(out, desc, size, mb)
            if args.trace_only:
                for _ in range(8):
                    rt.raster(ctx, desc, size, size, clear_color=CLEAR, bounds_dev=None, image=img, dev_status=status)
                torch.cuda.synchronize()
                continue
            name = "%s_%d" % (tag, size)
            alternate({name + "_boxes": lambda: rt.raster(ctx, desc, size, size, clear_color=CLEAR, bounds_dev=mb, image=img, dev_status=status),
                       name + "_null": lambda: rt.raster(ctx, desc, size, size, clear_color=CLEAR, bounds_dev=None, image=img, dev_status=status),
                       name + "_store_only": lambda: img.fill_(-1),
                       name + "_mesh_bounds": lambda: rt.mesh_bounds(ctx, out.pos, out.meshes, nm)})
            rt.raster(ctx, desc, size, size, clear_color=CLEAR, bounds_dev=mb, image=img, dev_status=status)
            torch.cuda.synchronize()
            res[name + "_status"] = int(status.item())
            res[name + "_pixels_painted"] = int((img != -1).sum().item())
            res[name + "_read_bytes"] = cache.nv * side * side * 12 + cache.ni * side * side * 2 + nm * (32 + 16)
            res[name + "_read_copy_ms"] = res[name + "_read_bytes"] / res["copy_TBps"] / 1e9
            res[name + "_scratch_bytes"] = ctx.scratch_bytes()
            del out, mb, img
    ctx.close()
    if args.trace_only:
        return
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
