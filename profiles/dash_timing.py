"""vgx_dash on the device's clock, one job on one box.

  walks_*     (a) workloads.random_walk_polylines() at its default size (10 000 x 1 000 segments) under [12,6]: ms per vgx_dash call
              (HIP events around K back-to-back calls after warm-up, median of 5 such runs), output vertices, ns per output vertex,
              and (bytes read + bytes written) / time. Bytes from the shapes: 8 per input vertex and 16 per input sub-path record read,
              8 per output vertex and 16 + 4 + 4 per piece written (the scratch traffic -- 16 bytes per segment written once and
              searched -- is NOT counted: the figure is what the caller's buffers see).
  skew_*      (b) 1 000 two-vertex lists of 100 000 units under [1,1]: 50 M pieces out of 1 000 segments. The same figures.
              skew_vs_walks_ns_per_vertex: a large ratio would mean work is still distributed by input segment.
  *_stroke_ms (c) vgx_stroke_count + vgx_stroke_emit on the same pieces (Butt caps, Miter joins, AA), and the dash pass as a share of it.
  writebw_*   (d) profiles/micro/writebw.hip's figures from this job: the pure-store ceiling the byte rates are judged against.

python profiles/dash_timing.py [--steps K] [--out FILE]   (prints one JSON object)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skew-lists", type=int, default=1000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from text_timing import writebw
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    K = max(args.steps, 5)
    dev = torch.device("cuda", 0)
    res = {"box": torch.cuda.get_device_name(0), "steps": K}

    def timed(fn, k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    def median(fn, k, runs=5):
        return sorted(timed(fn, k) for _ in range(runs))[runs // 2]

    res.update({"writebw_" + k: v for k, v in writebw().items()})
    ceiling = max(v for k, v in res.items() if k.startswith("writebw_write3_mis0"))
    res["writebw_ceiling_TBps"] = ceiling

    ctx = rt.Context(0)
    L = rt.lib()

    def leg(name, poly, subs, pattern):
        nl = subs.shape[0]
        npoly = poly.shape[0]
        dashes = np.zeros(1, capi.dash_dtype)
        dashes["count"] = len(pattern)
        p_dev = torch.from_numpy(poly).to(dev)
        s_dev = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
        sd_dev = torch.zeros(nl, dtype=torch.int32, device=dev)
        d_dev = torch.from_numpy(dashes.view(np.uint8).copy()).to(dev)
        pat_dev = torch.tensor(pattern, dtype=torch.float32, device=dev)
        z = rt.dash_count(ctx, p_dev, s_dev, sd_dev, nl, d_dev, 1, pat_dev, len(pattern))
        nv, ns = z["num_poly_vertices"], z["num_subpaths"]
        bufs = rt.DashBuffers(dev, nv, ns)
        call = lambda: rt.dash_async(ctx, p_dev, s_dev, sd_dev, nl, d_dev, 1, pat_dev, len(pattern), bufs)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        assert int(bufs.dev_status.item()) == 0, int(bufs.dev_status.item())
        ms = median(call, K)
        moved = 8 * npoly + 16 * nl + 8 * nv + 24 * ns
        res[name + "_lists"], res[name + "_input_vertices"], res[name + "_pieces"], res[name + "_output_vertices"] = nl, npoly, ns, nv
        res[name + "_dash_ms"] = ms
        res[name + "_ns_per_output_vertex"] = ms * 1e6 / nv
        res[name + "_bytes"] = moved
        res[name + "_TBps"] = moved / ms / 1e9
        res[name + "_vs_writebw"] = moved / ms / 1e9 / ceiling
        # the stroke the pieces feed
        draws = wl.make_draws(1)
        wl.set_stroke(draws, 0, 0xFF2080FF, 3.0, capi.CAP_BUTT, capi.JOIN_MITER, aa=True)
        dd = rt.upload_draws(draws)
        sizes = capi.Sizes()
        s = rt._stream_ptr()
        rt._check(L.vgx_stroke_count(ctx.handle, bufs.poly.data_ptr(), bufs.subs.data_ptr(), bufs.sub_draw.data_ptr(), ns, dd.data_ptr(), 1, C.byref(sizes), s), "vgx_stroke_count")
        mb = rt.MeshBuffers(dev, int(sizes.num_vertices), int(sizes.num_indices), int(sizes.num_meshes))
        out = mb.out_struct()

        def stroke():
            rt._check(L.vgx_stroke_count(ctx.handle, bufs.poly.data_ptr(), bufs.subs.data_ptr(), bufs.sub_draw.data_ptr(), ns, dd.data_ptr(), 1, C.byref(sizes), s), "vgx_stroke_count")
            rt._check(L.vgx_stroke_emit(ctx.handle, bufs.poly.data_ptr(), bufs.subs.data_ptr(), bufs.sub_draw.data_ptr(), ns, dd.data_ptr(), 1, C.byref(out), s), "vgx_stroke_emit")
        for _ in range(2):
            stroke()
        sms = median(stroke, max(K // 2, 3), runs=3)
        res[name + "_stroke_ms"] = sms
        res[name + "_stroke_mesh_vertices"] = int(sizes.num_vertices)
        res[name + "_dash_share_of_stroke"] = ms / sms
        del mb, bufs

    n, nseg = 10000, 1000
    ps, _ = wl.random_walk_polylines(n=n, nseg=nseg)
    poly = np.asarray(ps.args, dtype=np.float32).reshape(-1, 2).copy()
    subs = np.zeros(n, capi.subpath_dtype)
    subs["num_vertices"] = nseg + 1
    subs["first_vertex"] = np.arange(n, dtype=np.uint64) * (nseg + 1)
    leg("walks", poly, subs, [12.0, 6.0])

    m = args.skew_lists
    poly = np.zeros((2 * m, 2), np.float32)
    poly[:, 1] = np.repeat(np.arange(m), 2) * 10.0
    poly[1::2, 0] = 100000.0
    subs = np.zeros(m, capi.subpath_dtype)
    subs["num_vertices"] = 2
    subs["first_vertex"] = np.arange(m, dtype=np.uint64) * 2
    leg("skew", poly, subs, [1.0, 1.0])
    res["skew_vs_walks_ns_per_vertex"] = res["skew_ns_per_output_vertex"] / res["walks_ns_per_output_vertex"]

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
