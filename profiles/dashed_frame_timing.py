"""A frame with dashed strokes three ways, one job on one box, warmed up, the variants alternating:
  (a) vgx_tessellate_dashed: the one asynchronous call;
  (b) the composed chain of the entries that existed before it, for the same frame, its host round trips included:
      vgx_tessellate_immediate with the dashed draws' strokes off -> read its totals | vgx_flatten -> vgx_subpath_draws -> vgx_dash ->
      vgx_stroke_count (waits for the stream, reads the totals) -> vgx_stroke_emit | vgx_merge (copies every stream of the frame once more);
  (c) vgx_tessellate_immediate on the same draws undashed (what the frame costs without dashes: other, fewer meshes).
Every sample is a host clock around `call; synchronise` (the chain's round trips are part of what is measured, so device events around
back-to-back calls would not see them). Buffers and scratch are sized before the clock starts; all three run to VGX_OK.
Workloads: Tiger x1 (one recorded frame, 240 draws) and Tiger x1000 (240 000 draws), every stroked draw dashed [12,6].
Reports per workload the median, minimum and maximum of each variant over the repeated rounds, and the ratios (a)/(b) and (a)/(c) of
the medians; "a_below_b_beyond_spread" says whether (a)'s slowest round is still faster than (b)'s fastest.

python profiles/dashed_frame_timing.py [--rounds R] [--out FILE]   (prints one JSON object)"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--instances", type=int, nargs="*", default=[1, 1000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    L = rt.lib()
    dev = torch.device("cuda", 0)
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "pattern": [12.0, 6.0]}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def sizes_of(t):
        z = t.cpu().numpy()
        return {k: int(z[i]) for i, (k, _) in enumerate(capi.Sizes._fields_)}

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for inst in args.instances:
        name = "tiger_x%d" % inst
        ps, d = wl.tiger(inst)
        n = d.shape[0]
        stroked = (d["stroke_flags"] & capi.STROKE_ENABLE) != 0
        dashes = np.zeros(n, capi.dash_dtype)
        dashes["count"][stroked] = 2
        pattern = np.array([12.0, 6.0], np.float32)
        ddash, dpat = up(dashes), torch.from_numpy(pattern).to(dev)
        dd = rt.upload_draws(d)
        # (a): its own context, run to VGX_OK once (sizes the buffers and the scratch)
        ctx_a = rt.Context(0)
        pset_a = rt.PathSet(ctx_a, ps)
        ra = rt.tessellate_dashed(ctx_a, pset_a, dd, n, ddash, dpat, 2, to_host=False)
        bufs_a = ra.bufs
        dds = torch.zeros(10, dtype=torch.int64, device=dev)

        def call_a():
            rt.tessellate_dashed_async(ctx_a, pset_a, dd, n, ddash, dpat, 2, bufs_a, dds)
        # (c)
        ctx_c = rt.Context(0)
        pset_c = rt.PathSet(ctx_c, ps)
        rc, bufs_c = rt.tessellate_grow(ctx_c, pset_c, dd, n, max_calls=4)

        def call_c():
            rt.tessellate_immediate(ctx_c, pset_c, dd, n, bufs_c)
        # (b): one context for the whole chain, as a caller would have
        ctx_b = rt.Context(0)
        pset_b = rt.PathSet(ctx_b, ps)
        da = d.copy()
        da["stroke_flags"][stroked] = 0
        sel = np.flatnonzero(stroked)
        ds = d[sel].copy()
        ds["fill_flags"] = 0
        dda, dds_b, ddash_b = rt.upload_draws(da), rt.upload_draws(ds), up(dashes[sel])
        ns = sel.shape[0]
        _, bufs_ba = rt.tessellate_grow(ctx_b, pset_b, dda, n, max_calls=4)
        fl = rt.flatten(ctx_b, pset_b, dds_b, ns, apply_transform=True, to_host=False, entry="two_phase")
        npoly, nsub = fl.sizes["num_poly_vertices"], fl.sizes["num_subpaths"]
        fbufs = rt.FlatBuffers(dev, npoly, nsub, ns)
        sd = torch.empty(max(nsub, 1), dtype=torch.int32, device=dev)
        zc = rt.dash_count(ctx_b, fl.poly_dev, fl.subs_dev, rt.subpath_draws(ctx_b, fl.dinfo_dev, ns, nsub), nsub, ddash_b, ns, dpat, 2)
        dbufs = rt.DashBuffers(dev, zc["num_poly_vertices"], zc["num_subpaths"])
        npieces = zc["num_subpaths"]
        bufs_bb = rt.MeshBuffers(dev, ra.sizes["num_vertices"], ra.sizes["num_indices"], npieces)
        bufs_bo = rt.MeshBuffers(dev, ra.sizes["num_vertices"], ra.sizes["num_indices"], ra.sizes["num_meshes"])
        s = rt._stream_ptr()
        sel_dev = torch.from_numpy(sel.astype(np.int32)).to(dev)

        def call_b():
            rt.tessellate_immediate(ctx_b, pset_b, dda, n, bufs_ba)
            rt.flatten_async(ctx_b, pset_b, dds_b, ns, fbufs, apply_transform=True)
            rt._check(L.vgx_subpath_draws(ctx_b.handle, fbufs.dinfo.data_ptr(), ns, sd.data_ptr(), nsub, s), "vgx_subpath_draws")
            rt.dash_async(ctx_b, fbufs.poly, fbufs.subs, sd, nsub, ddash_b, ns, dpat, 2, dbufs)
            zs = capi.Sizes()  # (round trip 1: the count waits for the stream and reads the totals)
            rt._check(L.vgx_stroke_count(ctx_b.handle, dbufs.poly.data_ptr(), dbufs.subs.data_ptr(), dbufs.sub_draw.data_ptr(), npieces, dds_b.data_ptr(), ns, C.byref(zs), s), "vgx_stroke_count")
            out = bufs_bb.out_struct()
            rt._check(L.vgx_stroke_emit(ctx_b.handle, dbufs.poly.data_ptr(), dbufs.subs.data_ptr(), dbufs.sub_draw.data_ptr(), npieces, dds_b.data_ptr(), ns, C.byref(out), s), "vgx_stroke_emit")
            za = sizes_of(bufs_ba.dev_sizes)  # (round trip 2: vgx_merge takes both sequences' totals as host values)
            rt.merge(ctx_b, rt.mesh_seq(bufs_ba, za["num_vertices"], za["num_indices"], za["num_meshes"]),
                     rt.mesh_seq(bufs_bb, int(zs.num_vertices), int(zs.num_indices), int(zs.num_meshes)),
                     sel_dev[dbufs.sub_draw[:npieces].long()], dd, n, bufs_bo)  # (the dash pass names the draw inside the restricted batch: one gather gives the frame draw)
        calls = {"a": call_a, "b": call_b, "c": call_c}
        for _ in range(3):
            for k in "abc":
                calls[k]()
        torch.cuda.synchronize()
        assert int(bufs_a.dev_status.item()) == 0 and int(bufs_c.dev_status.item()) == 0 and int(bufs_bo.dev_status.item()) == 0
        zb = sizes_of(bufs_bo.dev_sizes)
        assert (zb["num_vertices"], zb["num_indices"], zb["num_meshes"]) == (ra.sizes["num_vertices"], ra.sizes["num_indices"], ra.sizes["num_meshes"]), (zb, ra.sizes)
        t = {k: [] for k in "abc"}
        for r in range(args.rounds):
            for k in ("abc", "bca", "cab")[r % 3]:
                t[k].append(sample(calls[k]))
        res[name + "_draws"], res[name + "_dashed_draws"] = n, int(ns)
        res[name + "_pieces"], res[name + "_meshes"], res[name + "_vertices"] = ra.dash_sizes["num_subpaths"], ra.sizes["num_meshes"], ra.sizes["num_vertices"]
        res[name + "_undashed_meshes"], res[name + "_undashed_vertices"] = rc.sizes["num_meshes"], rc.sizes["num_vertices"]
        for k in "abc":
            v = sorted(t[k])
            res["%s_%s_ms_median" % (name, k)], res["%s_%s_ms_min" % (name, k)], res["%s_%s_ms_max" % (name, k)] = v[len(v) // 2], v[0], v[-1]
        res[name + "_a_over_b"] = res[name + "_a_ms_median"] / res[name + "_b_ms_median"]
        res[name + "_a_over_c"] = res[name + "_a_ms_median"] / res[name + "_c_ms_median"]
        res[name + "_a_below_b_beyond_spread"] = bool(res[name + "_a_ms_max"] < res[name + "_b_ms_min"])
        for p in (pset_a, pset_b, pset_c):
            p.close()
        for c in (ctx_a, ctx_b, ctx_c):
            c.close()
        del bufs_a, bufs_c, bufs_ba, bufs_bb, bufs_bo, dbufs, fbufs

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
