"""vgx_raster_frame beside vgx_raster, one job on one box, warmed up, the variants alternating; host clock around `call(s); synchronise`,
scratch sized before the clock starts (vgx_raster_reserve and untimed calls that check dev_status). ONE Tiger (vgx_tessellate's frame,
moved to the frame's origin, about 890 x 770 pixels) into size x size, over a clear.
  replayK_*   K = 1, 8, 64 runs of draws, each under a scissor of its own, no regions: ONE vgx_raster_frame call (`_frame`) against
              the only thing the library could do for that frame before, K vgx_raster calls, one per run with the target's scissor set
              to the run's (`_calls`; the first of them clears the whole image under the full scissor, as a caller would)
  unused_*    one scissor that cuts nothing, no regions: vgx_raster_frame against one vgx_raster call -- what carrying the state costs
              when it is not used. `unused_exceeds_raster_range` says whether the difference of the medians is larger than the
              run-to-run range (max - min) of vgx_raster in this job
  region_*    one In region over the left half of the window (one clip quad in front of the frame), every draw tested against it

python profiles/raster_frame_timing.py [--rounds R] [--size N] [--out profiles/raster_frame_timing.json]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLEAR = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    size = args.size
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "size": size}

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

    # the frame: one Tiger, tessellated on the device, and a copy of its streams on the host
    ctx = rt.Context(0)
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    probe = rt.tessellate(ctx, pset, rt.upload_draws(d), d.shape[0])
    lo = np.floor(probe.pos.reshape(-1, 2).min(axis=0))
    d = d.copy()
    d["mtx"][:, 4] -= np.float32(lo[0])  # the drawing's corner to the frame's origin: a draw scissor is unsigned
    d["mtx"][:, 5] -= np.float32(lo[1])
    got = rt.tessellate(ctx, pset, rt.upload_draws(d), d.shape[0])
    pset.close()
    nd = d.shape[0]
    meshes = got.meshes.copy()
    pos = got.pos.reshape(-1, 2)
    nm, nv, ni = meshes.shape[0], pos.shape[0], got.idx.shape[0]
    res["meshes"], res["vertices"], res["indices"], res["draws"] = nm, nv, ni, nd

    def device_frame(pos, color, idx, mesh_tab):
        t = [up(pos.astype(np.float32)), up(color.astype(np.uint32)), up(idx.astype(np.uint16)), up(mesh_tab)]
        return t, capi.CacheDesc(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), mesh_tab.shape[0], pos.shape[0], idx.shape[0])

    keep, desc = device_frame(pos, got.color, got.idx, meshes)
    img = torch.zeros((size, size), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rt.raster_reserve(ctx, nm + 1, 64 * (nm + 1) + (size // 16 + 1) ** 2 * 8)

    def checked(fn):
        for _ in range(3):
            fn()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return
        raise RuntimeError("the call did not reach VGX_OK: %d" % int(status.item()))

    def draw_table(scissors, region=None, extra_clip=False):
        draws = np.zeros(nd + (1 if extra_clip else 0), dtype=capi.draw_dtype)
        st = np.zeros(draws.shape[0], dtype=capi.draw_state_dtype)
        st["scissor"][:nd] = scissors
        st["clip_first_draw"] = 0xFFFFFFFF
        if region is not None:
            st["clip_first_draw"][:nd], st["clip_num_draws"][:nd], st["clip_rule"][:nd] = region
        if extra_clip:
            draws["state_key"][nd] = 3 << 16
            st["scissor"][nd] = (0, 0, size, size)
        return up(draws), up(st), draws.shape[0]

    full = (0, 0, size, size)
    plain = lambda: rt.raster(ctx, desc, size, size, clear_color=CLEAR, image=img, dev_status=status)
    checked(plain)

    # 1. K runs of draws under K scissors, no regions
    for K in (1, 8, 64):
        run = (np.arange(nd) * K) // nd
        sc = np.array([(16 * (k % 4), 16 * (k % 3), size - 32 * (k % 4), size - 32 * (k % 3)) for k in range(K)], dtype=np.uint16)
        dt = draw_table(sc[run])
        first = np.searchsorted(run[meshes["draw"]], np.arange(K + 1))  # the meshes follow their draws in ascending order

        def one(dt=dt):
            rt.raster_frame(ctx, desc, dt[0], dt[1], dt[2], size, size, clear_color=CLEAR, image=img, dev_status=status)

        def many(K=K, sc=sc, first=first):
            rt.raster(ctx, desc, size, size, clear_color=CLEAR, mesh_begin=0, mesh_end=0, image=img, dev_status=status)
            for k in range(K):
                x, y, w, h = (int(v) for v in sc[k])
                rt.raster(ctx, desc, size, size, scissor=(x, y, x + w, y + h), mesh_begin=int(first[k]), mesh_end=int(first[k + 1]), image=img, dev_status=status)
        checked(one)
        a = img.clone()
        checked(many)
        res["replay%d_same_image" % K] = bool(torch.equal(a, img))
        alternate({"replay%d_frame" % K: one, "replay%d_calls" % K: many})

    # 2. the state carried and not used
    dt = draw_table(np.array([full] * nd, dtype=np.uint16))
    unused = lambda: rt.raster_frame(ctx, desc, dt[0], dt[1], dt[2], size, size, clear_color=CLEAR, image=img, dev_status=status)
    checked(unused)
    a = img.clone()
    checked(plain)
    res["unused_same_image"] = bool(torch.equal(a, img))
    alternate({"unused_frame": unused, "unused_raster": plain})
    res["unused_cost_ms"] = res["unused_frame_ms_median"] - res["unused_raster_ms_median"]
    res["raster_range_ms"] = res["unused_raster_ms_max"] - res["unused_raster_ms_min"]
    res["unused_exceeds_raster_range"] = bool(res["unused_cost_ms"] > res["raster_range_ms"])

    # 3. one In region over the left half: a clip quad in front of the frame's meshes
    quad = np.array([(0, 0), (size // 2, 0), (size // 2, size), (0, size)], dtype=np.float32)
    tab = np.zeros(nm + 1, dtype=capi.mesh_dtype)
    tab[1:] = meshes
    tab["first_vertex"][1:] += 4
    tab["first_index"][1:] += 6
    tab["num_vertices"][0], tab["num_indices"][0], tab["draw"][0] = 4, 6, nd
    keep2, desc2 = device_frame(np.concatenate([quad, pos]), np.concatenate([np.full(4, 0xFFFFFFFF, dtype=np.uint32), got.color]),
                                np.concatenate([np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), got.idx]), tab)
    dr = draw_table(np.array([full] * nd, dtype=np.uint16), region=(nd, 1, 0), extra_clip=True)
    region = lambda: rt.raster_frame(ctx, desc2, dr[0], dr[1], dr[2], size, size, clear_color=CLEAR, image=img, dev_status=status)
    checked(region)
    res["region_pixels_painted_right_half"] = int((img[:, size // 2:] != -1).sum().item())
    res["region_pixels_painted_left_half"] = int((img[:, :size // 2] != -1).sum().item())
    alternate({"region_frame": region, "region_unused_frame": unused, "region_raster": plain})
    res["scratch_bytes"] = ctx.scratch_bytes()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
