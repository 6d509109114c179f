"""The damage redraw beside a full redraw: one job on one box, warmed up, the variants alternating; host clock around `call(s); synchronise`,
buffers and scratch sized before the clock starts; medians and ranges of --rounds rounds.
  (a) a --drawings-side x --drawings-side grid of cached Tigers (one instance per drawing, scaled so that the grid fills the image) into
      1024 x 1024 and 4096 x 4096; k = 1, 16, 256 scattered instances moved by a few pixels, to and fro:
        s<size>_k<k>_chain     zero the bits, vgx_damage_instances, vgx_cache_update, vgx_damage_instances, vgx_raster_damaged
        s<size>_k<k>_marks     the two vgx_damage_instances calls alone (with the zeroing)
        s<size>_full           vgx_cache_update + vgx_raster_concave with clear: what the library needed before
        s<size>_k16_scissored  vgx_cache_update + 16 vgx_raster_concave calls, each under the scissor around one moved drawing
      with the tiles marked and the bin entries of the damaged call (counted on the host from the boxes and the bits), and whether the
      damaged image equals the full one. The variants alternate on one context, so each timed chain names its own sort window
      (max_entries = 1.25 x its entries + 256); the library's window (max_entries = 0) follows the LAST damaged call, which here would
      be another variant's.
  (b) --concave-only: vgx_raster_concave on the same grid into 1024 x 1024, nothing else: the program the parent job starts twice per
      round, once on this build and once on the library --parent-lib names (through VGX_LIB), to see what carrying the bitmap costs the
      existing call. The allowance is the parent library's own run-to-run range.

python profiles/damage_timing.py [--rounds R] [--drawings-side S] [--parent-lib FILE] [--out profiles/damage_timing.json]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF
CLEAR = 0xFF201810


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--drawings-side", type=int, default=40)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--concave-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    if args.concave_only:   # the parent's library lacks the calls this build adds: bind what it has
        import ctypes
        have = ctypes.CDLL(rt.LIB_PATH)
        for name in [k for k in capi.VGX_SYMBOLS if not hasattr(have, k)]:
            del capi.VGX_SYMBOLS[name]
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

    def alternate(calls, out):
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
            out[k + "_ms_median"], out[k + "_ms_min"], out[k + "_ms_max"] = v[len(v) // 2], v[0], v[-1]

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
    n = S * S
    nm, nv = cache.nm * n, cache.nv * n
    res["meshes"] = nm
    draws = np.zeros(n, dtype=capi.draw_dtype)
    st = np.zeros(n, dtype=capi.draw_state_dtype)
    st["scissor"], st["clip_first_draw"] = (0, 0, 65535, 65535), NONE
    dt = (up(draws), up(st), n)
    uv = torch.zeros(8, dtype=torch.uint8, device=dev)  # no mesh is sampled: never read

    def grid(size):
        s = size / (S * pitch)
        inst = np.zeros(n, dtype=capi.cache_instance_dtype)
        cell = np.arange(n)
        inst["num_meshes"], inst["color"] = cache.nm, 0xC0FFFFFF
        inst["mtx"][:, 0] = inst["mtx"][:, 3] = s
        inst["mtx"][:, 4], inst["mtx"][:, 5] = ((cell % S) * pitch - lo[0]) * s, ((cell // S) * pitch - lo[1]) * s
        return inst

    def full(desc, size, mb, img, status, scissor=None):
        rt.raster_concave(ctx, desc, dt[0], dt[1], dt[2], uv, 8, None, 0, None, 0, None, 0, size, size, scissor=scissor, clear_color=CLEAR, bounds_dev=mb,
                          image=img, dev_status=status)

    def until_ok(fn, status):
        for _ in range(4):
            fn()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return
        raise RuntimeError("the call did not reach VGX_OK: %d" % int(status.item()))

    for size in ((1024,) if args.concave_only else (1024, 4096)):
        inst0 = grid(size)
        out = rt.MeshBuffers(dev, nv, cache.ni * n, nm)
        i0 = up(inst0)
        rt.cache_submit(ctx, cache, i0, n, out)
        slots, _ = rt.cache_layout(ctx, cache, i0, n)
        mb = rt.mesh_bounds(ctx, out.pos, out.meshes, nm)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0
        desc = capi.CacheDesc(out.pos.data_ptr(), out.color.data_ptr(), out.idx.data_ptr(), out.meshes.data_ptr(), nm, nv, cache.ni * n)
        img = torch.zeros((size, size), dtype=torch.int32, device=dev)
        ref = torch.zeros((size, size), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        until_ok(lambda: full(desc, size, mb, img, status), status)
        if args.concave_only:
            t = {}
            alternate({"concave": lambda: full(desc, size, mb, img, status)}, t)
            print(json.dumps(t))
            ctx.close()
            return
        bits = torch.zeros(rt.damage_words(size, size), dtype=torch.int32, device=dev)
        tw = (size + 15) // 16
        rs = np.random.RandomState(11)
        sec = {}
        calls = {}
        after = {}
        cellpx = size / S
        for k in (1, 16, 256):
            dirty = rs.choice(n, k, replace=False).astype(np.uint32)
            moved = inst0.copy()
            moved["mtx"][dirty, 4] += np.float32(3.0)
            moved["mtx"][dirty, 5] += np.float32(2.0)
            arrays = (up(moved), i0)
            ddirty = up(dirty)
            ust = torch.zeros(3, dtype=torch.int32, device=dev)

            def update(k=k, arrays=arrays, ddirty=ddirty, ust=ust, flip=[0]):
                flip[0] ^= 1   # to and fro: every call moves its drawings
                rt.cache_update(ctx, cache, arrays[flip[0] ^ 1], n, slots, ddirty, k, out.pos, out.color, nv, nm, mesh_bounds=mb, dev_status=ust[1:2])

            def marks_only(k=k, ddirty=ddirty, ust=ust):
                bits.zero_()
                rt.damage_instances(ctx, mb, nm, slots, n, ddirty, k, size, size, bits, dev_status=ust[0:1])
                rt.damage_instances(ctx, mb, nm, slots, n, ddirty, k, size, size, bits, dev_status=ust[2:3])

            window = [0]   # max_entries of the timed calls: the variants alternate on one context, so each names its own window
            kstatus = torch.zeros(1, dtype=torch.int32, device=dev)

            def chain(k=k, ddirty=ddirty, ust=ust, update=update, window=window, kstatus=kstatus):
                bits.zero_()
                rt.damage_instances(ctx, mb, nm, slots, n, ddirty, k, size, size, bits, dev_status=ust[0:1])
                update()
                rt.damage_instances(ctx, mb, nm, slots, n, ddirty, k, size, size, bits, dev_status=ust[2:3])
                rt.raster_damaged(ctx, desc, dt[0], dt[1], dt[2], uv, 8, None, 0, None, 0, None, 0, size, size, bits, img, max_entries=window[0], clear_color=CLEAR,
                                  bounds_dev=mb, dev_status=kstatus)

            # the image the chain leaves against a full redraw of the same frame; the tiles and the entries of that call
            until_ok(lambda: full(desc, size, mb, img, status), status)
            for _ in range(3):   # the window settles
                chain()
                torch.cuda.synchronize()
            tag = "s%d_k%d" % (size, k)
            sec[tag + "_damaged_status"] = int(kstatus.item())
            until_ok(lambda: full(desc, size, mb, ref, status), status)
            sec[tag + "_equals_full"] = bool(torch.equal(img, ref))
            hb = bits.cpu().numpy().view(np.uint32)
            tiles = ((hb[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:tw * tw].reshape(tw, tw).astype(np.int64)
            sec[tag + "_tiles_marked"], sec[tag + "_tiles"] = int(tiles.sum()), tw * tw
            b = mb.cpu().numpy().astype(np.float64)
            i_lo, i_hi = np.maximum(np.floor(b[:, 0] - 0.5), 0), np.minimum(np.ceil(b[:, 2] - 0.5), size - 1)
            j_lo, j_hi = np.maximum(np.floor(b[:, 1] - 0.5), 0), np.minimum(np.ceil(b[:, 3] - 0.5), size - 1)
            ok = (i_lo <= i_hi) & (j_lo <= j_hi)
            pre = np.zeros((tw + 1, tw + 1), dtype=np.int64)
            pre[1:, 1:] = tiles.cumsum(0).cumsum(1)
            x0, x1, y0, y1 = (i_lo[ok] // 16).astype(int), (i_hi[ok] // 16).astype(int) + 1, (j_lo[ok] // 16).astype(int), (j_hi[ok] // 16).astype(int) + 1
            sec[tag + "_entries"] = int((pre[y1, x1] - pre[y0, x1] - pre[y1, x0] + pre[y0, x0]).sum())
            window[0] = sec[tag + "_entries"] + sec[tag + "_entries"] // 4 + 256
            sec[tag + "_max_entries"] = window[0]
            after[tag] = kstatus
            calls[tag + "_chain"] = chain
            calls[tag + "_marks"] = marks_only
            if k == 16:
                rects = []
                for c in dirty:
                    cx, cy = (int(c) % S) * cellpx, (int(c) // S) * cellpx
                    rects.append((max(int(cx) - 2, 0), max(int(cy) - 2, 0), min(int(cx + cellpx) + 6, size), min(int(cy + cellpx) + 5, size)))

                def scissored(update=update, rects=rects):
                    update()
                    for r in rects:
                        full(desc, size, mb, img, status, scissor=r)
                calls["s%d_k16_scissored" % size] = scissored
            if k == 1:
                def full_redraw(update=update):
                    update()
                    full(desc, size, mb, img, status)
                calls["s%d_full" % size] = full_redraw
        alternate(calls, sec)
        for tag, t in after.items():
            sec[tag + "_damaged_status_after_timing"] = int(t.item())
        for k in (1, 16, 256):
            sec["s%d_k%d_chain_over_full" % (size, k)] = sec["s%d_k%d_chain_ms_median" % (size, k)] / sec["s%d_full_ms_median" % size]
        res.update(sec)
        res["scratch_bytes_s%d" % size] = ctx.scratch_bytes()
        del out, mb, img, ref
    ctx.close()

    def write():
        line = json.dumps(res)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    write()   # section (a) is kept whatever becomes of the child processes below
    if args.parent_lib:
        runs = {"this": [], "parent": []}
        for r in range(3):
            for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                env = dict(os.environ)
                if which == "parent":
                    env["VGX_LIB"] = os.path.abspath(args.parent_lib)
                o = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--concave-only", "--rounds", str(args.rounds), "--drawings-side", str(S)],
                                            env=env, text=True, timeout=600)
                runs[which].append(json.loads(o.strip().splitlines()[-1])["concave_ms_median"])
        res["concave_1024_this_ms"], res["concave_1024_parent_ms"] = sorted(runs["this"]), sorted(runs["parent"])
        res["concave_1024_parent_range_ms"] = max(runs["parent"]) - min(runs["parent"])
        res["concave_1024_cost_ms"] = sorted(runs["this"])[1] - sorted(runs["parent"])[1]
        res["concave_1024_cost_exceeds_parent_range"] = bool(res["concave_1024_cost_ms"] > res["concave_1024_parent_range_ms"])

    print(write())


if __name__ == "__main__":
    main()
