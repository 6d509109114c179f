"""vgx_raster_painted beside vgx_raster_textured, one job on one box, warmed up, the variants alternating; host clock around
`call; synchronise`, scratch sized before the clock starts (vgx_raster_reserve and untimed calls that check dev_status). The frame is
raster_frame_timing.py's: ONE Tiger (vgx_tessellate's frame, moved to the frame's origin, about 890 x 770 pixels) into size x size,
over a clear, every draw's scissor the whole image, no regions.
  unused_*    (a) the frame as it is -- no painted draw -- through vgx_raster_painted (`_painted`) against vgx_raster_textured
              (`_textured`): what the second tile bit and the two further launches cost when nothing is painted.
              `unused_exceeds_textured_range` says whether the difference of the medians is larger than the run-to-run range
              (max - min) of vgx_raster_textured in this job
  fills_*     (b) the same streams with every fill mesh under a ColorGradient draw (one linear gradient across the image, its ends
              opaque) and every stroke mesh under the flat draw, through vgx_raster_painted (`_gradient`), beside (a)'s call in the
              same rounds (`_flat`). `fills_ns_per_changed_pixel` divides the difference of the medians by the pixels that differ
              between the two images: a pixel several fills cover counts once, so it is an upper bound per painted sample
  quad_*      (c) one quad over the whole image: a linear, a box and a radial gradient and an image pattern (nearest and linear, a
              64 x 64 image repeated), against the ruler of raster_timing.py: a kernel that only STORES the image (`_store_only`)

python profiles/raster_painted_timing.py [--rounds R] [--size N] [--out profiles/raster_painted_timing.json]   (prints one JSON object)"""
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
    d["mtx"][:, 4] -= np.float32(lo[0])
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

    def draw_table(keys):
        draws = np.zeros(len(keys), dtype=capi.draw_dtype)
        draws["state_key"] = keys
        st = np.zeros(len(keys), dtype=capi.draw_state_dtype)
        st["scissor"] = (0, 0, size, size)
        st["clip_first_draw"] = 0xFFFFFFFF
        return up(draws), up(st), len(keys)

    def paint(typ, handle, inv, params=(0, 0, 0, 0), inner=0, outer=0, image=0):
        p = np.zeros(1, dtype=capi.paint_dtype)
        p["type"], p["handle"], p["image"] = typ, handle, image
        p["matrix"] = [inv[0], inv[1], 0, inv[2], inv[3], 0, inv[4], inv[5], 1]
        p["params"] = params
        p["inner_color"] = [((inner >> (8 * k)) & 255) / 255.0 for k in range(4)]
        p["outer_color"] = [((outer >> (8 * k)) & 255) / 255.0 for k in range(4)]
        return p

    def linear(handle, inner, outer):  # along x across the image, as ctxCreateLinearGradient builds it under the identity
        return paint(1, handle, (0.0, 1.0, -1.0, 0.0, 0.0, 1e5), (1e5, 1e5 + size * 0.5, 0.0, float(size)), inner, outer)

    img = torch.zeros((size, size), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rt.raster_reserve(ctx, nm + 2, 64 * (nm + 2) + (size // 16 + 1) ** 2 * 8)

    def checked(fn):
        for _ in range(3):
            fn()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return
        raise RuntimeError("the call did not reach VGX_OK: %d" % int(status.item()))

    # (a) no painted draw
    keep, desc = device_frame(pos, got.color, got.idx, meshes)
    dt = draw_table([0] * nd)
    no_uv = torch.zeros((nv, 2), dtype=torch.int16, device=dev)
    textured = lambda: rt.raster_textured(ctx, desc, dt[0], dt[1], dt[2], no_uv, 4, None, 0, size, size, clear_color=CLEAR, image=img, dev_status=status)
    painted = lambda: rt.raster_painted(ctx, desc, dt[0], dt[1], dt[2], no_uv, 4, None, 0, None, 0, None, 0, size, size, clear_color=CLEAR, image=img,
                                        dev_status=status)
    checked(textured)
    a = img.clone()
    checked(painted)
    res["unused_same_image"] = bool(torch.equal(a, img))
    alternate({"unused_textured": textured, "unused_painted": painted})
    res["unused_cost_ms"] = res["unused_painted_ms_median"] - res["unused_textured_ms_median"]
    res["textured_range_ms"] = res["unused_textured_ms_max"] - res["unused_textured_ms_min"]
    res["unused_exceeds_textured_range"] = bool(res["unused_cost_ms"] > res["textured_range_ms"])

    # (b) every fill mesh under one gradient draw (draw 1), every other mesh under the flat draw (draw 0)
    kinds = meshes["subpath_kind"] >> 28
    is_fill = (kinds == capi.MESH_FILL) | (kinds == capi.MESH_FILL_AA) | (kinds == capi.MESH_CONCAVE_FILL_AA)
    tab = meshes.copy()
    tab["draw"] = is_fill.astype(np.uint32)
    res["fill_meshes"] = int(is_fill.sum())
    keep_b, desc_b = device_frame(pos, got.color, got.idx, tab)
    db = draw_table([0, 1 << 16])
    grad = up(linear(0, 0xFF2040FF, 0xFFFFC020))
    flat_b = lambda: rt.raster_painted(ctx, desc, dt[0], dt[1], dt[2], no_uv, 4, None, 0, None, 0, None, 0, size, size, clear_color=CLEAR, image=img,
                                       dev_status=status)
    grad_b = lambda: rt.raster_painted(ctx, desc_b, db[0], db[1], db[2], no_uv, 4, None, 0, grad, 1, None, 0, size, size, clear_color=CLEAR, image=img,
                                       dev_status=status)
    checked(grad_b)
    res["fills_pixels_changed"] = int((img != a).sum().item())
    alternate({"fills_flat": flat_b, "fills_gradient": grad_b})
    res["fills_cost_ms"] = res["fills_gradient_ms_median"] - res["fills_flat_ms_median"]
    res["fills_ns_per_changed_pixel"] = res["fills_cost_ms"] * 1e6 / max(res["fills_pixels_changed"], 1)

    # (c) one quad over the whole image
    quad = np.array([(0, 0), (size, 0), (size, size), (0, size)], dtype=np.float32)
    one = np.zeros(1, dtype=capi.mesh_dtype)
    one["num_vertices"], one["num_indices"], one["subpath_kind"] = 4, 6, capi.MESH_FILL << 28
    uv_c = torch.zeros((4, 2), dtype=torch.int16, device=dev)
    h = size * 0.5
    grads = up(np.concatenate([linear(0, 0xFF000000, 0xFFFFFFFF),
                               paint(1, 1, (1.0, 0.0, 0.0, 1.0, -h, -h), (h * 0.6, h * 0.4, h * 0.2, h * 0.3), 0xFFFFFFFF, 0xFF203040),   # box
                               paint(1, 2, (1.0, 0.0, 0.0, 1.0, -h, -h), (h * 0.5, h * 0.5, h * 0.5, h * 0.8), 0xFF40FFFF, 0xFF800040)]))  # radial
    y, x = np.mgrid[0:64, 0:64]
    src_dev = torch.from_numpy((0xFF000000 | ((x * 4) << 16) | ((y * 4) << 8) | ((x ^ y) * 4)).astype(np.uint32).view(np.int32)).to(dev)
    cs, sn = np.cos(0.3), np.sin(0.3)
    pats = up(paint(2, 0, (cs / 64.0, -sn / 64.0, sn / 64.0, cs / 64.0, 0.0, 0.0)))
    dg, dp = draw_table([1 << 16, (1 << 16) | 1, (1 << 16) | 2]), draw_table([2 << 16])

    alive = []

    def quad_call(draw_tab, which, flags=0):
        recs = rt.raster_images([(src_dev, flags)], dev)
        tab_c = one.copy()
        tab_c["draw"] = which
        k, dsc = device_frame(quad, np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), tab_c)
        alive.append((k, recs))
        return lambda: rt.raster_painted(ctx, dsc, draw_tab[0], draw_tab[1], draw_tab[2], uv_c, 4, recs, 1, grads, 3, pats, 1, size, size, clear_color=CLEAR,
                                         image=img, dev_status=status)

    calls = {"quad_linear": quad_call(dg, 0), "quad_box": quad_call(dg, 1), "quad_radial": quad_call(dg, 2),
             "quad_pattern_nearest": quad_call(dp, 0, capi.IMAGE_NEAREST), "quad_pattern_linear": quad_call(dp, 0, 0)}
    for k in sorted(calls):
        checked(calls[k])
        res[k + "_pixels_changed"] = int((img != -1).sum().item())
    calls["quad_store_only"] = lambda: img.fill_(-1)
    alternate(calls)
    res["scratch_bytes"] = ctx.scratch_bytes()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
