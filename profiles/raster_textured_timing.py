"""vgx_raster_textured beside vgx_raster_frame, one job on one box, warmed up, the variants alternating; host clock around
`call; synchronise`, scratch sized before the clock starts (vgx_raster_reserve and untimed calls that check dev_status). The frame is
raster_frame_timing.py's: ONE Tiger (vgx_tessellate's frame, moved to the frame's origin, about 890 x 770 pixels) into size x size,
over a clear, every draw's scissor the whole image, no regions.
  unused_*    (a) the frame as it is -- no sampled mesh -- through vgx_raster_textured (`_textured`) against vgx_raster_frame (`_frame`):
              what the wider tile kernel costs when nothing is sampled. `unused_exceeds_frame_range` says whether the difference of the
              medians is larger than the run-to-run range (max - min) of vgx_raster_frame in this job
  glyphs_*    (b) the same frame and, behind it, `--glyphs` glyph quads of 12 x 16 pixels in text runs of 64 (meshes of kind TEXT under
              one Textured draw) from a 512 x 512 atlas, int16 UVs: linear (`_linear`) and nearest (`_nearest`), beside the frame alone
              through the same call (`_none`)
  blit_*      (c) one quad over the whole image sampled 1:1 from a size x size image, linear and nearest, against the ruler of
              raster_timing.py: a kernel that only STORES the image (`_store_only`)

python profiles/raster_textured_timing.py [--rounds R] [--size N] [--glyphs G] [--out profiles/raster_textured_timing.json]   (prints one JSON object)"""
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
    ap.add_argument("--glyphs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    dev = torch.device("cuda", 0)
    size = args.size
    res = {"box": torch.cuda.get_device_name(0), "rounds": args.rounds, "size": size, "glyphs": args.glyphs}

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

    def draw_table(n, keys):
        draws = np.zeros(n, dtype=capi.draw_dtype)
        draws["state_key"] = keys
        st = np.zeros(n, dtype=capi.draw_state_dtype)
        st["scissor"] = (0, 0, size, size)
        st["clip_first_draw"] = 0xFFFFFFFF
        return up(draws), up(st), n

    img = torch.zeros((size, size), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nruns = (args.glyphs + 63) // 64
    rt.raster_reserve(ctx, nm + nruns + 2, 64 * (nm + nruns + 2) + (size // 16 + 1) ** 2 * 8)

    def checked(fn):
        for _ in range(3):
            fn()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return
        raise RuntimeError("the call did not reach VGX_OK: %d" % int(status.item()))

    # (a) no sampled mesh
    keep, desc = device_frame(pos, got.color, got.idx, meshes)
    dt = draw_table(nd, 0)
    no_uv = torch.zeros((nv, 2), dtype=torch.int16, device=dev)
    frame = lambda: rt.raster_frame(ctx, desc, dt[0], dt[1], dt[2], size, size, clear_color=CLEAR, image=img, dev_status=status)
    textured = lambda: rt.raster_textured(ctx, desc, dt[0], dt[1], dt[2], no_uv, 4, None, 0, size, size, clear_color=CLEAR, image=img, dev_status=status)
    checked(frame)
    a = img.clone()
    checked(textured)
    res["unused_same_image"] = bool(torch.equal(a, img))
    alternate({"unused_frame": frame, "unused_textured": textured})
    res["unused_cost_ms"] = res["unused_textured_ms_median"] - res["unused_frame_ms_median"]
    res["frame_range_ms"] = res["unused_frame_ms_max"] - res["unused_frame_ms_min"]
    res["unused_exceeds_frame_range"] = bool(res["unused_cost_ms"] > res["frame_range_ms"])

    # (b) glyph quads behind the frame: runs of 64 quads of 12 x 16 pixels on a grid over the image, cells of a 512 x 512 atlas
    rs = np.random.RandomState(1)
    g = args.glyphs
    per_row = max(size // 14, 1)
    gx, gy = (np.arange(g) % per_row) * 14.0 + 1.25, ((np.arange(g) // per_row) * 18.0 + 1.5) % max(size - 18, 1)
    corners = np.stack([np.stack([gx, gy], 1), np.stack([gx + 12, gy], 1), np.stack([gx + 12, gy + 16], 1), np.stack([gx, gy + 16], 1)], 1).reshape(-1, 2)
    cell = rs.randint(0, 32 * 32, size=g)
    s0, t0 = (cell % 32) / 32.0, (cell // 32) / 32.0
    st_ = np.stack([np.stack([s0, t0], 1), np.stack([s0 + 1 / 32.0, t0], 1), np.stack([s0 + 1 / 32.0, t0 + 1 / 32.0], 1), np.stack([s0, t0 + 1 / 32.0], 1)], 1).reshape(-1, 2)
    guv = (st_.astype(np.float32) * np.float32(32767)).astype(np.int32).astype(np.int16)
    gidx = np.tile(np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), g) + np.repeat((4 * (np.arange(g) % 64)).astype(np.uint16), 6)
    tab = np.zeros(nm + nruns, dtype=capi.mesh_dtype)
    tab[:nm] = meshes
    q = np.minimum(64, g - 64 * np.arange(nruns))
    tab["first_vertex"][nm:], tab["first_index"][nm:] = nv + 4 * 64 * np.arange(nruns), ni + 6 * 64 * np.arange(nruns)
    tab["num_vertices"][nm:], tab["num_indices"][nm:], tab["draw"][nm:], tab["subpath_kind"][nm:] = 4 * q, 6 * q, nd, capi.MESH_TEXT << 28
    keep2, desc2 = device_frame(np.concatenate([pos, corners]), np.concatenate([got.color, np.full(4 * g, 0xFFFFFFFF, dtype=np.uint32)]),
                                np.concatenate([got.idx, gidx]), tab)
    uv2 = up(np.concatenate([np.zeros((nv, 2), dtype=np.int16), guv]))
    y, x = np.mgrid[0:512, 0:512]
    atlas = (((x * 7 + y * 13) & 255) << 24 | 0x00FFFFFF).astype(np.uint32)
    atlas_dev = torch.from_numpy(atlas.view(np.int32)).to(dev)
    dg = draw_table(nd + 1, 0)

    def glyph_call(flags):
        recs = rt.raster_images([(atlas_dev, flags)], dev)
        return lambda: rt.raster_textured(ctx, desc2, dg[0], dg[1], dg[2], uv2, 4, recs, 1, size, size, clear_color=CLEAR, image=img, dev_status=status)

    linear, nearest = glyph_call(0), glyph_call(capi.IMAGE_NEAREST)
    checked(linear)
    res["glyphs_pixels_changed"] = int((img != a).sum().item())
    checked(nearest)
    alternate({"glyphs_linear": linear, "glyphs_nearest": nearest, "glyphs_none": textured})

    # (c) one quad over the whole image, sampled 1:1
    quad = np.array([(0, 0), (size, 0), (size, size), (0, size)], dtype=np.float32)
    one = np.zeros(1, dtype=capi.mesh_dtype)
    one["num_vertices"], one["num_indices"], one["subpath_kind"] = 4, 6, capi.MESH_TRILIST << 28
    keep3, desc3 = device_frame(quad, np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), one)
    uv3 = up(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=np.float32))
    y, x = np.mgrid[0:size, 0:size]
    src = (0xFF000000 | ((x * 3 + y * 5) & 0xFFFFFF)).astype(np.uint32)
    src_dev = torch.from_numpy(src.view(np.int32)).to(dev)
    db = draw_table(1, 0)

    def blit_call(flags):
        recs = rt.raster_images([(src_dev, flags)], dev)
        return lambda: rt.raster_textured(ctx, desc3, db[0], db[1], db[2], uv3, 8, recs, 1, size, size, clear_color=CLEAR, image=img, dev_status=status)

    blit_linear, blit_nearest = blit_call(0), blit_call(capi.IMAGE_NEAREST)
    checked(blit_linear)
    res["blit_linear_exact"] = bool(torch.equal(img, src_dev))
    checked(blit_nearest)
    res["blit_nearest_exact"] = bool(torch.equal(img, src_dev))
    alternate({"blit_linear": blit_linear, "blit_nearest": blit_nearest, "blit_store_only": lambda: img.fill_(-1)})
    res["scratch_bytes"] = ctx.scratch_bytes()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
