"""vgx_raster_commands beside vgx_raster_painted, one job on one box, every shape warmed up, the variants alternating; host clock around
`call; synchronise`, scratch sized before the clock starts (reserve calls and untimed calls that check dev_status); medians and ranges
of R rounds. Into size x size, over a clear:
  tiger_*   ONE Tiger (about 890 x 770 pixels) tessellated under an armed draw-command assembly (VGX_ASM_SPLIT_STATE): a few draw
            commands of tens of thousands of triangles
  text_*    the same frame plus 4 096 glyph quads in 64 runs (one sampled command / mesh per run)
  quad_*    one quad over the whole image
each three ways:
  *_commands    vgx_raster_commands on the command table (bins chunks of 64 triangles)
  *_per_command vgx_raster_painted on the equivalent frame of one TRILIST mesh per command (bins meshes: what a caller could fake before)
  *_unassembled vgx_raster_painted on the unassembled frame (per-draw state, mesh-local indices); for quad_* the same frame as per_command
`*_same_image` says whether the three images were equal byte for byte.

python profiles/raster_commands_timing.py [--rounds R] [--size N] [--out profiles/raster_commands_timing.json]   (prints one JSON object)"""
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
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return torch.from_numpy(raw.copy() if raw.size else np.zeros(16, dtype=np.uint8)).to(dev)

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

    ctx = rt.Context(0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def checked(fn):
        for _ in range(3):
            fn()
            torch.cuda.synchronize()
            if int(status.item()) == 0:
                return
        raise RuntimeError("the call did not reach VGX_OK: %d" % int(status.item()))

    # ---- the Tiger, unassembled and assembled ----
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    probe = rt.tessellate(ctx, pset, rt.upload_draws(d), d.shape[0])
    lo = np.floor(probe.pos.reshape(-1, 2).min(axis=0))
    d = d.copy()
    d["mtx"][:, 4] -= np.float32(lo[0])  # the drawing's corner to the frame's origin: a command's scissor is unsigned
    d["mtx"][:, 5] -= np.float32(lo[1])
    dd = rt.upload_draws(d)
    plain = rt.tessellate(ctx, pset, dd, d.shape[0])
    nd, nm, nv, ni = d.shape[0], plain.meshes.shape[0], plain.pos.reshape(-1, 2).shape[0], plain.idx.shape[0]
    cap = 64
    dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device=dev)
    num = torch.zeros(1, dtype=torch.int64, device=dev)
    white = int(np.array([16384, 16384], dtype=np.int16).view(np.uint32)[0])
    auv = torch.zeros((nv, 2), dtype=torch.int16, device=dev)
    bufs = rt.MeshBuffers(dev, nv, ni, nm)
    ctx.set_assembly(dcmds, max_vb_vertices=65536, dev_num=num, split_state=True, uv=auv, uv_value=(white, 0))
    try:
        rt.tessellate_count(ctx, pset, dd, nd)
        rt.tessellate_emit(ctx, pset, dd, nd, bufs)
    finally:
        ctx.set_assembly(None)
    torch.cuda.synchronize()
    pset.close()
    dstate = np.zeros(nd, dtype=capi.draw_state_dtype)
    dstate["scissor"], dstate["clip_first_draw"] = (0, 0, size, size), 0xFFFFFFFF
    out, n, st = rt.raster_cmds_from_assembly(ctx, dcmds, cap, num, bufs.meshes, nm, up(dstate), nd)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    k = int(n.item())
    tiger_cmds = out.cpu().numpy()[:k * 56].view(capi.raster_cmd_dtype).copy()
    apos, acol, aidx = bufs.pos[:nv].cpu().numpy(), bufs.color[:nv].cpu().numpy().view(np.uint32), bufs.idx[:ni].cpu().numpy().view(np.uint16)
    auv_h = auv.cpu().numpy()
    res["tiger"] = {"draws": nd, "meshes": nm, "vertices": nv, "indices": ni, "commands": k}

    # ---- 4 096 glyph quads in 64 runs, behind the Tiger's vertices and indices ----
    rs = np.random.RandomState(7)
    gpos, gcol, guv, gidx, gcmds, gmesh = [], [], [], [], [], []
    for run in range(64):
        x0, y0 = float(rs.randint(0, max(size - 64 * 9, 1))), float(rs.randint(12, size - 4))
        v0 = len(gpos)
        for q in range(64):
            x = x0 + 9.0 * q
            gpos += [(x, y0 - 12.0), (x + 8.0, y0 - 12.0), (x + 8.0, y0), (x, y0)]
            u = (q % 8) / 8.0
            guv += [(u, 0.0), (u + 0.125, 0.0), (u + 0.125, 1.0), (u, 1.0)]
            gidx += [4 * q, 4 * q + 1, 4 * q + 2, 4 * q, 4 * q + 2, 4 * q + 3]
        gcol += [0xFF000000 | int(rs.randint(1 << 24))] * 256
        gcmds.append((nv + v0, ni + 384 * run, 256, 384, 0, 1, (0, 0, size, size), 0, 0xFFFFFFFF, 0, 0))
        gmesh.append((v0, 384 * run, 256, 384, nd + run, capi.MESH_TEXT << 28))
    guv16 = np.round(np.array(guv) * 32767.0).astype(np.int16)
    glyphs = rs.randint(0, 1 << 32, size=(16, 64), dtype=np.uint64).astype(np.uint32)
    images = [torch.full((2, 2), -1, dtype=torch.int32, device=dev), torch.from_numpy(glyphs.view(np.int32)).to(dev)]
    images_dev = rt.raster_images([(images[0], capi.IMAGE_NEAREST), (images[1], 0)], dev)

    def scene(pos, col, uv, idx, cmds):
        t = [up(pos.astype(np.float32)), up(col.astype(np.uint32)), up(uv.astype(np.int16)), up(idx.astype(np.uint16)), up(cmds)]
        return t, rt.raster_streams(t[0], t[1], t[3], pos.shape[0], idx.shape[0], uv_dev=t[2], uv_bytes=4), cmds.shape[0]

    def frame(pos, col, uv, idx, meshes, draws, dstate):
        t = [up(pos.astype(np.float32)), up(col.astype(np.uint32)), up(idx.astype(np.uint16)), up(meshes), up(uv.astype(np.int16)), up(draws), up(dstate)]
        return t, capi.CacheDesc(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), meshes.shape[0], pos.shape[0], idx.shape[0]), draws.shape[0]

    def per_command(pos, col, uv, idx, cmds):
        m = np.zeros(cmds.shape[0], dtype=capi.mesh_dtype)
        for f in ("first_vertex", "first_index", "num_vertices", "num_indices"):
            m[f] = cmds[f]
        m["draw"], m["subpath_kind"] = np.arange(cmds.shape[0]), capi.MESH_TRILIST << 28
        dr = np.zeros(cmds.shape[0], dtype=capi.draw_dtype)
        dr["state_key"] = (cmds["type"] << 16) | (cmds["handle"] & 0xFFFF)
        ds = np.zeros(cmds.shape[0], dtype=capi.draw_state_dtype)
        ds["scissor"], ds["clip_first_draw"] = cmds["scissor"], 0xFFFFFFFF
        return frame(pos, col, uv, idx, m, dr, ds)

    img = torch.zeros((size, size), dtype=torch.int32, device=dev)
    empty = up(np.zeros(1, dtype=capi.paint_dtype))

    def commands_call(sc):
        keep, streams, nc = sc
        return lambda: rt.raster_commands(ctx, streams, keep[4], nc, size, size, images_dev=images_dev, num_images=2, clear_color=CLEAR, image=img, dev_status=status)

    def painted_call(fr):
        keep, desc, ndraws = fr
        return lambda: rt.raster_painted(ctx, desc, keep[5], keep[6], ndraws, keep[4], 4, images_dev, 2, empty, 0, empty, 0, size, size, clear_color=CLEAR, image=img,
                                         dev_status=status)

    def case(name, sc, fr_cmd, fr_plain):
        calls = {name + "_commands": commands_call(sc), name + "_per_command": painted_call(fr_cmd), name + "_unassembled": painted_call(fr_plain)}
        shots = []
        for key in sorted(calls):
            checked(calls[key])
            shots.append(img.clone())
        res[name + "_same_image"] = bool(all(torch.equal(shots[0], s) for s in shots[1:]))
        alternate(calls)

    rt.raster_reserve(ctx, nm + 128, 64 * (nm + 128) + (size // 16 + 1) ** 2 * 8)
    rt.raster_commands_reserve(ctx, 128, (ni // 192) + 4096, 1 << 18)
    # (a) the Tiger
    dr0 = np.zeros(nd, dtype=capi.draw_dtype)
    case("tiger", scene(apos, acol, auv_h, aidx, tiger_cmds), per_command(apos, acol, auv_h, aidx, tiger_cmds),
         frame(plain.pos.reshape(-1, 2), plain.color, np.zeros((nv, 2), dtype=np.int16), plain.idx, plain.meshes, dr0, dstate))
    # (b) and the glyph runs
    gp, gc = np.array(gpos, dtype=np.float32), np.array(gcol, dtype=np.uint32)
    tcmds = np.concatenate([tiger_cmds, np.array(gcmds, dtype=capi.raster_cmd_dtype)])
    tpos, tcol, tuv, tidx = np.concatenate([apos, gp]), np.concatenate([acol, gc]), np.concatenate([auv_h, guv16]), np.concatenate([aidx, np.array(gidx, dtype=np.uint16)])
    gm = np.array(gmesh, dtype=capi.mesh_dtype)
    gm["first_vertex"] += nv
    gm["first_index"] += ni
    dr1 = np.zeros(nd + 64, dtype=capi.draw_dtype)
    dr1["state_key"][nd:] = 1  # type 0, image 1
    ds1 = np.zeros(nd + 64, dtype=capi.draw_state_dtype)
    ds1["scissor"], ds1["clip_first_draw"] = (0, 0, size, size), 0xFFFFFFFF
    case("text", scene(tpos, tcol, tuv, tidx, tcmds), per_command(tpos, tcol, tuv, tidx, tcmds),
         frame(np.concatenate([plain.pos.reshape(-1, 2), gp]), np.concatenate([plain.color, gc]), np.concatenate([np.zeros((nv, 2), dtype=np.int16), guv16]),
               np.concatenate([plain.idx, np.array(gidx, dtype=np.uint16)]), np.concatenate([plain.meshes, gm]), dr1, ds1))
    # (c) one quad over the whole image
    qpos = np.array([(0, 0), (size, 0), (size, size), (0, size)], dtype=np.float32)
    qcmd = np.array([(0, 0, 4, 6, 0, 0, (0, 0, size, size), 0, 0xFFFFFFFF, 0, 0)], dtype=capi.raster_cmd_dtype)
    qargs = (qpos, np.full(4, 0x80402010, dtype=np.uint32), np.full((4, 2), 16384, dtype=np.int16), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16), qcmd)
    case("quad", scene(*qargs), per_command(*qargs), per_command(*qargs))
    res["scratch_bytes"] = ctx.scratch_bytes()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
