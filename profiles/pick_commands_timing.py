"""vgx_pick_commands beside vgx_pick_frame on the same drawing: one job on one box, every shape warmed up, the variants alternating; host
clock around `call; synchronise`, buffers and scratch sized before the clock starts; medians and ranges of --rounds rounds.
  tiger_*   one Tiger tessellated under vgx_set_assembly (VGX_ASM_SPLIT_STATE, 65 536-vertex buffers) and turned into a command table by
            vgx_raster_cmds_from_assembly, 1 / 16 / 256 cursor positions through vgx_pick_commands with the mesh table as owners; the
            same Tiger tessellated WITHOUT assembly through vgx_pick_frame under an all-PLAIN draw table, boxes taken once by vgx_mesh_bounds
  grid_*    --drawings-side x --drawings-side cached Tigers (one instance per drawing) submitted under an armed assembly with 65 536-vertex
            buffers, against vgx_pick_frame on the same grid submitted without
The yardstick is vgx_pick_frame in the same job: per section `*_ratio` = median(vgx_pick_commands) / median(vgx_pick_frame),
`*_pick_frame_range_ms` = max - min of vgx_pick_frame, and whether the difference of the medians exceeds that range. The hit records are
compared: mesh and draw of the two calls must agree.
`--trace-only` runs the 256-position calls a few times and nothing else: the program of a rocprofv3 --kernel-trace --stats run, which
says which kernel carries a cost.

python profiles/pick_commands_timing.py [--rounds R] [--drawings-side S] [--out FILE]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NONE = 0xFFFFFFFF
WIDE = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--drawings-side", type=int, default=40)
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

    def compare(section):
        new, old = section + "_pick_commands", section + "_pick_frame"
        res[section + "_ratio"] = res[new + "_ms_median"] / res[old + "_ms_median"]
        res[section + "_pick_frame_range_ms"] = res[old + "_ms_max"] - res[old + "_ms_min"]
        res[section + "_difference_exceeds_pick_frame_range"] = bool(abs(res[new + "_ms_median"] - res[old + "_ms_median"]) > res[section + "_pick_frame_range_ms"])

    def plain_table(nd):
        draws = np.zeros(nd, dtype=capi.draw_dtype)
        st = np.zeros(nd, dtype=capi.draw_state_dtype)
        st["scissor"] = (0, 0, WIDE, WIDE)
        st["clip_first_draw"] = NONE
        return up(draws), up(st), nd

    def queries(pts):
        q = np.zeros(len(pts), dtype=capi.pick_cmd_query_dtype)
        q["x"], q["y"], q["cmd_end"] = [p[0] for p in pts], [p[1] for p in pts], NONE
        q16 = np.zeros(len(pts), dtype=capi.pick_query_dtype)
        q16["x"], q16["y"], q16["mesh_end"] = q["x"], q["y"], NONE
        return q, q16

    hc = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 256)}
    hf = {n: torch.empty(n * 16, dtype=torch.uint8, device=dev) for n in (1, 16, 256)}
    status = torch.zeros(2, dtype=torch.int32, device=dev)

    def section(name, ctx, plain, assembled, pts, dt):
        """plain: (desc, boxes); assembled: (streams, cmds, cap, n, meshes, nm). Times both calls at 1 / 16 / 256 positions."""
        desc, mb = plain
        streams, cmds, cap, n_dev, meshes, nm = assembled
        q, q16 = queries(pts)
        qc, qf = {n: up(q[:n]) for n in (1, 16, 256)}, {n: up(q16[:n]) for n in (1, 16, 256)}

        def commands(n):
            rt.pick_commands(ctx, streams, cmds, cap, qc[n], n, meshes_dev=meshes, num_meshes=nm, dev_num_cmds=n_dev, hits_dev=hc[n], dev_status=status[0:1])

        def frame(n):
            rt.pick_frame(ctx, desc, dt[0], dt[1], dt[2], qf[n], n, mb, hits_dev=hf[n], dev_status=status[1:2])

        if args.trace_only:
            for _ in range(6):
                commands(256)
                frame(256)
            torch.cuda.synchronize()
            return
        calls = {}
        for n in (1, 16, 256):
            calls["%s_q%d_pick_commands" % (name, n)] = (lambda n=n: commands(n))
            calls["%s_q%d_pick_frame" % (name, n)] = (lambda n=n: frame(n))
        alternate(calls)
        for n in (1, 16, 256):
            compare("%s_q%d" % (name, n))
        torch.cuda.synchronize()
        a, b = hc[256].cpu().numpy().view(capi.pick_cmd_hit_dtype), hf[256].cpu().numpy().view(capi.pick_hit_dtype)
        res[name + "_status"] = status.cpu().tolist()
        res[name + "_q256_hits"] = int((a["cmd"] != NONE).sum())
        res[name + "_q256_mesh_and_draw_equal_pick_frame"] = bool(np.array_equal(a["mesh"], b["mesh"]) and np.array_equal(a["draw"], b["draw"]))

    def command_table(ctx, dcmds, cap, num, bufs, nm, dt):
        cmds, n_dev, st = rt.raster_cmds_from_assembly(ctx, dcmds, cap, num, bufs.meshes, nm, dt[1], dt[2])
        torch.cuda.synchronize()
        assert int(st.item()) == 0, int(st.item())
        return cmds, n_dev

    ctx = rt.Context(0)
    ps, d = wl.tiger(1)
    pset = rt.PathSet(ctx, ps)
    dd = rt.upload_draws(d)
    nd = d.shape[0]
    sizes = rt.tessellate_count(ctx, pset, dd, nd)
    nv, ni, nm = sizes["num_vertices"], sizes["num_indices"], sizes["num_meshes"]
    plain = rt.MeshBuffers(dev, nv, ni, nm)
    rt.tessellate_emit(ctx, pset, dd, nd, plain)
    torch.cuda.synchronize()
    res["tiger_meshes"], res["tiger_triangles"] = int(nm), int(ni) // 3

    # ---- one Tiger ---------------------------------------------------------------------------------------------------------------------
    cap = 64
    dcmds = torch.zeros(cap * 48, dtype=torch.uint8, device=dev)
    num = torch.zeros(1, dtype=torch.int64, device=dev)
    asm = rt.MeshBuffers(dev, nv, ni, nm)
    ctx.set_assembly(dcmds, max_vb_vertices=65536, dev_num=num, split_state=True)
    try:
        rt.tessellate_count(ctx, pset, dd, nd)
        rt.tessellate_emit(ctx, pset, dd, nd, asm)
    finally:
        ctx.set_assembly(None)
    torch.cuda.synchronize()
    dt = plain_table(nd)
    cmds, n_dev = command_table(ctx, dcmds, cap, num, asm, nm, dt)
    res["tiger_commands"] = int(n_dev.item())
    desc = capi.CacheDesc(plain.pos.data_ptr(), plain.color.data_ptr(), plain.idx.data_ptr(), plain.meshes.data_ptr(), nm, nv, ni)
    mb = rt.mesh_bounds(ctx, plain.pos, plain.meshes, nm)
    torch.cuda.synchronize()
    box = mb.cpu().numpy()
    lo, hi = box[:, :2].min(axis=0), box[:, 2:].max(axis=0)
    rs = np.random.RandomState(4)
    pts = [(lo[0] + rs.uniform(0.3, 0.7) * (hi[0] - lo[0]), lo[1] + rs.uniform(0.3, 0.7) * (hi[1] - lo[1])) for _ in range(256)]
    streams = rt.raster_streams(asm.pos, asm.color, asm.idx, nv, ni)
    section("tiger", ctx, (desc, mb), (streams, cmds, cap, n_dev, asm.meshes, nm), pts, dt)

    # ---- the grid ------------------------------------------------------------------------------------------------------------------------
    cb = rt.MeshBuffers(dev, nv, ni, nm)
    sizes = rt.tessellate_count(ctx, pset, dd, nd)
    rt.tessellate_emit(ctx, pset, dd, nd, cb)
    cache = rt.MeshCache(ctx, cb, sizes, dd, nd)
    torch.cuda.synchronize()
    cbox = cache.bounds.cpu().numpy()
    clo, chi = cbox[:, :2].min(axis=0), cbox[:, 2:].max(axis=0)
    pitch = 1.25 * float(max(chi - clo))
    k = min(1.0, 65000.0 / (S * pitch))
    inst = np.zeros(S * S, dtype=capi.cache_instance_dtype)
    cell = np.arange(S * S)
    inst["num_meshes"], inst["color"] = cache.nm, 0xFFFFFFFF
    inst["mtx"][:, 0] = inst["mtx"][:, 3] = k
    inst["mtx"][:, 4], inst["mtx"][:, 5] = k * ((cell % S) * pitch - clo[0]), k * ((cell // S) * pitch - clo[1])
    n = S * S
    gv, gi, gm = cache.nv * n, cache.ni * n, cache.nm * n
    inst_dev = up(inst)

    def submit():
        out = rt.MeshBuffers(dev, gv, gi, gm)
        rt.cache_submit(ctx, cache, inst_dev, n, out)
        torch.cuda.synchronize()
        assert int(out.dev_status.item()) == 0, int(out.dev_status.item())
        return out

    gplain = submit()
    gcap = 2 * gv // 65536 + 2 + n
    gdcmds = torch.zeros(gcap * 48, dtype=torch.uint8, device=dev)
    gnum = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.set_assembly(gdcmds, max_vb_vertices=65536, dev_num=gnum, split_state=True)
    try:
        gasm = submit()
    finally:
        ctx.set_assembly(None)
    gdt = plain_table(n)
    gcmds, gn_dev = command_table(ctx, gdcmds, gcap, gnum, gasm, gm, gdt)
    res["grid_scale"], res["grid_meshes"], res["grid_triangles"], res["grid_commands"] = k, gm, gi // 3, int(gn_dev.item())
    gdesc = capi.CacheDesc(gplain.pos.data_ptr(), gplain.color.data_ptr(), gplain.idx.data_ptr(), gplain.meshes.data_ptr(), gm, gv, gi)
    gmb = rt.mesh_bounds(ctx, gplain.pos, gplain.meshes, gm)
    qcell = rs.randint(0, n, 256)
    pts = [(k * ((c % S) * pitch + rs.uniform(0.3, 0.7) * (chi[0] - clo[0])), k * ((c // S) * pitch + rs.uniform(0.3, 0.7) * (chi[1] - clo[1]))) for c in qcell]
    gstreams = rt.raster_streams(gasm.pos, gasm.color, gasm.idx, gv, gi)
    section("grid", ctx, (gdesc, gmb), (gstreams, gcmds, gcap, gn_dev, gasm.meshes, gm), pts, gdt)
    res["scratch_bytes"] = ctx.scratch_bytes()
    pset.close()
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
