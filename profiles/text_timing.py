"""vgx_text_quads on the device's clock, one job on one box.

  stream_*    (a) 16 M glyph quads in runs of 8 .. 120, dense placement, int16 and float UVs: ms per call (HIP events around K
              back-to-back calls after warm-up) and (bytes read + bytes written) / time. Bytes counted from the shapes: 32 per quad
              read, 76 / 92 per quad written (positions 32, colours 16, UVs 16 / 32, indices 12), 80 read + 32 written per run.
  writebw_*   (b) profiles/micro/writebw.hip's three-stream figures from this job: what this memory system gives a kernel that
              only stores -- the ceiling (a) is judged against (stream_*_vs_writebw).
  ref_*       (c) the reference's loops on 1 M quads on one core: vgutil::batchTransformTextQuads + the UV loop of
              renderTextQuads restated in numpy + vgutil::genQuadIndices_unaligned through ctypes (oracle/_ref/libvgref.so).
  frame_*     (d) one 316-draw Tiger frame plus 4 000 glyph quads in 80 runs: microseconds for vgx_text_quads alone, and for the frame
              (vgx_tessellate_immediate + vgx_merge_uv with assembly armed) with and without the text. Reported, not judged: at this size the call
              is launch latency.

python profiles/text_timing.py [--steps K] [--quads N] [--out FILE]   (prints one JSON object)"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def writebw():
    """Build (if needed) and run profiles/micro/writebw.hip; the three-stream lines as {name: TB/s}."""
    src = os.path.join(ROOT, "profiles", "micro", "writebw.hip")
    exe = os.path.join(ROOT, "profiles", "micro", "writebw.bin")
    if not os.path.exists(exe):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=300, check=True).stdout
    res = {}
    for m in re.finditer(r"write3 \(.*misaligned=(\d)\) grid=(\d+): *([\d.]+) ms +([\d.]+) TB/s", out):
        res["write3_mis%s_grid%s_TBps" % (m.group(1), m.group(2))] = float(m.group(4))
    for m in re.finditer(r"write grid=(\d+) +(\d+) B/lane: *([\d.]+) ms +([\d.]+) TB/s", out):
        res["write1_%sB_grid%s_TBps" % (m.group(2), m.group(1))] = float(m.group(4))
    return res


def make_runs(capi, rt, np, rng, counts):
    n = len(counts)
    runs = np.zeros(n, capi.text_run_dtype)
    runs["num_quads"] = counts
    runs["first_quad"] = np.cumsum(counts) - counts
    ang = rng.uniform(-3.0, 3.0, n)
    runs["mtx"][:, 0], runs["mtx"][:, 1], runs["mtx"][:, 2], runs["mtx"][:, 3] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    runs["mtx"][:, 4], runs["mtx"][:, 5] = rng.uniform(0, 1000, n), rng.uniform(0, 700, n)
    runs["x"], runs["y"], runs["dx"], runs["dy"] = rng.uniform(0, 900, n), rng.uniform(0, 600, n), rng.uniform(-100, 0, n), rng.uniform(-10, 10, n)
    runs["scale"] = np.round(rng.uniform(0.5, 3.0, n), 1)
    runs["color"] = 0xFFFFFFFF
    runs["draw"] = np.arange(n)
    rt.text_runs_dense(runs)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--quads", type=int, default=16 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    capi = rt.capi
    K = max(args.steps, 20)
    dev = torch.device("cuda", 0)
    res = {"box": torch.cuda.get_device_name(0), "steps": K}

    def timed(fn, k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(k):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    res.update({"writebw_" + k: v for k, v in writebw().items()})
    ceiling = max(v for k, v in res.items() if k.startswith("writebw_write3_mis0"))
    res["writebw_ceiling_TBps"] = ceiling

    ctx = rt.Context(0)
    rng = np.random.default_rng(1)
    # (a) the stream
    counts = []
    total = 0
    while total < args.quads:
        c = rng.integers(8, 121, 4096)
        counts.append(c)
        total += int(c.sum())
    counts = np.concatenate(counts)
    counts = counts[:int(np.searchsorted(np.cumsum(counts), args.quads)) + 1]
    runs = make_runs(capi, rt, np, rng, counts)
    nq, nr = int(counts.sum()), int(counts.shape[0])
    quads = torch.rand((nq, 8), dtype=torch.float32, device=dev)
    rd = torch.from_numpy(runs.view(np.uint8).copy()).to(dev)
    bufs = rt.MeshBuffers(dev, 4 * nq, 6 * nq, nr)
    res["stream_quads"], res["stream_runs"] = nq, nr
    for name, ub, dt in (("int16", 4, torch.int16), ("float", 8, torch.float32)):
        uv = torch.empty((4 * nq, 2), dtype=dt, device=dev)
        for _ in range(3):
            rt.text_quads(ctx, quads, nq, rd, nr, bufs, uv_dev=uv, uv_bytes=ub)
        torch.cuda.synchronize()
        assert int(bufs.dev_status.item()) == 0
        ms = min(timed(lambda i: rt.text_quads(ctx, quads, nq, rd, nr, bufs, uv_dev=uv, uv_bytes=ub), K) for _ in range(3))
        moved = nq * (32 + 60 + 4 * ub) + nr * (80 + 32)
        res["stream_%s_ms" % name] = ms
        res["stream_%s_bytes" % name] = moved
        res["stream_%s_TBps" % name] = moved / ms / 1e9
        res["stream_%s_vs_writebw" % name] = moved / ms / 1e9 / ceiling
        del uv
    del quads, bufs, rd

    # (c) the reference's loops, one core
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libvgref.so"))
    bt = getattr(lib, "_ZN6vgutil23batchTransformTextQuadsEPKfjS1_Pf")
    gq = getattr(lib, "_ZN6vgutil24genQuadIndices_unalignedEPtjt")
    bt.restype = gq.restype = None
    bt.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    gq.argtypes = [C.c_void_p, C.c_uint32, C.c_uint16]
    n1 = 1 << 20
    c1 = rng.integers(8, 121, n1 // 64 + 64)
    c1 = c1[:int(np.searchsorted(np.cumsum(c1), n1))]
    q1 = rng.uniform(0, 1, (int(c1.sum()), 8)).astype(np.float32)
    pos, idx, uvo = np.zeros((4 * q1.shape[0], 2), np.float32), np.zeros(6 * q1.shape[0], np.uint16), np.zeros((4 * q1.shape[0], 2), np.int16)
    m = np.asarray([0.8, 0.6, -0.6, 0.8, 10, 20], np.float32)
    first = np.cumsum(c1) - c1
    t0 = time.perf_counter()
    for a, n in zip(first.tolist(), c1.tolist()):
        bt(q1.ctypes.data + 32 * a, n, m.ctypes.data, pos.ctypes.data + 32 * a)
        gq(idx.ctypes.data + 12 * a, n, 0)
    t1 = time.perf_counter()
    uvo[:] = (q1[:, [4, 5, 6, 5, 6, 7, 4, 7]].reshape(-1, 2) * np.float32(32767)).astype(np.int32)
    t2 = time.perf_counter()
    res["ref_quads"] = int(q1.shape[0])
    res["ref_transform_indices_ms"] = (t1 - t0) * 1e3   # includes one ctypes call pair per run
    res["ref_uv_numpy_ms"] = (t2 - t1) * 1e3
    res["ref_Mquads_per_s"] = q1.shape[0] / (t2 - t0) / 1e6

    # (d) a 316-draw frame + 4 000 glyph quads
    fps, fd = wl.tiger(2)
    fd = fd[:316].copy()
    fset = rt.PathSet(ctx, fps)
    c4 = np.full(80, 50, np.int64)
    r4 = make_runs(capi, rt, np, rng, c4)
    r4["draw"] = 316 + np.arange(80)
    q4 = torch.rand((4000, 8), dtype=torch.float32, device=dev)
    rd4 = torch.from_numpy(r4.view(np.uint8).copy()).to(dev)
    B = rt.MeshBuffers(dev, 16000, 24000, 80)
    buv = torch.empty((16000, 2), dtype=torch.int16, device=dev)
    for _ in range(5):
        rt.text_quads(ctx, q4, 4000, rd4, 80, B, uv_dev=buv, uv_bytes=4)
    res["frame_text_quads_us"] = timed(lambda i: rt.text_quads(ctx, q4, 4000, rd4, 80, B, uv_dev=buv, uv_bytes=4), 8 * K) * 1e3
    assert int(B.dev_status.item()) == 0
    # the frame's draw table: the 316 Tiger draws + 80 text draws behind them
    draws = np.zeros(396, capi.draw_dtype)
    draws[:316] = fd
    draws["fill_flags"][316:] = capi.FILL_TEXT
    draws["mtx"][316:, 0] = draws["mtx"][316:, 3] = 1.0
    draws["scale"][316:], draws["tess_tol"][316:], draws["fringe"][316:] = 1.0, 0.25, 1.0
    dd = rt.upload_draws(draws)
    r, A = rt.tessellate_grow(ctx, fset, dd, 396)   # immediate mode: the frame is never counted
    sa = r.sizes
    nv, ni, nm = sa["num_vertices"] + 16000, sa["num_indices"] + 24000, sa["num_meshes"] + 80
    out = rt.MeshBuffers(dev, nv, ni, nm)
    cmds = torch.zeros((nm + 2) * 48, dtype=torch.uint8, device=dev)
    ncmd = torch.zeros(1, dtype=torch.int64, device=dev)
    uvs = torch.zeros((nv, 2), dtype=torch.int16, device=dev)
    seq_a = rt.mesh_seq(A, sa["num_vertices"], sa["num_indices"], sa["num_meshes"])
    seq_b = rt.mesh_seq(B, 16000, 24000, 80)
    seq_0 = rt.mesh_seq(B, 0, 0, 0)

    def frame(text):
        ctx.set_assembly(None)   # (a host-side switch) sequence A is assembled by the merge, not by the tessellator
        rt.tessellate_immediate(ctx, fset, dd, 396, A)
        ctx.set_assembly(cmds, 65536, ncmd, split_state=True, uv=uvs, uv_value=(0, 0))
        if text:
            rt.text_quads(ctx, q4, 4000, rd4, 80, B, uv_dev=buv, uv_bytes=4)
            rt.merge(ctx, seq_a, seq_b, None, dd, 396, out, b_uv_dev=buv)
        else:
            rt.merge(ctx, seq_a, seq_0, None, dd, 396, out)
    try:
        for t in (True, False):
            for _ in range(5):
                frame(t)
            torch.cuda.synchronize()
            assert int(out.dev_status.item()) == 0, int(out.dev_status.item())
            res["frame_with_text_us" if t else "frame_without_text_us"] = timed(lambda i: frame(t), 4 * K) * 1e3
    finally:
        ctx.set_assembly(None)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    fset.close()
    ctx.close()


if __name__ == "__main__":
    main()
