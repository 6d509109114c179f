"""Immediate mode against the counted calls, on the device's clock (HIP events around K back-to-back calls, no sync in between).

  immediate       vgx_tessellate_immediate, one context, two Tiger x10k batches of equal size alternating: the same draws in two
                  different random orders (changing content: every call is a batch the last call did not have). No period, but every
                  path is used by 10 000 draws: both calls here and the counted calls take the grouped instanced flatten (draws sorted
                  by path, k_flatten_inst)
  hot             vgx_tessellate on a counted batch (the steady state of a caller whose content does not change)
  count_emit      vgx_tessellate_count + vgx_tessellate_emit per batch, the two batches alternating (what changing content cost before)
  frame316_*      a 316-draw frame: immediate against vgx_tessellate on the counted frame
  uninstanced.*   the same three legs with VGX_INST=0 (no instancing at all: k_flatten_build, bench.py's tiger10k_command_parallel), in a
                  child process

python profiles/immediate_timing.py [--steps K] [--out FILE]   (prints one JSON object)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--instances", type=int, default=10000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs-only", action="store_true", help="the three Tiger legs only (the child process of the VGX_INST=0 run)")
    args = ap.parse_args()
    import numpy as np
    import torch
    rt = importlib.import_module("vg-renderer_amd.runtime")
    wl = importlib.import_module("vg-renderer_amd.workloads")
    K = args.steps

    def timed(fn, k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(k):
            fn(i)
        e1.record()
        host = (time.perf_counter() - t0) * 1e3 / k
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k, host

    ps, d = wl.tiger(args.instances)
    X = d[np.random.RandomState(1).permutation(d.shape[0])]
    Y = d[np.random.RandomState(2).permutation(d.shape[0])]
    res = {"ndraws": int(d.shape[0]), "steps": K, "flatten": "grouped instanced (k_flatten_inst)" if os.environ.get("VGX_INST", "1") != "0" else "k_flatten_build (VGX_INST=0)"}
    ctx = rt.Context(0)
    pset = rt.PathSet(ctx, ps)
    dx, dy = rt.upload_draws(X), rt.upload_draws(Y)
    n = d.shape[0]
    # immediate, changing content
    r, bufs = rt.tessellate_grow(ctx, pset, dx, n)
    r2, bufs = rt.tessellate_grow(ctx, pset, dy, n, bufs)
    res["immediate_first_calls"] = [r.statuses, r2.statuses]
    for i in range(4):
        rt.tessellate_immediate(ctx, pset, dx if i % 2 == 0 else dy, n, bufs)
    torch.cuda.synchronize()
    assert int(bufs.dev_status.item()) == 0
    res["immediate_ms"], res["immediate_host_ms"] = timed(lambda i: rt.tessellate_immediate(ctx, pset, dx if i % 2 == 0 else dy, n, bufs), K)
    assert int(bufs.dev_status.item()) == 0
    # hot vgx_tessellate on a counted batch
    rt.tessellate_count(ctx, pset, dx, n)
    for _ in range(3):
        rt.tessellate_async(ctx, pset, dx, n, bufs)
    res["hot_ms"], res["hot_host_ms"] = timed(lambda i: rt.tessellate_async(ctx, pset, dx, n, bufs), K)
    assert int(bufs.dev_status.item()) == 0

    # count + emit, alternating
    def count_emit(i):
        dd = dx if i % 2 == 0 else dy
        rt.tessellate_count(ctx, pset, dd, n)
        rt.tessellate_emit(ctx, pset, dd, n, bufs)
    count_emit(0)
    res["count_emit_ms"], res["count_emit_host_ms"] = timed(count_emit, K)
    res["immediate_vs_hot"] = res["immediate_ms"] / res["hot_ms"]
    res["immediate_vs_count_emit"] = res["immediate_ms"] / res["count_emit_ms"]
    if args.legs_only:
        print(json.dumps(res))
        pset.close()
        ctx.close()
        return
    import subprocess
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--legs-only", "--steps", str(K), "--instances", str(args.instances)],
                           env=dict(os.environ, VGX_INST="0"), stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    res["uninstanced"] = json.loads(child.stdout.strip().splitlines()[-1])
    # a 316-draw frame
    fps, fd = wl.tiger(2)
    fd = fd[:316]
    fset = rt.PathSet(ctx, fps)
    dfr = rt.upload_draws(fd)
    r, fb = rt.tessellate_grow(ctx, fset, dfr, 316)
    for _ in range(3):
        rt.tessellate_immediate(ctx, fset, dfr, 316, fb)
    res["frame316_immediate_ms"], res["frame316_immediate_host_ms"] = timed(lambda i: rt.tessellate_immediate(ctx, fset, dfr, 316, fb), 4 * K)
    assert int(fb.dev_status.item()) == 0
    rt.tessellate_count(ctx, fset, dfr, 316)
    for _ in range(3):
        rt.tessellate_async(ctx, fset, dfr, 316, fb)
    res["frame316_hot_ms"], res["frame316_hot_host_ms"] = timed(lambda i: rt.tessellate_async(ctx, fset, dfr, 316, fb), 4 * K)
    assert int(fb.dev_status.item()) == 0
    res["frame316_delta_us"] = (res["frame316_immediate_ms"] - res["frame316_hot_ms"]) * 1e3
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    fset.close()
    pset.close()
    ctx.close()


if __name__ == "__main__":
    main()
