"""Host-time A/B of two libvgx builds (a change of host code only: kernels are the same, so the host path is what is timed).
Variants run round-robin, each item in a fresh process (VGX_LIB is read at import), the procedure of profiles/ab_run.py. Items:
call_latency (profiles/call_latency.py, back-to-back x1 / x10 / x100), the static-batch frame (bench.py's frame_leg), bench.py's
headline step, immediate_timing.py's steady-state call (host and device clock). Per item and variant: every run, min, median, max;
`inside` says whether the median of the second variant lies within the first variant's own min .. max of this job.
  python profiles/host_ab.py --rounds 4 [--items latency,frame,bench,immediate] --out FILE parent=PATH/libvgx.so head=PATH/libvgx.so"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import importlib, json, os, sys
sys.path.insert(0, %r)
import torch
import bench
rt = importlib.import_module("vg-renderer_amd.runtime")
ctx = rt.Context(0)
fr = bench.frame_leg(rt, torch, ctx, 0)
print("AB " + json.dumps({"frame_tiger_x1_us_static_batch": fr.get("static_tessellate_assembled_us_back_to_back"),
                          "frame_tiger_x1_us_back_to_back": fr.get("tessellate_assembled_us_back_to_back")}))
""" % ROOT


def run(cmd, env):
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (cmd, r.returncode, r.stdout[-400:]))
    return r.stdout


def measure(lib, items):
    env = dict(os.environ, VGX_LIB=lib)
    m = {}
    if "latency" in items:
        for k, us in re.findall(r"tiger x(\d+): ([0-9.]+) us per call back-to-back", run([sys.executable, "profiles/call_latency.py"], env)):
            m["call_latency_x%s_us" % k] = float(us)
    if "frame" in items:
        out = run([sys.executable, "-c", WORKER], env)
        m.update(json.loads([ln for ln in out.splitlines() if ln.startswith("AB ")][-1][3:]))
    if "bench" in items:
        line = json.loads(run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"], env).strip().splitlines()[-1])
        m["bench_headline_ms_per_step"] = line["ms_per_step"]
    if "immediate" in items:
        imm = json.loads(run([sys.executable, "profiles/immediate_timing.py", "--legs-only", "--steps", "20"], env).strip().splitlines()[-1])
        m["immediate_host_us"] = imm["immediate_host_ms"] * 1e3
        m["immediate_ms"] = imm["immediate_ms"]
        m["hot_host_us"] = imm["hot_host_ms"] * 1e3
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--items", default="latency,frame,bench,immediate")
    ap.add_argument("variants", nargs=2, help="NAME=PATH of libvgx.so; the first is the one whose spread is the margin")
    args = ap.parse_args()
    variants = [v.split("=", 1) for v in args.variants]
    runs = {name: {} for name, _ in variants}
    for r in range(args.rounds):
        for name, lib in (variants if r % 2 == 0 else variants[::-1]):
            for k, x in measure(os.path.abspath(lib), args.items.split(",")).items():
                runs[name].setdefault(k, []).append(x)
            print("round %d %s done" % (r, name), flush=True)
    a, b = variants[0][0], variants[1][0]
    res = {"rounds": args.rounds, "order": "alternating, fresh process per item", "measured": args.items, "items": {}}
    for k in runs[a]:
        xa, xb = runs[a][k], runs[b][k]
        res["items"][k] = {a: {"runs": xa, "min": min(xa), "median": statistics.median(xa), "max": max(xa)},
                           b: {"runs": xb, "min": min(xb), "median": statistics.median(xb), "max": max(xb)},
                           "inside": min(xa) <= statistics.median(xb) <= max(xa)}
        print("%-36s %s %.3f .. %.3f .. %.3f   %s median %.3f   %s" % (k, a, min(xa), statistics.median(xa), max(xa), b, statistics.median(xb),
                                                                         "inside" if res["items"][k]["inside"] else "OUTSIDE"), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
