"""A/B of two libvgx builds around a change to the command-parallel flatten kernels (k_flatten, k_flatten_build, k_flat1), both loaded
through VGX_LIB in one job on one box; the method of profiles/host_ab.py: a fresh process per item, the variants alternating, the order
swapped every round.
  outputs  every bench.py config (one step): sha256 of each --dump-outputs array and the context's scratch_bytes, per variant; `same`
  timing   stage_times.py cubics / tiger / shuffled (device time of every flatten stage, and the total), the same for cubics with
           VGX_TESS_FLAT1=0 and tiger with VGX_INST=0 VGX_TMPL=0 (k_flatten_build under `flatten_build`), count_timing.py (the two-pass
           count inside vgx_tessellate_count), bench.py --config cubics1m. Per row every run, the medians, the first variant's
           run-to-run range (max - min of its runs) and the verdict: the second variant's median minus the first's does not exceed it.
  python profiles/flatten_chunk_ab.py [--rounds 4] [--mode outputs,timing] --out FILE parent=PATH/libvgx.so head=PATH/libvgx.so"""
import argparse
import ast
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OUTPUTS_WORKER = r"""
import hashlib, importlib, json, os, shutil, sys, tempfile
sys.path.insert(0, %r)
import torch
import bench
rt = importlib.import_module("vg-renderer_amd.runtime")
wl = importlib.import_module("vg-renderer_amd.workloads")
base = dict(os.environ)
for name in sorted(k for k in bench.WORKLOADS if k != "tiger10k_animated"):
    os.environ.clear(); os.environ.update(base); os.environ.update(bench.CONFIG_ENV.get(name, {}))  # library options are read at vgx_create
    ps, d, _, kind = bench.make_workload(wl, name, 10000, 0)
    ctx = rt.Context(0)
    tmp = tempfile.mkdtemp()
    res = bench.run_config(rt, torch, ctx, 0, name, ps, d, kind, 1, 1, torch.cuda.synchronize, full=False, dump_dir=tmp)
    sha = {f: hashlib.sha256(open(os.path.join(tmp, f), "rb").read()).hexdigest()[:16] for f in sorted(os.listdir(tmp))}
    print("AB " + json.dumps({"config": name, "scratch_bytes": ctx.scratch_bytes(), "sha256": sha}), flush=True)
    shutil.rmtree(tmp)
    res["pset"].close(); del res; ctx.close()
""" % ROOT


def run(cmd, lib, knobs=None):
    env = dict(os.environ, VGX_LIB=os.path.abspath(lib), PYTHONPATH=ROOT, **(knobs or {}))
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (cmd, r.returncode, r.stdout[-400:]))
    return r.stdout


def outputs(lib):
    return {j["config"]: j for j in (json.loads(ln[3:]) for ln in run([sys.executable, "-c", OUTPUTS_WORKER], lib).splitlines() if ln.startswith("AB "))}


def timing_items():
    def stages(which, label=None, knobs=None):
        def f(lib):
            out = run([sys.executable, "profiles/stage_times.py", which], lib, knobs).strip().splitlines()[-1]
            d = ast.literal_eval(out[out.index("{"):])
            m = {"%s_%s_ms" % (label or which, k): v for k, v in d.items() if "flatten" in k}
            m["%s_total_ms" % (label or which)] = sum(d.values())
            return m
        return f

    def count(lib):
        ms = ast.literal_eval(re.search(r"ms per call (\[[^\]]*\])", run([sys.executable, "profiles/count_timing.py"], lib)).group(1))
        return {"tessellate_count_1m_cubics_ms": statistics.median(ms[1:])}  # (the first call sizes the scratch)

    def cubics1m(lib):
        line = json.loads(run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2", "--config", "cubics1m", "--no-configs", "--no-cpu"], lib).strip().splitlines()[-1])
        return {"bench_cubics1m_ms_per_step": line["ms_per_step"]}
    # the default routes of cubics / tiger / shuffled are k_flat1, the template and k_flatten_inst: k_flatten_build's own rows take knobs
    return [stages("cubics"), stages("tiger"), stages("shuffled"), stages("cubics", "cubics_heap_route", {"VGX_TESS_FLAT1": "0"}),
            stages("tiger", "tiger_command_parallel", {"VGX_INST": "0", "VGX_TMPL": "0"}), count, cubics1m]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--mode", default="outputs,timing")
    ap.add_argument("--out", default=None)
    ap.add_argument("variants", nargs=2, help="NAME=PATH of libvgx.so; the first is the one whose spread is the margin")
    args = ap.parse_args()
    variants = [v.split("=", 1) for v in args.variants]
    a, b = variants[0][0], variants[1][0]
    res = {"variants": [a, b], "order": "alternating, fresh process per item, swapped every round"}
    if "outputs" in args.mode:
        oa, ob = outputs(variants[0][1]), outputs(variants[1][1])
        res["outputs"] = {k: {a: oa[k], b: ob.get(k), "same": ob.get(k) == oa[k]} for k in oa}
        print("outputs: %d configs, %d the same (arrays and scratch_bytes)" % (len(oa), sum(v["same"] for v in res["outputs"].values())), flush=True)
    if "timing" in args.mode:
        runs = {a: {}, b: {}}
        for r in range(args.rounds):
            for item in timing_items():
                for name, lib in (variants if r % 2 == 0 else variants[::-1]):
                    for k, x in item(lib).items():
                        runs[name].setdefault(k, []).append(x)
            print("round %d done" % r, flush=True)
        res["rounds"] = args.rounds
        res["timing"] = {}
        for k in runs[a]:
            xa, xb = runs[a][k], runs[b][k]
            row = {a: {"runs": xa, "median": statistics.median(xa)}, b: {"runs": xb, "median": statistics.median(xb)}, "range_of_" + a: max(xa) - min(xa)}
            row["passes"] = row[b]["median"] - row[a]["median"] <= row["range_of_" + a]
            res["timing"][k] = row
            print("%-36s %s %.4f (range %.4f)   %s %.4f   %s" % (k, a, row[a]["median"], row["range_of_" + a], b, row[b]["median"], "passes" if row["passes"] else "FAILS"), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
