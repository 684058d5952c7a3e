#!/usr/bin/env python3
"""Collect the per-round evidence under profiles/ on an MI355X box (run from the repo root):

    python tools/collect_profiles.py r01 gpurun_out/profiles_new

  <tag>_bench.json                  python bench.py --full               (all extras: cpu baseline, sweep, in-run traffic)
  <tag>_bench_single_stream.json    python bench.py --no-pipeline --no-extras
  <tag>_bench_config5.json / _config3.json     python bench.py --config 5 --full / --config 3
  <tag>_bench_frame_loop.json / _bench_config4_1gpu(_autocast|_bf16).json   python bench.py --config loop / --config 4 [--autocast|--bf16]
  <tag>_kernel_stats_config4(_autocast|_bf16).csv   rocprofv3 --kernel-trace --stats of the same three settings of config 4
  <tag>_bench_dropin.json           python bench.py --config dropin --steps 200   (wall vs device per call of the drop-in)
  <tag>_kernel_stats.csv            rocprofv3 --kernel-trace --stats  -- python bench.py --no-extras
  <tag>_kernel_stats_single_stream.csv / _config5.csv / _config3.csv   same with --no-pipeline / --config 5 / --config 3
  <tag>_pmc_traffic.json            two separate --pmc passes (FETCH_SIZE, WRITE_SIZE), per-kernel averages;
                                    bytes = KiB * 1024, FETCH x 2 (gfx950 correction, MI355X_MICROARCH.md HBM section)
  <tag>_agent_info.csv
rocprofv3 runs from /tmp with TMPDIR=/tmp; --pmc is never combined with other trace domains than --kernel-trace.
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

tag, out = sys.argv[1], os.path.abspath(sys.argv[2])
only_pmc = len(sys.argv) > 3 and sys.argv[3] == "pmc"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.makedirs(out, exist_ok=True)
env = dict(os.environ, TMPDIR="/tmp")
bench = [sys.executable, os.path.join(root, "bench.py")]


def run(cmd, **kw):
    return subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, **kw)


def last_json(stdout):
    return [l for l in stdout.strip().splitlines() if l.startswith("{")][-1]


if not only_pmc and os.environ.get("ONLY_STATS") is None:
    open(os.path.join(out, f"{tag}_bench.json"), "w").write(last_json(run(bench + ["--full"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_single_stream.json"), "w").write(
        last_json(run(bench + ["--no-pipeline", "--no-extras"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_config5.json"), "w").write(
        last_json(run(bench + ["--config", "5", "--full", "--no-cpu-baseline"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_config3.json"), "w").write(
        last_json(run(bench + ["--config", "3"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_frame_loop.json"), "w").write(
        last_json(run(bench + ["--config", "loop"]).stdout) + "\n")
    # config 4: the reference's precision (fp32 encoder, the default) and the bf16-autocast variant; 3 repeats of 8 steps
    open(os.path.join(out, f"{tag}_bench_config4_1gpu.json"), "w").write(
        last_json(run(bench + ["--config", "4", "--steps", "8", "--warmup", "2"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_config4_1gpu_autocast.json"), "w").write(
        last_json(run(bench + ["--config", "4", "--steps", "8", "--warmup", "2", "--autocast"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_config4_1gpu_bf16.json"), "w").write(
        last_json(run(bench + ["--config", "4", "--steps", "8", "--warmup", "2", "--bf16"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_dropin.json"), "w").write(
        last_json(run(bench + ["--config", "dropin", "--steps", "200"]).stdout) + "\n")
    open(os.path.join(out, f"{tag}_bench_train.json"), "w").write(
        last_json(run(bench + ["--config", "train", "--steps", "40", "--warmup", "6"]).stdout) + "\n")

only = os.environ.get("ONLY_STATS")                       # e.g. ONLY_STATS=_config3: just that kernel-stats pass
for suffix, extra in (() if only_pmc else (("", []), ("_single_stream", ["--no-pipeline"]), ("_config5", ["--config", "5"]),
                                           ("_config3", ["--config", "3", "--steps", "50"]),
                                           ("_frame_loop", ["--config", "loop"]),
                                           ("_train", ["--config", "train", "--frames", "512", "--steps", "16", "--warmup", "4"]),
                                           # config 4's step, kernel by kernel: the reference's fp32 setting, stock bf16
                                           # autocast, and the shipped bf16 training form
                                           ("_config4", ["--config", "4", "--steps", "4", "--warmup", "1", "--repeats", "1", "--settle", "3"]),
                                           ("_config4_autocast", ["--config", "4", "--steps", "4", "--warmup", "1", "--repeats", "1",
                                                                  "--settle", "3", "--autocast"]),
                                           ("_config4_bf16", ["--config", "4", "--steps", "4", "--warmup", "1", "--repeats", "1",
                                                              "--settle", "3", "--bf16"]))):
    if only is not None and suffix != only:
        continue
    d = f"/tmp/prof_stats{suffix}"
    shutil.rmtree(d, ignore_errors=True)
    if suffix in ("_config3", "_frame_loop"):
        # MIOpen's find step (GraphedEncoder(miopen_find=True), first forward of the process) times every applicable
        # solver once, its reference `naive_conv_*` kernels included: 128 calls of 4.8 ms = 83 % of the summary.  For
        # THIS profile only they are taken out of the candidates (the timed encoder is the same with and without:
        # 1.119 / 1.122 ms); the product leaves the variable alone -- with it the shipped find-db no longer matched
        # the frame-loop shapes and the live search picked slower kernels (2.09 -> 2.15-2.49 ms per frame step).
        env["MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD"] = "0"
    else:
        env.pop("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", None)
    if suffix.startswith("_config4"):
        # (under rocprofv3 MIOpen searched some of config 4's problems again although the shipped find-db holds them -- its
        # reference kernels, 9-125 ms each, then bury the step in the summary; for THESE profiles they leave the candidates)
        for d_ in ("FWD", "BWD", "WRW"):
            env["MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + d_] = "0"
    else:
        for d_ in ("BWD", "WRW"):
            env.pop("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + d_, None)
    run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + bench +
        ["--no-extras"] + extra)
    for f in glob.glob(d + "/**/*_kernel_stats.csv", recursive=True):
        shutil.copy(f, os.path.join(out, f"{tag}_kernel_stats{suffix}.csv"))
    for f in glob.glob(d + "/**/*_agent_info.csv", recursive=True):
        shutil.copy(f, os.path.join(out, f"{tag}_agent_info.csv"))

if os.environ.get("ONLY_STATS") is not None:
    sys.exit(0)
kernels = {}
for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
    d = f"/tmp/prof_{ctr}"
    shutil.rmtree(d, ignore_errors=True)
    run(["rocprofv3", "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--"] + bench +
        ["--steps", "3", "--warmup", "1", "--no-extras"])
    for f in glob.glob(d + "/**/*_counter_collection.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].split("(")[0]
            name = name[5:] if name.startswith("void ") else name
            if not name.startswith("dmm::") or row["Counter_Name"] != ctr:
                continue
            k = kernels.setdefault(name, {})
            k.setdefault(ctr, []).append(float(row["Counter_Value"]))
res = {"round": tag,
       "command": "rocprofv3 --kernel-trace --pmc FETCH_SIZE|WRITE_SIZE --output-format csv -- python bench.py --steps 3 "
                  "--warmup 1 --no-cpu-baseline (separate passes; default 2-lane schedule: 512 frames per cost launch)",
       "units": "counter values are KiB (rocprofv3 FETCH_SIZE / WRITE_SIZE); bytes = value * 1024",
       "gfx950_correction": "FETCH_SIZE reports 1/2 of the bytes of a wide coalesced streaming read on gfx950 "
                            "(MI355X_MICROARCH.md, HBM section) -> read bytes = FETCH_SIZE * 1024 * 2; WRITE_SIZE used "
                            "as is (uncalibrated)",
       "kernels": {}}
for name, k in kernels.items():
    f, w = k.get("FETCH_SIZE", []), k.get("WRITE_SIZE", [])
    fa, wa = (sum(f) / len(f) if f else 0.0), (sum(w) / len(w) if w else 0.0)
    res["kernels"][name] = {"FETCH_SIZE_KiB_avg": fa, "FETCH_SIZE_samples": len(f), "WRITE_SIZE_KiB_avg": wa,
                            "WRITE_SIZE_samples": len(w), "hbm_bytes_per_launch": int(fa * 1024 * 2 + wa * 1024)}
cost = [v for n, v in res["kernels"].items() if n.startswith("dmm::iou_counts_kernel")]
if cost:
    res["hbm_bytes_per_launch_at_frames"] = {"512": cost[0]["hbm_bytes_per_launch"]}
    res["algorithmic_bytes_per_launch_at_frames"] = {"512": 512 * (60 * 65025 * 4 + 2000)}
json.dump(res, open(os.path.join(out, f"{tag}_pmc_traffic.json"), "w"), indent=1)
# the training form of the layer (bench.py --config train, 512 frames): the same two passes
tk = {}
for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
    d = f"/tmp/prof_train_{ctr}"
    shutil.rmtree(d, ignore_errors=True)
    run(["rocprofv3", "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", d, "--"] + bench +
        ["--config", "train", "--frames", "512", "--steps", "4", "--warmup", "2"])
    for f in glob.glob(d + "/**/*_counter_collection.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].split("(")[0]
            name = name[5:] if name.startswith("void ") else name
            if not name.startswith("dmm::") or row["Counter_Name"] != ctr:
                continue
            tk.setdefault(name, {}).setdefault(ctr, []).append(float(row["Counter_Value"]))
tres = {"round": tag, "command": "rocprofv3 --kernel-trace --pmc FETCH_SIZE|WRITE_SIZE -- python bench.py --config train "
                                 "--frames 512 --steps 4 --warmup 2 (separate passes)",
        "units": res["units"], "gfx950_correction": res["gfx950_correction"], "kernels": {}}
for name, k in tk.items():
    f, w = k.get("FETCH_SIZE", []), k.get("WRITE_SIZE", [])
    fa, wa = (sum(f) / len(f) if f else 0.0), (sum(w) / len(w) if w else 0.0)
    tres["kernels"][name] = {"FETCH_SIZE_KiB_avg": fa, "WRITE_SIZE_KiB_avg": wa, "samples": len(f),
                             "hbm_bytes_per_launch": int(fa * 1024 * 2 + wa * 1024)}
json.dump(tres, open(os.path.join(out, f"{tag}_pmc_traffic_train.json"), "w"), indent=1)
print(json.dumps({n: v["hbm_bytes_per_launch"] for n, v in res["kernels"].items()}, indent=1))
if not only_pmc:
    print(open(os.path.join(out, f"{tag}_bench.json")).read())
