"""Measurement of the batched AdGD optimizer (dzo_adgd_batch_*, csrc/dzo_adgd_batch.hip) on the device: recorded, not gated.

    python tools/bench_adgd_batch.py [--out profiles/adgd_batch_bench.json] [--repeats 5] [--baseline-count 256]

Workload: the tempered replicas of tools/bench_quench.py (256 replicas of an N-particle Lennard-Jones cluster, fixed seed,
20 batches of 500 steps); a device-to-device copy is quenched by ONE BatchedAdGD handle (step 0.01, 50 step!() calls per launch,
the host asking `all stuck?` after every launch) until every instance is stuck.  N = 38 and 13 (WAVE shape) and N = 200 (BLOCK),
fp64 and fp32.  After a warm-up quench of the same size, `repeats` quenches of fresh copies are timed twice over: by the
library's HIP events around every launch (dzo_profile_*: the device time) and by the host clock around create + the launches +
the last wait (what a caller sees).  Reported as in tools/bench_quench.py: median and range of the total time, instance-step!()
calls per second, the distribution of steps to stuck, and the register and LDS figures of the kernels from the code object.

Baseline: the only path the parent commit offers -- the same 256 starting points, each through its own dzo_adgd_* optimizer on a
DZO_PROBLEM_PAIRWISE_LJ handle, one after the other, until stuck (N = 38, fp64; `baseline-count` of them, the rest extrapolated
by the mean when fewer than 256 are run).  This commit does not touch dzo_adgd.hip, dzo_problems.hip or dzo_pairwise.hip, so the
baseline run in this tree is the parent's.  For information, the BatchedLBFGS quench of the same starts (steps and time).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_quench as bq  # noqa: E402

REPLICAS = bq.REPLICAS
STEPS_PER_LAUNCH, MAX_STEPS = 50, 200000


def quench_once(dzo, replicas, n):
    """(host seconds, device ms of the launches, step launches, optimizer) of one quench of a fresh copy"""
    copy = replicas.copy()
    dzo.synchronize()
    dzo.profile_reset()
    t0 = time.perf_counter()
    opt = dzo.BatchedAdGD(copy, n, 0.01)
    done, taken = False, 0
    while not done and taken < MAX_STEPS:
        done = opt.step(STEPS_PER_LAUNCH)
        taken += STEPS_PER_LAUNCH
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    launches, step_ms = table["adgd_batch_step"][0], table["adgd_batch_step"][1]
    return wall, step_ms + table["adgd_batch_init"][1], launches, opt


def device_case(dzo, n, dtype, repeats):
    replicas = bq.tempered_replicas(dzo, n, dtype)
    e_start = dzo.pairwise_batch_energy_gradient(replicas, n)
    dzo.profile_enable(2)
    quench_once(dzo, replicas, n)                            # warm-up pass of the same size
    walls, devs = [], []
    for _ in range(repeats):
        wall, dev_ms, launches, opt = quench_once(dzo, replicas, n)
        walls.append(wall * 1e3); devs.append(dev_ms)
    counts = opt.iteration_counts
    f = opt.current_objective_values.astype(np.float64)
    total = int(counts.sum())
    wall_ms, dev_ms = float(np.median(walls)), float(np.median(devs))
    srt = np.sort(f)
    row = {"n": n, "dtype": np.dtype(dtype).name, "shape": "wave" if n <= 64 else "block", "instances": REPLICAS,
           "steps_per_launch": STEPS_PER_LAUNCH, "launches": int(launches), "repeats": repeats, "all_stuck": bool(opt.is_stuck.all()),
           "total_ms_host_clock_median": wall_ms, "total_ms_host_clock_min_max": [float(min(walls)), float(max(walls))],
           "total_ms_device_events_median": dev_ms, "total_ms_device_events_min_max": [float(min(devs)), float(max(devs))],
           "instance_steps_total": total, "instance_steps_per_s_host_clock": total / (wall_ms * 1e-3),
           "instance_steps_per_s_device_events": total / (dev_ms * 1e-3),
           "us_per_step_per_instance_device_events": dev_ms * 1e3 / max(int(counts.max()), 1),
           "steps_to_stuck": {"min": int(counts.min()), "p25": float(np.percentile(counts, 25)), "median": float(np.median(counts)),
                              "p75": float(np.percentile(counts, 75)), "max": int(counts.max()), "mean": float(counts.mean())},
           "energy_before_median": float(np.median(e_start)), "lowest_minimum": float(srt[0]), "highest_minimum": float(srt[-1]),
           "distinct_minima_1e-6": int(1 + np.sum(np.diff(srt) > 1e-6))}
    # for information: the batched L-BFGS quench of the same starts, one timed pass after its own warm-up
    bq.quench_once(dzo, replicas, n)
    wall, dev_ms, launches, lb = bq.quench_once(dzo, replicas, n)
    lcounts = lb.iteration_counts
    row["batched_lbfgs_same_starts"] = {"history_length": 10, "total_ms_host_clock": wall * 1e3, "total_ms_device_events": dev_ms,
                                        "launches": int(launches), "all_stuck": bool(lb.is_stuck.all()),
                                        "instance_steps_total": int(lcounts.sum()),
                                        "steps_to_stuck": {"min": int(lcounts.min()), "median": float(np.median(lcounts)),
                                                           "max": int(lcounts.max()), "mean": float(lcounts.mean())},
                                        "lowest_minimum": float(lb.current_objective_values.min())}
    dzo.profile_enable(0)
    return row, replicas


def baseline_case(dzo, replicas, n, count):
    """the same starting points, one dzo_adgd_* optimizer each, one after the other"""
    starts = replicas.to_host().reshape(REPLICAS, 3 * n)
    which = list(range(REPLICAS)) if count >= REPLICAS else [int(k) for k in np.linspace(0, REPLICAS - 1, count).round()]
    seconds, steps, finals, stuck = [], [], [], []
    for idx, k in enumerate([which[0]] + which):             # the first one twice: its first run is the warm-up
        x = dzo.DeviceArray.from_host(starts[k])
        dzo.synchronize()
        t0 = time.perf_counter()
        prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
        opt = dzo.AdGDOptimizer(None, prob, None, x, 0.01)
        taken = 0
        while taken < MAX_STEPS and not opt.is_stuck:
            opt.step()
            taken += 1
        dzo.synchronize()
        dt = time.perf_counter() - t0
        if idx:
            seconds.append(dt); steps.append(opt.iteration_count); finals.append(opt.current_objective_value); stuck.append(opt.is_stuck)
    measured = float(np.sum(seconds))
    return {"n": n, "dtype": "float64", "instances_run": len(which), "which": "all 256" if len(which) == REPLICAS else which,
            "all_stuck": bool(all(stuck)), "seconds_measured": measured, "steps_measured": int(np.sum(steps)),
            "us_per_step": measured / max(int(np.sum(steps)), 1) * 1e6,
            "seconds_for_256": measured * REPLICAS / len(which), "extrapolated": len(which) != REPLICAS,
            "steps_to_stuck": {"min": int(np.min(steps)), "median": float(np.median(steps)), "max": int(np.max(steps)),
                               "mean": float(np.mean(steps))},
            "lowest_minimum": float(np.min(finals))}


def dynamic_lds(n, es):
    """bytes of dynamic LDS a step launch asks for (dzo_adgd_batch_create)"""
    return 0 if n <= 64 else 16 * 4 + 5 * 3 * n * es


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adgd_batch_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-count", type=int, default=256)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    args = ap.parse_args()
    from dzo_loader import dzo
    lib_path = dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit,
           "workload": f"{REPLICAS} replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps, a copy run by BatchedAdGD to all_stuck",
           "device_runs": [], "baseline": [], "kernels": bq.kernel_figures(lib_path, "adgd_batch_"),
           "dynamic_lds_bytes": {f"n{n}_{'f64' if es == 8 else 'f32'}": dynamic_lds(n, es) for n in (13, 38, 200, 1024) for es in (8, 4)}}
    keep = None
    for dtype in (np.float64, np.float32):
        for n in (38, 13, 200):
            row, replicas = device_case(dzo, n, dtype, args.repeats)
            if n == 38 and dtype == np.float64:
                keep = (replicas, row)
            res["device_runs"].append(row)
            print(json.dumps(row), flush=True)
    if args.baseline_count > 0:
        replicas, row = keep
        base = baseline_case(dzo, replicas, 38, args.baseline_count)
        res["baseline"].append(base)
        print(json.dumps(base), flush=True)
        ratio = base["seconds_for_256"] * 1e3 / row["total_ms_host_clock_median"]
        res["comparison_n38_f64"] = {"batched_ms_host_clock": row["total_ms_host_clock_median"], "baseline_ms_for_256": base["seconds_for_256"] * 1e3,
                                     "ratio": ratio, "extrapolated": base["extrapolated"],
                                     "batched_is_faster": bool(row["total_ms_host_clock_median"] < base["seconds_for_256"] * 1e3)}
        print(json.dumps(res["comparison_n38_f64"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
