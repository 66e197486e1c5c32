"""Measurement of the Thomson unit (csrc/dzo_sphere.hip) on the device: recorded, not gated.  There was no device path for this
objective before, so there is no speed-up to claim; the figures stand next to the Lennard-Jones units of the same launch shapes.

    python tools/bench_sphere.py [--out profiles/sphere_bench.json] [--repeats 5] [--twin-count 4]

Shapes: N = 38 x 256 (WAVE) and N = 200 x 64 (BLOCK), fp64 and fp32, one session, a warm-up before every timed group, medians
of `repeats` runs (at least 3).
  * sphere_energy_gradient (tangent gradient) next to pairwise_batch_energy_gradient for Lennard-Jones on points of the same shape,
    by the library's HIP events around the launch (dzo_profile_*): the ratio is what the square root and the second division cost
    per pair.
  * one SphereLBFGS run (step 0.01, history 10, 50 step!() calls per launch) from random starts on the sphere to all_stuck, by the
    host clock around create + launches + the last wait: the step counts, the time per instance-step (total / the sum of the
    instances' steps) and per step of the slowest instance; next to one BatchedLBFGS run on tempered Lennard-Jones replicas of the
    same shape (the start of tools/bench_quench.py with that many replicas), code that the parent commit has.
  * the numpy twin (tests/sphere_twin.py, SphereQuench) on the first `twin-count` of the same sphere starts to is_stuck, by the host
    clock, extrapolated to the batch by the mean: the host baseline.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_tempering import start_replicas  # noqa: E402

SHAPES = [(38, 256), (200, 64)]
STEPS_PER_LAUNCH, MAX_STEPS = 50, 20000


def sphere_starts(n, batch, dtype):
    import sphere_twin as st
    return st.random_starts(n, batch, 2026 + n, dtype)


def tempered_replicas(dzo, n, batch, dtype):
    radius = 2.25 * (n / 38.0) ** (1.0 / 3.0)
    reps = start_replicas(n, batch, radius, dtype)
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), batch))
    dev = dzo.DeviceArray.from_host(reps.reshape(-1))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(batch, 0.05), radius, 1)
    pt.run(500, 20)
    dzo.synchronize()
    return dev


def eval_times(dzo, call, timer, repeats):
    """device-event ms of `repeats` single evaluations after a warm-up"""
    call()
    out = []
    for _ in range(repeats):
        dzo.synchronize()
        dzo.profile_reset()
        call()
        out.append(dzo.profile_table()[timer][1])
    return out


def run_once(dzo, make, points):
    copy = points.copy()
    dzo.synchronize()
    t0 = time.perf_counter()
    opt = make(copy)
    done, taken = False, 0
    while not done and taken < MAX_STEPS:
        done = opt.step(STEPS_PER_LAUNCH)
        taken += STEPS_PER_LAUNCH
    return (time.perf_counter() - t0) * 1e3, opt


def run_case(dzo, make, points, repeats):
    run_once(dzo, make, points)                                # warm-up of the same size
    walls = []
    for _ in range(repeats):
        wall, opt = run_once(dzo, make, points)
        walls.append(wall)
    counts = opt.iteration_counts
    f = opt.current_objective_values.astype(np.float64)
    med = float(np.median(walls))
    return {"all_stuck": bool(opt.is_stuck.all()), "total_ms_host_clock_median": med, "total_ms_host_clock_min_max": [float(min(walls)), float(max(walls))],
            "steps_to_stuck": {"min": int(counts.min()), "median": float(np.median(counts)), "max": int(counts.max())},
            "instance_steps_total": int(counts.sum()), "us_per_instance_step": med * 1e3 / max(int(counts.sum()), 1),
            "us_per_step_of_the_slowest_instance": med * 1e3 / max(int(counts.max()), 1),
            "lowest_energy": float(f.min()), "highest_energy": float(f.max())}


def twin_case(starts, dtype, count):
    import sphere_twin as st
    seconds, steps = [], []
    for p in starts[:count]:
        t0 = time.perf_counter()
        q = st.SphereQuench(p, 0.01, 10, dtype)
        steps.append(q.run(MAX_STEPS))
        seconds.append(time.perf_counter() - t0)
    total_steps = max(int(np.sum(steps)), 1)
    return {"instances_run": len(seconds), "seconds_measured": float(np.sum(seconds)), "steps_measured": int(np.sum(steps)),
            "us_per_instance_step": float(np.sum(seconds)) / total_steps * 1e6,
            "seconds_for_the_batch_extrapolated": float(np.mean(seconds)) * len(starts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twin-count", type=int, default=4)
    ap.add_argument("--on-top-of", default=None, help="the commit the measured tree was built on top of, where it is not a commit itself")
    args = ap.parse_args()
    assert args.repeats >= 3
    from dzo_loader import dzo
    dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "commit": commit, "on_top_of_commit": args.on_top_of,
           "method": "one session; a warm-up before every timed group; medians of %d runs; evaluations by device events, runs by the host clock" % args.repeats,
           "not_measured": ["other N and batch sizes", "history lengths other than 10", "the ring in device memory (N >= 98 in fp64 at history 32)",
                            "the Julia module", "the twin on more than --twin-count instances (extrapolated by the mean)",
                            "hardware counters of the new kernels"],
           "cases": []}
    for dtype in (np.float64, np.float32):
        for n, batch in SHAPES:
            starts = sphere_starts(n, batch, dtype)
            sphere = dzo.DeviceArray.from_host(starts.reshape(-1))
            lj = tempered_replicas(dzo, n, batch, dtype)
            gs, gl = dzo.DeviceArray.zeros(3 * n * batch, dtype), dzo.DeviceArray.zeros(3 * n * batch, dtype)
            dzo.profile_enable(2)
            ts = eval_times(dzo, lambda: dzo.sphere_energy_gradient(sphere, n, gs), "sphere_batch_energy_gradient", args.repeats)
            tl = eval_times(dzo, lambda: dzo.pairwise_batch_energy_gradient(lj, n, gl), "pairwise_batch_energy_gradient", args.repeats)
            dzo.profile_enable(0)
            pairs = n * (n - 1) * batch
            row = {"n": n, "batch": batch, "dtype": np.dtype(dtype).name, "shape": "wave" if n <= 64 else "block",
                   "energy_gradient": {"sphere_us_median": float(np.median(ts)) * 1e3, "sphere_us_min_max": [min(ts) * 1e3, max(ts) * 1e3],
                                       "lennard_jones_us_median": float(np.median(tl)) * 1e3, "lennard_jones_us_min_max": [min(tl) * 1e3, max(tl) * 1e3],
                                       "ratio_sphere_over_lennard_jones": float(np.median(ts) / np.median(tl)),
                                       "sphere_ordered_pairs_per_s": pairs / (float(np.median(ts)) * 1e-3)},
                   "sphere_lbfgs": run_case(dzo, lambda p: dzo.SphereLBFGS(p, n, 0.01, 10), sphere, args.repeats),
                   "lennard_jones_lbfgs": run_case(dzo, lambda p: dzo.BatchedLBFGS(p, n, 0.01, 10), lj, args.repeats)}
            row["us_per_instance_step_ratio_sphere_over_lennard_jones"] = (row["sphere_lbfgs"]["us_per_instance_step"]
                                                                           / row["lennard_jones_lbfgs"]["us_per_instance_step"])
            if args.twin_count > 0:
                row["numpy_twin"] = twin_case(starts, dtype, args.twin_count)
                row["twin_over_device_per_instance_step"] = row["numpy_twin"]["us_per_instance_step"] / row["sphere_lbfgs"]["us_per_instance_step"]
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
