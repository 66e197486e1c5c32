"""What the Morse pair term costs on the device next to Lennard-Jones, in one session: recorded, not gated.

    python tools/bench_morse.py [--out profiles/morse_bench.json] [--repeats 5]

For each radial (Lennard-Jones, Morse rho = 6, Morse rho = 14), each element type and the two sizes N = 38 x 256 instances (WAVE
shape) and N = 200 x 64 instances (BLOCK shape):

* evaluation: dzo_pairwise_batch_energy_gradient of the tempered replicas below, `--calls` calls after a warm-up, timed by the
  library's HIP events around every launch (dzo_profile_*).  Pairs per second counts ordered pairs, instances x N x (N - 1) per
  call: every lane evaluates its own (i, j) term.
* quench: the workload of tools/bench_quench.py under the radial -- the replicas (the start of tools/bench_tempering.py, fixed
  seed) are tempered for 20 batches of 500 steps under that radial, and a copy is quenched by ONE BatchedLBFGS handle (step 0.01,
  history 10, 50 step!() calls per launch) until every instance is stuck.  After a warm-up quench, `repeats` quenches of fresh
  copies are timed by the device events and by the host clock; the quenches of one case are bit-identical, so the spread is the
  clock's.  The Lennard-Jones N = 38 x 256 row is the same workload as profiles/quench_bench.json.

The ratios Morse / Lennard-Jones of the same session are in `ratios`.  A quench under another potential runs another number of
steps, so the quench ratio is given per step of the longest instance as well as in total.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tempering import start_replicas  # noqa: E402

STEPS, BATCHES, STEPS_PER_LAUNCH, MAX_STEPS = 500, 20, 50, 20000
SIZES = [(38, 256), (200, 64)]


def tempered(dzo, n, count, dtype, radial):
    radius = 2.25 * (n / 38.0) ** (1.0 / 3.0)
    reps = start_replicas(n, count, radius, dtype)
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), count))
    dev = dzo.DeviceArray.from_host(reps.reshape(-1))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(count, 0.05), radius, 1, radial=radial)
    pt.run(STEPS, BATCHES)
    dzo.synchronize()
    return dev


def evaluation(dzo, replicas, n, count, radial, calls):
    grad = dzo.DeviceArray.zeros(replicas.size, replicas.dtype)
    dzo.pairwise_batch_energy_gradient(replicas, n, grad, radial=radial)
    dzo.profile_enable(2)
    dzo.profile_reset()
    for _ in range(calls):
        dzo.pairwise_batch_energy_gradient(replicas, n, grad, radial=radial)
    launches, ms = dzo.profile_table()["pairwise_batch_energy_gradient"][:2]
    dzo.profile_enable(0)
    pairs = count * n * (n - 1)
    return {"calls": int(launches), "us_per_call_device_events": ms * 1e3 / launches, "ordered_pairs_per_call": pairs,
            "pairs_per_s": pairs * launches / (ms * 1e-3)}


def quench_once(dzo, replicas, n, radial):
    copy = replicas.copy()
    dzo.synchronize()
    dzo.profile_reset()
    t0 = time.perf_counter()
    opt = dzo.BatchedLBFGS(copy, n, 0.01, 10, radial=radial)
    done, taken = False, 0
    while not done and taken < MAX_STEPS:
        done = opt.step(STEPS_PER_LAUNCH)
        taken += STEPS_PER_LAUNCH
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    return wall * 1e3, table["lbfgs_batch_step"][1] + table["lbfgs_batch_init"][1], opt


def quench(dzo, replicas, n, radial, repeats):
    dzo.profile_enable(2)
    quench_once(dzo, replicas, n, radial)
    walls, devs = [], []
    for _ in range(repeats):
        wall, dev, opt = quench_once(dzo, replicas, n, radial)
        walls.append(wall); devs.append(dev)
    dzo.profile_enable(0)
    counts, f = opt.iteration_counts, opt.current_objective_values.astype(np.float64)
    dev_ms = float(np.median(devs))
    return {"all_stuck": bool(opt.is_stuck.all()), "repeats": repeats, "total_ms_device_events_median": dev_ms,
            "total_ms_device_events_min_max": [float(min(devs)), float(max(devs))], "total_ms_host_clock_median": float(np.median(walls)),
            "total_ms_host_clock_min_max": [float(min(walls)), float(max(walls))], "steps_max": int(counts.max()), "steps_mean": float(counts.mean()),
            "us_per_step_per_instance_device_events": dev_ms * 1e3 / max(int(counts.max()), 1), "lowest_minimum": float(f.min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morse_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the HIP runtime first)
    from dzo_loader import dzo
    dzo.init(0)
    radials = [("lennard_jones", dzo.RADIAL_LENNARD_JONES), ("morse_rho6", dzo.RADIAL_MORSE_RHO6), ("morse_rho14", dzo.RADIAL_MORSE_RHO14)]
    res = {"device": dzo.device_info(), "workload": __doc__.split("\n\n")[2], "rows": [], "ratios": []}
    for n, count in SIZES:
        for dtype in (np.float64, np.float32):
            rows = {}
            for name, radial in radials:
                replicas = tempered(dzo, n, count, dtype, radial)
                row = {"radial": name, "n": n, "instances": count, "dtype": np.dtype(dtype).name, "shape": "wave" if n <= 64 else "block",
                       "evaluation": evaluation(dzo, replicas, n, count, radial, args.calls), "quench": quench(dzo, replicas, n, radial, args.repeats)}
                rows[name] = row
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            lj = rows["lennard_jones"]
            for name in ("morse_rho6", "morse_rho14"):
                m = rows[name]
                ratio = {"radial": name, "n": n, "dtype": np.dtype(dtype).name,
                         "evaluation_time_over_lennard_jones": m["evaluation"]["us_per_call_device_events"] / lj["evaluation"]["us_per_call_device_events"],
                         "quench_total_time_over_lennard_jones": m["quench"]["total_ms_device_events_median"] / lj["quench"]["total_ms_device_events_median"],
                         "quench_time_per_step_over_lennard_jones": m["quench"]["us_per_step_per_instance_device_events"]
                         / lj["quench"]["us_per_step_per_instance_device_events"]}
                res["ratios"].append(ratio)
                print(json.dumps(ratio), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
