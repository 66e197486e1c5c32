"""Measurement of the batched basin hopping (csrc/dzo_basin_hopping.hip) on the device: recorded, not gated.

    python tools/bench_basin_hopping.py [--out profiles/basin_hopping_bench.json] [--hops 48] [--repeats 3]

Workload: 256 walkers of the 38-atom Lennard-Jones cluster from random starts inside the sphere (the start of
tools/bench_tempering.py, fixed seed), temperature 0.8, perturbation radius 0.35, quench by L-BFGS (step 0.01, history 10, at
most 400 steps), `hops` hops per walker in launches of 8, fp64 and fp32.

* `hop`: after a warm-up run of the same size, `repeats` runs on fresh handles (the same seed: bit-identical work) are timed by
  the host clock around create + the launches + the last wait, and by the library's HIP events around the launches
  (dzo_profile_*).  Reported: hops per second and L-BFGS iterations per second.
* host loop: the path there was before this unit, on dzo.BatchedLBFGS alone.  Per hop the host reads the minima, perturbs them
  (numpy normals, the same sphere rule), uploads, creates a BatchedLBFGS, steps 50 at a time until all_stuck or 400 steps, reads
  the energies, decides on the host and keeps the accepted points.  Its random numbers are numpy's, so its walk is another
  sample of the same process: compare rates, not trajectories.
* own pace: from REC_QUENCH_ITERATIONS of one recorded run, sum over hops of the slowest walker's iterations (what lock-step
  hopping waits for) and the largest sum over hops of one walker's iterations (what one launch per call waits for); their
  ratio is the gain own-pace hopping can give over lock step.
* the first hop at which any walker's quench reached -173.928427 (within 5e-7), if one did: reported, not asserted.
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

from bench_quench import kernel_figures  # noqa: E402
from bench_tempering import start_replicas  # noqa: E402

N, WALKERS = 38, 256
TEMPERATURE, RADIUS, SPHERE = 0.8, 0.35, 2.25
STEP, HISTORY, QUENCH_STEPS = 0.01, 10, 400
HOPS_PER_LAUNCH, STEPS_PER_LAUNCH = 8, 50
LJ38 = -173.928427


def make(dzo, starts, seed=1):
    dev = dzo.DeviceArray.from_host(starts.reshape(-1))
    return dev, dzo.BasinHopping(dev, N, np.full(WALKERS, 1.0 / TEMPERATURE), np.full(WALKERS, RADIUS), SPHERE, STEP, HISTORY, QUENCH_STEPS, seed)


def device_run(dzo, starts, hops):
    """(host seconds, device ms of the launches, handle) of create + hops + wait on a fresh handle"""
    dzo.synchronize()
    dzo.profile_reset()
    t0 = time.perf_counter()
    dev, bh = make(dzo, starts)
    bh.hop(hops, adapt=False, hops_per_launch=HOPS_PER_LAUNCH, wait=True)
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    return wall, table["basin_hopping_hop"][1] + table["basin_hopping_init"][1], bh


def recorded_run(dzo, starts, hops):
    """REC_QUENCH_ITERATIONS (walkers, hops) and REC_TRIAL_ENERGY of the same walk, read after every launch"""
    dev, bh = make(dzo, starts)
    bh.set_record(HOPS_PER_LAUNCH)
    its, energies = [], []
    done = 0
    while done < hops:
        k = min(HOPS_PER_LAUNCH, hops - done)
        bh.hop(k, adapt=False, hops_per_launch=HOPS_PER_LAUNCH)
        its.append(bh.read(dzo.BASIN_HOPPING_REC_QUENCH_ITERATIONS)[:, :k])
        energies.append(bh.read(dzo.BASIN_HOPPING_REC_TRIAL_ENERGY)[:, :k])
        done += k
    return np.concatenate(its, axis=1).astype(np.int64), np.concatenate(energies, axis=1).astype(np.float64), bh


def host_loop(dzo, starts, hops, dtype, seed=1):
    """the same walk as a host loop over dzo.BatchedLBFGS; (host seconds, total L-BFGS iterations, best energy, accepted)"""
    rng = np.random.default_rng(seed)
    t = np.dtype(dtype).type
    beta = 1.0 / TEMPERATURE

    def quench(points):
        dev = dzo.DeviceArray.from_host(points.reshape(-1))
        opt = dzo.BatchedLBFGS(dev, N, STEP, HISTORY)
        done, taken = False, 0
        while not done and taken < QUENCH_STEPS:
            done = opt.step(STEPS_PER_LAUNCH)
            taken += STEPS_PER_LAUNCH
        out = opt.current_points, opt.current_objective_values.astype(np.float64), int(opt.iteration_counts.sum())
        opt.close()
        return out

    dzo.synchronize()
    t0 = time.perf_counter()
    x, e, total = quench(starts)
    best, accepted = e.copy(), 0
    for _ in range(hops):
        trial = x.reshape(WALKERS, 3, N) + t(RADIUS) * rng.standard_normal((WALKERS, 3, N)).astype(dtype)
        inside = (trial ** 2).sum(axis=1, keepdims=True) < t(SPHERE) ** 2
        trial = np.where(inside, trial, x.reshape(WALKERS, 3, N)).reshape(WALKERS, 3 * N)
        xq, eq, its = quench(trial)
        total += its
        delta = eq - e
        with np.errstate(all="ignore"):
            take = np.isfinite(eq) & ((delta <= 0) | (rng.random(WALKERS) <= np.exp(-beta * delta)))
        x[take], e[take] = xq[take], eq[take]
        accepted += int(take.sum())
        best = np.where(np.isfinite(eq) & (eq < best), eq, best)
    return time.perf_counter() - t0, total, float(best.min()), accepted


def case(dzo, dtype, hops, repeats):
    starts = start_replicas(N, WALKERS, SPHERE, dtype)
    dzo.profile_enable(2)
    device_run(dzo, starts, hops)                            # warm-up run of the same size
    walls, devs = [], []
    for _ in range(repeats):
        wall, dev_ms, bh = device_run(dzo, starts, hops)
        walls.append(wall * 1e3); devs.append(dev_ms)
    dzo.profile_enable(0)
    iterations = int(bh.quench_iterations.sum())
    wall_ms, dev_ms = float(np.median(walls)), float(np.median(devs))
    its, energies, rec = recorded_run(dzo, starts, hops)
    assert int(its.sum()) == iterations, "the recorded run is the timed one"
    lock_step, own_pace = int(its.max(axis=0).sum()), int(its.sum(axis=1).max())
    hit = np.flatnonzero((np.abs(energies - LJ38) <= 5e-7).any(axis=0))
    host_loop(dzo, starts, min(hops, 4), dtype)              # warm-up
    base = [host_loop(dzo, starts, hops, dtype) for _ in range(repeats)]
    base_ms = float(np.median([b[0] for b in base])) * 1e3
    base_its = base[0][1]
    total_hops = hops * WALKERS
    return {"n": N, "dtype": np.dtype(dtype).name, "walkers": WALKERS, "hops": hops, "hops_per_launch": HOPS_PER_LAUNCH, "repeats": repeats,
            "temperature": TEMPERATURE, "radius": RADIUS, "constraining_radius": SPHERE, "quench_steps": QUENCH_STEPS,
            "hop": {"total_ms_host_clock_median": wall_ms, "total_ms_host_clock_min_max": [float(min(walls)), float(max(walls))],
                    "total_ms_device_events_median": dev_ms, "total_ms_device_events_min_max": [float(min(devs)), float(max(devs))],
                    "hops_per_s_host_clock": total_hops / (wall_ms * 1e-3), "lbfgs_iterations": iterations,
                    "lbfgs_iterations_per_s_host_clock": iterations / (wall_ms * 1e-3),
                    "accepted_last_launch": int(bh.num_accept.sum()), "quenches_unfinished": int(bh.quench_unfinished.sum()),
                    "best_energy": float(bh.best_energies.min())},
            "host_loop": {"total_ms_host_clock_median": base_ms, "total_ms_host_clock_min_max": [float(min(b[0] for b in base)) * 1e3,
                                                                                                   float(max(b[0] for b in base)) * 1e3],
                          "hops_per_s_host_clock": total_hops / (base_ms * 1e-3), "lbfgs_iterations": base_its,
                          "lbfgs_iterations_per_s_host_clock": base_its / (base_ms * 1e-3), "steps_per_launch": STEPS_PER_LAUNCH,
                          "accepted": base[0][3], "best_energy": base[0][2]},
            "host_loop_over_hop_host_clock": base_ms / wall_ms,
            "own_pace": {"sum_over_hops_of_max_over_walkers": lock_step, "max_over_walkers_of_sum_over_hops": own_pace,
                         "ratio": lock_step / max(own_pace, 1),
                         "iterations_per_quench": {"min": int(its.min()), "median": float(np.median(its)), "max": int(its.max())}},
            "first_hop_at_lj38": int(hit[0]) + 1 if hit.size else None,
            "walkers_whose_best_is_lj38": int((np.abs(rec.best_energies.astype(np.float64) - LJ38) <= 5e-7).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basin_hopping_bench.json"))
    ap.add_argument("--hops", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
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
           "workload": f"{WALKERS} walkers of LJ{N} from random starts, T = {TEMPERATURE}, radius {RADIUS}, {args.hops} hops in launches of "
                       f"{HOPS_PER_LAUNCH}; the host loop runs the same process on dzo.BatchedLBFGS with numpy's random numbers",
           "sessions": 1, "runs": [], "kernels": kernel_figures(lib_path, "basin_hop_")}
    for dtype in (np.float64, np.float32):
        row = case(dzo, dtype, args.hops, args.repeats)
        res["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
