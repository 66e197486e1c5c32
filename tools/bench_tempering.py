"""Measurement of the parallel-tempering kernels (csrc/dzo_tempering.hip) on the device: recorded, not gated.

    python tools/bench_tempering.py [--out profiles/tempering_bench.json] [--batches 20] [--baseline-moves 3000]

Workload: the reference's own (scripts/MonteCarlo.jl:252-260): N = 38, 256 replicas, num_steps = 500, temperatures
0.05 .. 0.35, constraining radius 2.25, fp64 and fp32; the same for N = 13 and N = 200 (constraining radius scaled with
N^(1/3)).  After a warm-up run() of the same size, `batches` batches of run() (each: temper, swap, temper, swap) are timed
twice over: by the library's HIP events around every kernel on the launching stream (dzo_profile_*: the device time), and by
the host clock around run() + synchronize (what a caller sees).  Reported: Monte Carlo steps per second (the reference's
metric: 2 * num_steps * batches * replicas / time) and time per step per replica.

Baseline: the only way the parent commit offers to do the same work -- a host loop over dzo_pairwise_energy_delta on ONE
replica (one launch and one host wait per move; an accepted move uploads the three new coordinates).  Its rate is measured
over `baseline-moves` moves.  The handle-less pairwise entry points share one stream and one result word per device, so 256
replicas driven this way are served one move at a time: the whole workload runs at that same rate (the extrapolation:
256 x the moves at the measured time per move).  `ratio_if_256_host_threads_overlapped` divides by 256 once more, for a
caller who could overlap 256 such loops perfectly -- which the parent cannot.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPLICAS, STEPS = 256, 500


def start_replicas(n, replicas, radius, dtype, seed=1):
    """(:198-213) standard-normal points redrawn until they lie inside the sphere, spread out enough to be finite"""
    rng = np.random.default_rng(seed)
    out = np.empty((replicas, 3, n))
    for k in range(replicas):
        for i in range(n):
            while True:
                p = rng.standard_normal(3) * radius / 2.25
                if (p * p).sum() < radius * radius:
                    out[k, :, i] = p
                    break
    return out.astype(dtype)


def device_case(dzo, n, dtype, batches):
    radius = 2.25 * (n / 38.0) ** (1.0 / 3.0)
    reps = start_replicas(n, REPLICAS, radius, dtype)
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), REPLICAS))
    dev = dzo.DeviceArray.from_host(reps.reshape(-1))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(REPLICAS, 0.05), radius, 1)
    rows = 2 * STEPS * batches
    energies = dzo.DeviceArray.zeros(rows * REPLICAS, dtype)
    pt.run(STEPS, batches, energies)                     # warm-up: leaves the random start behind
    dzo.synchronize()
    dzo.profile_enable(2)
    dzo.profile_reset()
    t0 = time.perf_counter()
    pt.run(STEPS, batches, energies)
    dzo.synchronize()
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    dzo.profile_enable(0)
    temper_ms, swap_ms = table["tempering_temper"][1], table["tempering_swap"][1]
    trials = 2 * STEPS * batches * REPLICAS
    dev_s = (temper_ms + swap_ms) * 1e-3
    cv, cvp, mom = pt.analyze(energies, rows)
    return {"n": n, "dtype": np.dtype(dtype).name, "shape": "wave" if n <= 64 else "block", "replicas": REPLICAS, "num_steps": STEPS,
            "batches": batches, "temper_launches": table["tempering_temper"][0], "temper_ms_total": temper_ms, "swap_ms_total": swap_ms,
            "mc_steps_per_s_device_events": trials / dev_s, "mc_steps_per_s_host_clock": trials / wall,
            "ns_per_step_per_replica_device_events": dev_s / (2 * STEPS * batches) * 1e9,
            "mean_energy_coldest": float(mom[0, 0]), "mean_energy_hottest": float(mom[-1, 0]),
            "mean_acceptance": float(pt.num_accept.mean() / STEPS)}


def baseline_case(dzo, n, dtype, moves):
    """Metropolis moves of one replica through dzo_pairwise_energy_delta, the host deciding"""
    import pairwise_twin as pw
    xyz = np.stack(pw.cluster(n, seed=n)).astype(dtype)
    buf = dzo.DeviceArray.from_host(xyz.reshape(-1))
    x, y, z = (buf.view(c * n, n) for c in range(3))
    rng = np.random.default_rng(0)
    beta, radius = 10.0, 0.03
    host = xyz.astype(np.float64)
    for timed in (False, True):
        count = moves if timed else 200
        accepted = 0
        t0 = time.perf_counter()
        for _ in range(count):
            j = int(rng.integers(n))
            new = host[:, j] + radius * rng.standard_normal(3)
            d = dzo.pairwise_radial_energy_delta(x, y, z, j, *new)
            if d <= 0 or rng.random() <= np.exp(-beta * d):
                host[:, j] = new
                for c in range(3):
                    buf.view(c * n + j, 1).upload(np.array([new[c]]))
                accepted += 1
        dt = time.perf_counter() - t0
    return {"n": n, "dtype": np.dtype(dtype).name, "moves": moves, "accepted": accepted, "seconds": dt, "mc_steps_per_s": moves / dt,
            "us_per_move": dt / moves * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempering_bench.json"))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--baseline-moves", type=int, default=3000)
    args = ap.parse_args()
    from dzo_loader import dzo
    dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": commit,
           "note": "every number here is new: the parent commit has no tempering loop; its only path is the baseline below",
           "device_runs": [], "baseline": []}
    for dtype in (np.float64, np.float32):
        for n in (38, 13, 200):
            row = device_case(dzo, n, dtype, args.batches)
            res["device_runs"].append(row)
            print(json.dumps(row), flush=True)
    for dtype in (np.float64, np.float32):
        row = baseline_case(dzo, 38, dtype, args.baseline_moves)
        res["baseline"].append(row)
        print(json.dumps(row), flush=True)
    res["comparison_n38"] = []
    for b in res["baseline"]:
        d = next(r for r in res["device_runs"] if r["n"] == 38 and r["dtype"] == b["dtype"])
        ratio = d["mc_steps_per_s_host_clock"] / b["mc_steps_per_s"]
        res["comparison_n38"].append({"dtype": b["dtype"], "device_mc_steps_per_s": d["mc_steps_per_s_host_clock"],
                                      "baseline_mc_steps_per_s": b["mc_steps_per_s"], "ratio": ratio,
                                      "ratio_if_256_host_threads_overlapped": ratio / REPLICAS,
                                      "extrapolation": "baseline measured on one replica; 256 replicas share the one stream and are served at the same rate"})
        print(json.dumps(res["comparison_n38"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
