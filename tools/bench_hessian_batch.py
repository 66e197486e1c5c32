"""Measurement of the batched Hessian entry points (dzo_pairwise_batch_hessian / dzo_pairwise_batch_hvp,
csrc/dzo_hessian_batch.hip) on the device: recorded, not gated.

    python tools/bench_hessian_batch.py [--out profiles/hessian_batch_bench.json] [--repeats 20] [--baseline-repeats 3]

Workload: the tempered replicas of tools/bench_quench.py (256 replicas of the 38-atom Lennard-Jones cluster, fixed seed, 20
batches of 500 steps), quenched by one BatchedLBFGS handle; then the dense 114 x 114 Hessian of every quenched replica.

New path: ONE dzo_pairwise_batch_hessian call into a preallocated device array (the call blocks).  After a warm-up call,
`repeats` calls are timed twice over: by the library's HIP events around the launch (dzo_profile_*: the kernel's time) and by
the host clock around the call (what a caller sees).  From the kernel's time, the bytes it writes per second (9 N^2 elements per
instance; it reads 3 N), next to dzo_calibrate_read_bandwidth over the same number of bytes, for information.

Baseline: the only path the parent commit has -- per replica 114 blocking dzo_pairwise_hvp calls with the unit vectors as
directions, column c written straight into column c of a dense matrix of the same layout; all 256 replicas run, host clock
around the 29184 calls, `baseline-repeats` passes after a warm-up replica.  This commit does not touch dzo_pairwise.hip, so the
baseline run in this tree is the parent's.  The two sets of Hessians are compared (the single-cluster kernel sums a row in
another order, so they agree to rounding, not bit for bit).

For information: the same one-call measurement at N = 13 and 200 (BLOCK shape) and in fp32, and one dzo_pairwise_batch_hvp call
with one direction per replica.
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


def quenched(dzo, n, dtype):
    """(device array of the quenched replicas, the optimizer that holds it)"""
    replicas = bq.tempered_replicas(dzo, n, dtype)
    dzo.profile_enable(2)                                    # quench_once reads its launches' times
    _, _, _, opt = bq.quench_once(dzo, replicas, n)
    dzo.profile_enable(0)
    return opt.points, opt


def timed_calls(dzo, call, kernel, repeats):
    """median / min / max of the host clock around `call` and of the HIP events of `kernel`, in microseconds"""
    call()                                                   # warm-up: loads the code object
    dzo.profile_enable(2)
    host, dev = [], []
    for _ in range(repeats):
        dzo.synchronize()
        dzo.profile_reset()
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e6)
        launches, ms = dzo.profile_table()[kernel]
        assert launches == 1
        dev.append(ms * 1e3)
    dzo.profile_enable(0)
    stats = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    return stats(host), stats(dev)


def hessian_case(dzo, points, n, dtype, repeats):
    lib = dzo.lib()
    es = np.dtype(dtype).itemsize
    out = dzo.DeviceArray.zeros(9 * n * n * REPLICAS, dtype)

    def call():
        dzo._check(lib.dzo_pairwise_batch_hessian(dzo.RADIAL_LENNARD_JONES, n, REPLICAS, dzo._dt(dtype), points.ptr, out.ptr))

    host, dev = timed_calls(dzo, call, "hess_batch_hessian", repeats)
    written = 9 * n * n * REPLICAS * es
    row = {"n": n, "dtype": np.dtype(dtype).name, "shape": "wave" if n <= 64 else "block", "instances": REPLICAS, "repeats": repeats,
           "call_us_host_clock": host, "kernel_us_device_events": dev, "bytes_written": written,
           "written_GB_per_s_device_events": written / (dev["median"] * 1e-6) / 1e9,
           "pair_terms_per_s_device_events": n * n * REPLICAS / (dev["median"] * 1e-6),
           "read_bandwidth_GB_per_s_same_bytes": dzo.calibrate_read_bandwidth(written)}
    return row, out


def hvp_case(dzo, points, n, dtype, repeats):
    lib = dzo.lib()
    rng = np.random.default_rng(3)
    d = dzo.DeviceArray.from_host(rng.normal(size=3 * n * REPLICAS), dtype=dtype)
    out = dzo.DeviceArray.zeros(3 * n * REPLICAS, dtype)
    curv = dzo.DeviceArray.zeros(2 * REPLICAS)

    def call():
        dzo._check(lib.dzo_pairwise_batch_hvp(dzo.RADIAL_LENNARD_JONES, n, REPLICAS, dzo._dt(dtype), points.ptr, 3 * n, d.ptr, out.ptr, curv.ptr))

    host, dev = timed_calls(dzo, call, "hess_batch_hvp", repeats)
    return {"n": n, "dtype": np.dtype(dtype).name, "instances": REPLICAS, "directions_per_instance": 1, "repeats": repeats,
            "call_us_host_clock": host, "kernel_us_device_events": dev}


def baseline_case(dzo, points, n, passes):
    """114 dzo_pairwise_hvp calls with unit vectors per replica, all replicas, fp64; returns (row, device array of the Hessians)"""
    lib = dzo.lib()
    n3, es = 3 * n, 8
    eye = dzo.DeviceArray.from_host(np.eye(n3).ravel())
    out = dzo.DeviceArray.zeros(n3 * n3 * REPLICAS)
    hvp, radial, f64 = lib.dzo_pairwise_hvp, dzo.RADIAL_LENNARD_JONES, dzo.F64

    def replica(k):
        x = points.ptr + es * n3 * k
        base = out.ptr + es * n3 * n3 * k
        for c in range(n3):
            col, e = base + es * n3 * c, eye.ptr + es * n3 * c
            rc = hvp(radial, n, f64, col, col + es * n, col + es * 2 * n, x, x + es * n, x + es * 2 * n, e, e + es * n, e + es * 2 * n)
            if rc:
                dzo._check(rc)

    replica(0)                                               # warm-up
    seconds = []
    for _ in range(passes):
        dzo.synchronize()
        t0 = time.perf_counter()
        for k in range(REPLICAS):
            replica(k)
        dzo.synchronize()
        seconds.append(time.perf_counter() - t0)
    calls = REPLICAS * n3
    return {"n": n, "dtype": "float64", "instances_run": REPLICAS, "which": "all 256", "calls_per_pass": calls, "passes": passes,
            "seconds_host_clock_median": float(np.median(seconds)), "seconds_host_clock_min_max": [float(min(seconds)), float(max(seconds))],
            "us_per_call": float(np.median(seconds)) / calls * 1e6}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_batch_bench.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--baseline-repeats", type=int, default=3)
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
           "workload": f"the dense Hessians of {REPLICAS} replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps and quenched by BatchedLBFGS",
           "hessian_runs": [], "hvp_runs": [], "baseline": [], "kernels": bq.kernel_figures(lib_path, "hess_batch_")}
    keep = None
    for dtype in (np.float64, np.float32):
        for n in (38, 13, 200):
            points, opt = quenched(dzo, n, dtype)
            row, out = hessian_case(dzo, points, n, dtype, args.repeats)
            row["instances_stuck_after_quench"] = int(opt.is_stuck.sum())
            res["hessian_runs"].append(row)
            print(json.dumps(row), flush=True)
            if n == 38:
                hv = hvp_case(dzo, points, n, dtype, args.repeats)
                res["hvp_runs"].append(hv)
                print(json.dumps(hv), flush=True)
            if n == 38 and dtype == np.float64:
                keep = (points, opt, row, out)
            else:
                out.free()
    if args.baseline_repeats > 0:
        points, opt, row, out = keep
        base, base_out = baseline_case(dzo, points, 38, args.baseline_repeats)
        a, b = out.to_host(), base_out.to_host()
        finite = np.isfinite(a) & np.isfinite(b)
        base["largest_difference_to_the_batched_hessians"] = float(np.abs(a[finite] - b[finite]).max())
        base["largest_entry"] = float(np.abs(a[finite]).max())
        base["entries_not_finite_in_either"] = int((~finite).sum())
        res["baseline"].append(base)
        print(json.dumps(base), flush=True)
        new_us = row["call_us_host_clock"]["median"]
        res["comparison_n38_f64"] = {"batched_call_us_host_clock": new_us, "batched_kernel_us_device_events": row["kernel_us_device_events"]["median"],
                                     "baseline_us_for_256": base["seconds_host_clock_median"] * 1e6,
                                     "ratio_host_clock": base["seconds_host_clock_median"] * 1e6 / new_us,
                                     "batched_is_faster": bool(new_us < base["seconds_host_clock_median"] * 1e6)}
        print(json.dumps(res["comparison_n38_f64"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
