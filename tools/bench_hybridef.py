"""Measurement of batched hybrid eigenvector following (dzo_hybridef_batch_*, csrc/dzo_hybridef.hip) on the device: recorded, not
gated.

    python tools/bench_hybridef.py [--out profiles/hybridef_bench.json] [--repeats 3]
    python tools/bench_hybridef.py --readme profiles/hybridef_bench.json   # no device: rewrite the README paragraph from a result

Workloads, each in fp64 and fp32:

(a) the tempered replicas of tools/bench_quench.py (256 replicas of the 38-atom Lennard-Jones cluster, fixed seed, 20 batches of
    500 steps), quenched by one BatchedLBFGS handle, then `dzo.find_saddles_hybrid` (kick 0.05, at most 300 steps, one host wait
    per 20 steps).  In fp64, against `dzo.find_saddles` -- the dense path of the parent commit -- on the same starts in the same
    session.
(b) 64 replicas of a 200-atom cluster, tempered and quenched likewise: above the 128 particles the dense path stops at, so there
    is no device baseline.  A sample of the final points is checked by `dzo.hessian_eigenvalues` on the host.

Host clock around the whole run of a fresh copy (the lowest modes of the start, the kick, the handle, the steps), `repeats` times
after a warm-up run of the same size, median reported; next to it the two launches of a step by the library's HIP events
(dzo_profile_*), in a run of their own.  The index of a final point is the device spectrum's (`dzo.hessian_spectrum`) for
N = 38.  The dense baseline is timed once after its own warm-up step: its run takes seconds.
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

MARKERS = ("<!-- hybridef-readme -->", "<!-- /hybridef-readme -->")
KICK, MAX_STEPS, STEPS_PER_CALL = 0.05, 300, 20
# per element type: zero_tol and grad_tol.  fp32: the rigid-body eigenvalues are zeros to some 1e-4 only, and the gradient of a
# stationary point bottoms out near 1e-5 (tests/test_gpu_hybridef.py measures the floor of the 13-atom cluster)
TOLERANCES = {"float64": (1e-4, 1e-10), "float32": (1e-3, 3e-5)}
KERNELS = ("hybridef_mode", "hybridef_step")
SAMPLE = 4


def stats(v):
    v = np.asarray(v)
    return {"min": float(v.min()), "median": float(np.median(v)), "max": float(v.max())}


def tempered_and_quenched(dzo, bq, n, replicas, dtype):
    """`replicas` clusters of n atoms tempered like tools/bench_quench.py's and quenched to all_stuck: the DeviceArray."""
    radius = 2.25 * (n / 38.0) ** (1.0 / 3.0)
    reps = bq.start_replicas(n, replicas, radius, dtype)
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), replicas))
    dev = dzo.DeviceArray.from_host(reps.reshape(-1))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(replicas, 0.05), radius, 1)
    pt.run(bq.STEPS, bq.BATCHES)
    dzo.synchronize()
    opt = dzo.BatchedLBFGS(dev, n, 0.01, 10)
    done, taken = False, 0
    while not done and taken < bq.MAX_STEPS:
        done = opt.step(bq.STEPS_PER_LAUNCH)
        taken += bq.STEPS_PER_LAUNCH
    opt.close()
    return dev


def hybrid_run(dzo, start, n, zero_tol, grad_tol):
    """One search on a fresh copy: (host seconds, handle, the copy)."""
    pts = start.copy()
    dzo.synchronize()
    t0 = time.perf_counter()
    search = dzo.find_saddles_hybrid(pts, n, kick=KICK, grad_tol=grad_tol, max_steps=MAX_STEPS, zero_tol=zero_tol)
    return time.perf_counter() - t0, search, pts


def index_counts(dzo, points, n, zero_tol):
    """(negative, zero) eigenvalue counts of every point ((batch, 3n) host array) by the device spectrum in fp64."""
    ev = dzo.hessian_spectrum(dzo.DeviceArray.from_host(np.ascontiguousarray(points, dtype=np.float64)), n)
    return dzo.morse_index(ev, zero_tol)


def hybrid_case(dzo, start, n, dtype, repeats):
    zero_tol, grad_tol = TOLERANCES[dtype]
    hybrid_run(dzo, start, n, zero_tol, grad_tol)           # warm-up: loads the code objects
    host, search, pts = [], None, None
    for _ in range(repeats):
        seconds, search, pts = hybrid_run(dzo, start, n, zero_tol, grad_tol)
        host.append(seconds * 1e3)
    status, lam, iters = search.status, search.eigenvalues.astype(np.float64), search.iteration_counts
    converged = status == dzo.HYBRIDEF_CONVERGED
    dzo.profile_enable(2)
    dzo.profile_reset()
    hybrid_run(dzo, start, n, zero_tol, grad_tol)
    table = dzo.profile_table()
    dzo.profile_enable(0)
    per_launch = {k: {"launches": int(table[k][0]), "us_per_launch": 1e3 * table[k][1] / table[k][0]} for k in KERNELS}
    row = {"n_particles": n, "dtype": dtype, "instances": int(len(status)), "repeats": repeats, "kick": KICK, "max_steps": MAX_STEPS,
           "steps_per_host_wait": STEPS_PER_CALL, "zero_tol": zero_tol, "grad_tol": grad_tol, "run_ms_host_clock": stats(host),
           "converged": int(converged.sum()), "failed": int((status == dzo.HYBRIDEF_FAILED).sum()),
           "converged_with_negative_lowest_mode": int((converged & (lam < -zero_tol)).sum()),
           "outer_steps": stats(iters), "products": stats(search.products), "evaluations": stats(search.evaluations),
           "largest_grms_of_converged": float(search.grms[converged].max()) if converged.any() else None,
           "launches_us_device_events": per_launch}
    return row, search, pts


def dense_baseline(dzo, start, n):
    """`dzo.find_saddles` on a fresh copy, once: (host seconds, saddles handle)."""
    warm = start.copy()
    dzo.ModeFollowing(warm, n, 0).step(1)                    # loads the code objects
    pts = start.copy()
    dzo.synchronize()
    t0 = time.perf_counter()
    saddles, _ = dzo.find_saddles(pts, n, start_mode=0, kick=KICK, grad_tol=1e-10, max_steps=MAX_STEPS, max_step=0.1, zero_tol=1e-4)
    return time.perf_counter() - t0, saddles


def readme_paragraph(res):
    rows = {(r["n_particles"], r["dtype"]): r for r in res["runs"]}
    a, a32, b, b32 = rows[38, "float64"], rows[38, "float32"], rows[200, "float64"], rows[200, "float32"]
    base = a["dense_baseline"]
    k = a["launches_us_device_events"]
    text = ("Measured %s on top of commit %s (`profiles/hybridef_bench.json`). (a) 256 tempered and quenched replicas of the 38-atom cluster, "
            "fp64, `dzo.find_saddles_hybrid` (kick 0.05, at most 300 steps, one host wait per 20): %.0f ms for the whole run by the host "
            "clock (median of %d), %d of 256 CONVERGED, %d of them on index-1 saddles with six zeros by `dzo.hessian_spectrum`, after "
            "%d / %.0f / %d outer steps, %d / %.0f / %d products and %d / %.0f / %d gradient evaluations per instance (min / median / max). "
            "`dzo.find_saddles`, the dense path (its polish of the minima included, as the hybrid time includes `dzo.lowest_modes` at the "
            "minima), on the same starts in the same session: %.0f ms (timed once), %d index-1 saddles. The "
            "ratio dense / hybrid is %.2f in time and the hybrid search finds %+d saddles against it. Per launch by device events: the mode "
            "refinement %.0f µs, the step kernel %.0f µs. In fp32 (`grad_tol = %g`, `zero_tol = %g`): %.0f ms, %d CONVERGED, %d on "
            "index-1 saddles; the dense path was not measured in fp32. (b) 64 replicas of a 200-atom cluster, where no dense device path "
            "exists: fp64 %.0f ms, %d of 64 CONVERGED with a negative lowest mode after %d / %.0f / %d outer steps (mode refinement %.0f µs, "
            "step kernel %.0f µs per launch), %d of a sample of %d with index 1 by `dzo.hessian_eigenvalues` on the host (indices %s); "
            "fp32 %.0f ms, %d CONVERGED. Not measured: other sizes, other settings of `krylov`, `mode_cycles` and the tangent counts, "
            "and a second kick mode."
            % (res["date"], res["parent_commit"], a["run_ms_host_clock"]["median"], a["repeats"], a["converged"], a["index_1_with_six_zeros"],
               a["outer_steps"]["min"], a["outer_steps"]["median"], a["outer_steps"]["max"], a["products"]["min"], a["products"]["median"],
               a["products"]["max"], a["evaluations"]["min"], a["evaluations"]["median"], a["evaluations"]["max"], base["run_ms_host_clock"],
               base["index_1_with_six_zeros"], base["run_ms_host_clock"] / a["run_ms_host_clock"]["median"],
               a["index_1_with_six_zeros"] - base["index_1_with_six_zeros"], k["hybridef_mode"]["us_per_launch"], k["hybridef_step"]["us_per_launch"],
               a32["grad_tol"], a32["zero_tol"], a32["run_ms_host_clock"]["median"], a32["converged"], a32["index_1_with_six_zeros"],
               b["run_ms_host_clock"]["median"], b["converged_with_negative_lowest_mode"], b["outer_steps"]["min"], b["outer_steps"]["median"],
               b["outer_steps"]["max"], b["launches_us_device_events"]["hybridef_mode"]["us_per_launch"],
               b["launches_us_device_events"]["hybridef_step"]["us_per_launch"], sum(1 for i in b["sample_indices_host_spectrum"] if i == 1),
               len(b["sample_indices_host_spectrum"]), b["sample_indices_host_spectrum"], b32["run_ms_host_clock"]["median"], b32["converged"]))
    words, lines, line = text.split(" "), [], ""
    for w in words:
        if line and len(line) + 1 + len(w) > 140:
            lines.append(line)
            line = w
        else:
            line = (line + " " + w) if line else w
    return "\n".join(lines + [line])


def write_readme(res):
    path = os.path.join(ROOT, "README.md")
    text = open(path).read()
    i, j = text.index(MARKERS[0]) + len(MARKERS[0]), text.index(MARKERS[1])
    open(path, "w").write(text[:i] + "\n" + readme_paragraph(res) + "\n" + text[j:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybridef_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    ap.add_argument("--readme", default=None, metavar="JSON", help="rewrite the README paragraph from this result and exit (no device)")
    args = ap.parse_args()
    if args.readme:
        write_readme(json.load(open(args.readme)))
        return
    import bench_quench as bq
    from dzo_loader import dzo
    lib_path = dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit,
           "workload": f"replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps and quenched by BatchedLBFGS, then dzo.find_saddles_hybrid: "
                       "256 of 38 atoms (against dzo.find_saddles in fp64) and 64 of 200 atoms",
           "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)), "runs": [],
           "kernels": bq.kernel_figures(lib_path, "hybridef_")}
    for n, replicas in ((38, 256), (200, 64)):
        for dtype in ("float64", "float32"):
            start = tempered_and_quenched(dzo, bq, n, replicas, np.dtype(dtype))
            row, search, pts = hybrid_case(dzo, start, n, dtype, args.repeats)
            zero_tol = row["zero_tol"]
            points, converged = search.current_points, search.status == dzo.HYBRIDEF_CONVERGED
            if n == 38:
                neg, zer = index_counts(dzo, points, n, zero_tol)
                row["index_1_with_six_zeros"] = int((converged & (neg == 1) & (zer == 6)).sum())
                row["higher_index_stationary_points"] = int((converged & (neg > 1)).sum())
                if dtype == "float64":
                    seconds, saddles = dense_baseline(dzo, start, n)
                    st, ix, zr = saddles.status, saddles.index, saddles.zeros
                    row["dense_baseline"] = {"path": "dzo.find_saddles (polish, kick along the lowest non-zero mode, dense eigenvector following)",
                                             "run_ms_host_clock": seconds * 1e3, "timed": "once, after a warm-up step",
                                             "converged": int((st == dzo.MODEFOLLOW_CONVERGED).sum()),
                                             "index_1_with_six_zeros": int(((st == dzo.MODEFOLLOW_CONVERGED) & (ix == 1) & (zr == 6)).sum()),
                                             "outer_steps": stats(saddles.iteration_counts)}
                    row["ratio_dense_over_hybrid_host_clock"] = seconds * 1e3 / row["run_ms_host_clock"]["median"]
                    saddles.close()
            else:
                which = np.flatnonzero(converged)[:SAMPLE]
                sample = dzo.DeviceArray.from_host(np.ascontiguousarray(points[which], dtype=np.float64))
                ev = dzo.hessian_eigenvalues(sample, n) if len(which) else np.zeros((0, 3 * n))
                row["sample_instances"] = which.tolist()
                row["sample_indices_host_spectrum"] = [int((e < -zero_tol).sum()) for e in ev]
                row["sample_zeros_host_spectrum"] = [int((np.abs(e) <= zero_tol).sum()) for e in ev]
                row["sample_lowest_eigenvalue_host_spectrum"] = [float(e[0]) for e in ev]
                row["sample_lowest_mode_of_the_search"] = search.eigenvalues[which].astype(np.float64).tolist()
            search.close()
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    print(readme_paragraph(res))


if __name__ == "__main__":
    main()
