"""Measurement of batched eigenvector following (dzo_modefollow_batch_*, csrc/dzo_modefollow.hip) on the device: recorded, not
gated.

    python tools/bench_modefollow.py [--out profiles/modefollow_bench.json] [--repeats 3] [--baseline-steps 10]
    python tools/bench_modefollow.py --readme profiles/modefollow_bench.json   # no device: rewrite the README paragraph from a result

Workload: the tempered replicas of tools/bench_quench.py (256 replicas of the 38-atom Lennard-Jones cluster, fixed seed, 20
batches of 500 steps), quenched by one BatchedLBFGS handle.  Then (1) polish: target index 0 until grms <= 1e-10; (2) saddles:
every polished minimum displaced by 0.05 along its lowest non-zero mode, target index 1 with max_step 0.1, at most 300 steps.

New path: dzo.ModeFollowing -- per step the Hessians, the eigensolver with vectors and the step kernel on one stream, one host
wait per 10 steps.  Host clock around the whole run of a fresh copy, `repeats` times after a warm-up; next to it the three
kernels of a step by the library's HIP events (dzo_profile_*), in a run of their own.

Baseline: the path a user had before, per step and on all 256 replicas: dzo.hessian_spectrum(vectors=True) (Hessians and
eigensolver on the device, eigenvalues and 26.6 MB of eigenvectors copied back), the numpy twin's step (tests/modefollow_twin.py)
instance after instance, the points uploaded again.  It walks the same path step for step, so `baseline-steps` steps are timed
and the cost is given per step; how fast its host part is depends on the host's numpy and CPU.
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

MARKERS = ("<!-- modefollow-readme -->", "<!-- /modefollow-readme -->")
N, ZERO_TOL, GRAD_TOL, KICK = 38, 1e-4, 1e-10, 0.05
WORKLOADS = {"polish": dict(target_index=0, max_step=0.2, max_steps=50), "saddles": dict(target_index=1, max_step=0.1, max_steps=300)}
KERNELS = ("modefollow_hessian", "modefollow_eigen", "modefollow_step")


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def device_run(dzo, start, dirs, target_index, max_step, max_steps):
    """One run of the handle on a fresh copy: (host seconds, handle, the copy)."""
    pts = start.copy()
    dzo.synchronize()
    t0 = time.perf_counter()
    mf = dzo.ModeFollowing(pts, N, target_index, max_step, ZERO_TOL, GRAD_TOL)
    if dirs is not None:
        mf.set_directions(dirs)
    mf.run(max_steps, steps_per_call=10)
    return time.perf_counter() - t0, mf, pts


def baseline_steps(dzo, mt, start, dirs, target_index, max_step, steps):
    """`steps` steps of the path there was before, on all instances: seconds per step, and the points it reached."""
    pts = start.copy()
    batch = pts.size // (3 * N)
    w = None if dirs is None else dirs.copy()
    status = np.zeros(batch, dtype=np.int32)
    times = []
    for _ in range(steps):
        dzo.synchronize()
        t0 = time.perf_counter()
        lam, vec = dzo.hessian_spectrum(pts, N, vectors=True)
        x = pts.to_host().reshape(batch, 3 * N)
        for b in range(batch):
            if status[b] != mt.ACTIVE:
                continue
            r = mt.step(x[b], lam[b], vec[b].T, None if w is None else w[b], w is not None, target_index, 0, max_step, ZERO_TOL, GRAD_TOL)
            status[b], x[b] = r["status"], r["point"]
            if w is not None and r["w"] is not None:
                w[b] = r["w"]
        pts.upload(x)
        dzo.synchronize()
        times.append(time.perf_counter() - t0)
    return times, pts.to_host().reshape(batch, 3 * N)


def workload_case(dzo, mt, name, start, dirs, repeats, base_steps):
    cfg = WORKLOADS[name]
    device_run(dzo, start, dirs, **cfg)                      # warm-up: loads the code objects
    host, mf = [], None
    for _ in range(repeats):
        seconds, mf, pts = device_run(dzo, start, dirs, **cfg)
        host.append(seconds * 1e3)
    status, index, zeros, iters = mf.status, mf.index, mf.zeros, mf.iteration_counts
    steps_enqueued = int(10 * np.ceil((iters.max() + 1) / 10.0)) if mf.count_active() == 0 else cfg["max_steps"]
    dzo.profile_enable(2)
    dzo.profile_reset()
    device_run(dzo, start, dirs, **cfg)
    table = dzo.profile_table()
    dzo.profile_enable(0)
    per_launch = {k: {"launches": int(table[k][0]), "us_per_launch": 1e3 * table[k][1] / table[k][0]} for k in KERNELS}
    want = cfg["target_index"]
    row = {"workload": name, "n_particles": N, "n": 3 * N, "dtype": "float64", "instances": int(len(status)), "repeats": repeats, **cfg,
           "zero_tol": ZERO_TOL, "grad_tol": GRAD_TOL, "run_ms_host_clock": stats(host), "steps_enqueued": steps_enqueued,
           "ms_per_step_host_clock": float(np.median(host)) / steps_enqueued,
           "converged": int((status == dzo.MODEFOLLOW_CONVERGED).sum()), "failed": int((status == dzo.MODEFOLLOW_FAILED).sum()),
           "converged_with_target_index_and_six_zeros": int(((status == dzo.MODEFOLLOW_CONVERGED) & (index == want) & (zeros == 6)).sum()),
           "moves": {"min": int(iters.min()), "median": float(np.median(iters)), "max": int(iters.max())},
           "largest_grms_of_converged": float(mf.grms[status == dzo.MODEFOLLOW_CONVERGED].max()) if (status == dzo.MODEFOLLOW_CONVERGED).any() else None,
           "kernels_us_device_events": per_launch,
           "step_kernel_over_eigensolver": per_launch["modefollow_step"]["us_per_launch"] / per_launch["modefollow_eigen"]["us_per_launch"]}
    if base_steps > 0:
        times, reached = baseline_steps(dzo, mt, start, dirs, cfg["target_index"], cfg["max_step"], base_steps)
        # the same walk: the handle's points after as many steps
        pts = start.copy()
        check = dzo.ModeFollowing(pts, N, cfg["target_index"], cfg["max_step"], ZERO_TOL, GRAD_TOL)
        if dirs is not None:
            check.set_directions(dirs)
        check.step(base_steps)
        row["baseline_ms_per_step_host_clock"] = stats([t * 1e3 for t in times[1:]] or [t * 1e3 for t in times])
        row["baseline_steps_timed"] = base_steps
        row["baseline_eigenvector_bytes_copied_per_step"] = int(len(status) * (3 * N) ** 2 * 8)
        row["largest_point_difference_after_baseline_steps"] = float(np.abs(check.current_points - reached).max())
        row["ratio_per_step_host_clock"] = row["baseline_ms_per_step_host_clock"]["median"] / row["ms_per_step_host_clock"]
        check.close()
    return row, mf, pts


def readme_paragraph(res):
    rows = {r["workload"]: r for r in res["runs"]}
    p, s = rows["polish"], rows["saddles"]
    k = s["kernels_us_device_events"]
    text = ("Measured %s on top of commit %s (`profiles/modefollow_bench.json`), 256 tempered and quenched replicas of the 38-atom cluster, "
            "fp64. Polish (`target_index = 0`, `grad_tol = 1e-10`): %d of 256 CONVERGED with index 0 and six zeros after %d–%d moves, "
            "%.1f ms for the whole run by the host clock (%.2f ms per enqueued step), against %.0f ms PER STEP for the path there was "
            "before (`dzo.hessian_spectrum(vectors=True)`, %.1f MB of eigenvectors copied back, the numpy step instance after instance, "
            "upload; all 256 run): a ratio of %.1f per step. Saddles (`target_index = 1`, kick 0.05, `max_step = 0.1`, at most %d steps): "
            "%d of 256 CONVERGED on index-1 stationary points with six zeros (%d CONVERGED in all) after %d–%d moves, %.0f ms for the run "
            "(%.2f ms per step) against %.0f ms per step before: a ratio of %.1f. Within a step the eigensolver dominates: Hessians "
            "%.0f µs, eigensolver %.2f ms, step kernel %.0f µs per launch by device events -- the step kernel takes %.1f %% of the "
            "eigensolver's time."
            % (res["date"], res["parent_commit"], p["converged_with_target_index_and_six_zeros"], p["moves"]["min"], p["moves"]["max"],
               p["run_ms_host_clock"]["median"], p["ms_per_step_host_clock"], p["baseline_ms_per_step_host_clock"]["median"],
               p["baseline_eigenvector_bytes_copied_per_step"] / 1e6, p["ratio_per_step_host_clock"], s["max_steps"],
               s["converged_with_target_index_and_six_zeros"], s["converged"], s["moves"]["min"], s["moves"]["max"],
               s["run_ms_host_clock"]["median"], s["ms_per_step_host_clock"], s["baseline_ms_per_step_host_clock"]["median"],
               s["ratio_per_step_host_clock"], k["modefollow_hessian"]["us_per_launch"], k["modefollow_eigen"]["us_per_launch"] / 1e3,
               k["modefollow_step"]["us_per_launch"], 100.0 * s["step_kernel_over_eigensolver"]))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modefollow_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-steps", type=int, default=10)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    ap.add_argument("--readme", default=None, metavar="JSON", help="rewrite the README paragraph from this result and exit (no device)")
    args = ap.parse_args()
    if args.readme:
        write_readme(json.load(open(args.readme)))
        return
    import bench_quench as bq
    import modefollow_twin as mt
    from dzo_loader import dzo
    lib_path = dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit,
           "workload": f"{bq.REPLICAS} replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps and quenched by BatchedLBFGS; polish, then "
                       "saddle searches from the polished minima",
           "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)), "runs": [],
           "kernels": bq.kernel_figures(lib_path, "modefollow_")}
    replicas = bq.tempered_replicas(dzo, N, np.float64)
    dzo.profile_enable(2)                                    # quench_once reads its launches' times
    _, _, _, opt = bq.quench_once(dzo, replicas, N)
    dzo.profile_enable(0)
    row, polished, minima = workload_case(dzo, mt, "polish", opt.points, None, args.repeats, args.baseline_steps)
    res["runs"].append(row)
    print(json.dumps(row), flush=True)
    # the kick along the lowest non-zero mode of every polished minimum (dzo.find_saddles does the same)
    lam, vec, x = polished.eigenvalues, polished.eigenvectors, polished.current_points
    dirs = np.stack([vec[b, np.flatnonzero(np.abs(lam[b]) > ZERO_TOL)[0]] for b in range(len(lam))])
    start = dzo.DeviceArray.from_host(x + KICK * dirs)
    row, _, _ = workload_case(dzo, mt, "saddles", start, dirs, args.repeats, args.baseline_steps)
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
