"""Measurement of the batched alignment (dzo_align_batch_*, csrc/dzo_align.hip): recorded, not gated.

    python tools/bench_align.py [--out profiles/align_bench.json] [--repeats 3]
    python tools/bench_align.py --readme profiles/align_bench.json   # no device: rewrite the README paragraph from a result

Pairs of DISTINCT quenched minima of the Lennard-Jones cluster: replicas tempered and quenched as in tools/bench_quench.py, in
fp64, classified by `dzo.unique_structures`; distinct structure k is paired with distinct structure k + 1.  256 pairs at N = 38,
64 pairs at N = 200.  The fp32 runs take the same pairs rounded to fp32.  Per size and element type:

* one `dzo.align_pairs` call with its default options (the identity, the four principal starts, 8 random ones; 20 cycles at
  most): host clock around the call, `repeats` times after a warm-up, median reported, and the two launches by the library's
  HIP events; the distribution of cycles and of winning starts;
* the same work on the host: the points downloaded, then per pair and start (the same first rotations) the alternation of
  `scipy.optimize.linear_sum_assignment` on the squared distances with the rotation from numpy's SVD (Kabsch) until the
  permutation repeats, where scipy imports; else the test twin (tests/align_twin.py).  Timed once; the result says which;
* at N = 38, `dzo.connect_minima` with `align=True` against `align=False` on the same pairs at the settings of the neb-readme
  block: how many bands end CONVERGED and how many FAILED."""
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

MARKERS = ("<!-- align-readme -->", "<!-- /align-readme -->")
CASES = ((38, 256, 640), (200, 64, 96))                      # N, pairs, replicas tempered to find pairs + 1 distinct minima among
STRUCTURE_TOL = 1.4e-4                                       # the structure block of README.md (fp64)
RANDOM_TRIALS, MAX_CYCLES, SEED = 8, 20, 0
IMAGES, MAX_ITERATIONS, STEPS_PER_CALL = 9, 6000, 200         # tools/bench_neb.py
FORCE_TOL = {"float64": 1e-6, "float32": 1e-4}


def distinct_minima(dzo, bq, bh, n, count, replicas):
    """(count, 3n) host array of distinct fp64 minima, in the order the replicas gave them; fewer if there are fewer."""
    minima = bh.tempered_and_quenched(dzo, bq, n, replicas, np.dtype(np.float64))
    dzo.quench_to_rest(minima, n)
    _, reps, _, _ = dzo.unique_structures(minima, n, STRUCTURE_TOL)
    return minima.to_host().reshape(replicas, 3 * n)[reps[:count]], len(reps)


def host_alignment(a, b, n):
    """(seconds, distances, which): the default starts and the alternation on the host, from host arrays (pairs, 3n)."""
    import align_twin as at
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        t0 = time.perf_counter()
        d = [at.align(a[k], b[k], n, random_trials=RANDOM_TRIALS, max_cycles=MAX_CYCLES, seed=SEED).distance for k in range(len(a))]
        return time.perf_counter() - t0, np.array(d), "tests/align_twin.py"
    randoms = [at.random_rotation(SEED, r) for r in range(RANDOM_TRIALS)]
    t0 = time.perf_counter()
    out = np.empty(len(a))
    for k in range(len(a)):
        pa, pb = a[k].reshape(3, n).T.astype(np.float64), b[k].reshape(3, n).T.astype(np.float64)
        pa, pb = pa - pa.mean(axis=0), pb - pb.mean(axis=0)
        fa, fb = np.linalg.eigh(pa.T @ pa)[1], np.linalg.eigh(pb.T @ pb)[1]
        fa[:, 2] *= np.sign(np.linalg.det(fa))
        fb[:, 2] *= np.sign(np.linalg.det(fb))
        starts = [np.eye(3)] + [fa @ np.diag(s) @ fb.T for s in at.SIGNS] + randoms
        best = np.inf
        for rot in starts:
            prev = None
            for _ in range(MAX_CYCLES):
                moved = pb @ rot.T
                cost = ((pa[:, None, :] - moved[None, :, :]) ** 2).sum(axis=2)
                perm = linear_sum_assignment(cost)[1]
                u, _, vt = np.linalg.svd(pa.T @ pb[perm])
                sign = np.sign(np.linalg.det(u @ vt))
                rot = u @ np.diag([1.0, 1.0, sign]) @ vt
                if prev is not None and np.array_equal(prev, perm):
                    break
                prev = perm
            best = min(best, np.sqrt(((pa - pb[perm] @ rot.T) ** 2).sum()))
        out[k] = best
    return time.perf_counter() - t0, out, "scipy.optimize.linear_sum_assignment + numpy.linalg.svd"


def device_alignment(dzo, a, b, n):
    dzo.synchronize()
    dzo.profile_reset()
    t0 = time.perf_counter()
    r = dzo.align_pairs(a, b, n, random_trials=RANDOM_TRIALS, max_cycles=MAX_CYCLES, seed=SEED, want_trials=True)
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    return wall, sum(table.get(k, (0, 0.0))[1] for k in ("align_starts", "align_finish")), r


def band_counts(dzo, a, b, n, dtype, align):
    c = dzo.connect_minima(a, b, n, IMAGES, FORCE_TOL[dtype], max_iterations=MAX_ITERATIONS, steps_per_call=STEPS_PER_CALL, align=align)
    return {"converged": int((c.status == dzo.NEB_CONVERGED).sum()), "failed": int((c.status == dzo.NEB_FAILED).sum()),
            "active": int((c.status == dzo.NEB_ACTIVE).sum()), "median_residual": float(np.median(c.residuals)),
            "refined_saddles": int((c.saddle_status == dzo.HYBRIDEF_CONVERGED).sum())}


def readme_paragraph(res):
    out = ["Measured %s on top of commit %s (`profiles/align_bench.json`): pairs of distinct quenched minima (distinct structure k with k + 1 of "
           "tempered and quenched replicas, by `dzo.unique_structures`), one `dzo.align_pairs` call with its defaults (identity, four principal "
           "starts, %d random ones: 13 starts per pair, at most %d cycles each); host baseline: %s, per pair and start, after a download."
           % (res["date"], res["parent_commit"], RANDOM_TRIALS, MAX_CYCLES, res["host_method"])]
    for r in res["runs"]:
        cyc, win = r["cycles_histogram"], r["winning_start_kind"]
        out.append("**N = %d, %s**, %d pairs (%d distinct minima among %d replicas): %.2f ms by the host clock (median of %d; %.2f ms by device "
                   "events); %d CONVERGED, %d at the cycle limit; cycles of the winning start %d / %d / %d (min / median / max); the winner was "
                   "the identity %d, a principal start %d, a random start %d times; median distance %.4f against %.4f as the pairs came "
                   "(centred). Host: %.0f ms (once), ratio %.0f; the device distance is within 1e-9 of the host's on %d pairs, shorter on %d, "
                   "longer on %d." % (r["n_particles"], r["dtype"], r["pairs"], r["distinct_minima"], r["replicas"], r["device_ms_host_clock_median"],
                                      r["repeats"], r["device_ms_events"], r["converged"], r["cycle_limit"], cyc["min"], cyc["median"], cyc["max"],
                                      win["identity"], win["principal"], win["random"], r["median_distance"], r["median_raw_distance"],
                                      r["host_ms_once"], r["ratio_host_over_device"], r["host_same"], r["device_shorter"], r["device_longer"]))
        if "bands" in r:
            on, off = r["bands"]["align_true"], r["bands"]["align_false"]
            out.append("`dzo.connect_minima` on these pairs (%d images, `force_tol = %g`, at most %d iterations): with `align=True` %d bands "
                       "CONVERGED, %d FAILED and %d still ACTIVE at the limit (median residual %.2e); with `align=False` %d CONVERGED, %d FAILED "
                       "and %d still ACTIVE (median residual %.2e)."
                       % (IMAGES, FORCE_TOL[r["dtype"]], MAX_ITERATIONS, on["converged"], on["failed"], on["active"], on["median_residual"],
                          off["converged"], off["failed"], off["active"], off["median_residual"]))
    out.append("Not measured: the worst case at N = 1024 (bounded by N^2 / 2 column scans per assignment; the tests run the cheap, nearly aligned "
               "case there), other trial counts and cycle limits, `allow_inversion`, how a call's time divides between the scans and the "
               "rotations, and how often the best of 13 starts is the global minimum. Out of scope: several atom species, point-group symmetry "
               "detection, a guarantee of the global minimum.")
    words, lines, line = " ".join(out).split(" "), [], ""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    ap.add_argument("--readme", default=None, metavar="JSON", help="rewrite the README paragraph from this result and exit (no device)")
    args = ap.parse_args()
    if args.readme:
        write_readme(json.load(open(args.readme)))
        return
    import bench_hybridef as bh
    import bench_quench as bq
    from dzo_loader import dzo
    lib_path = dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    dzo.profile_enable(2)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit, "numpy": np.__version__,
           "host_cpus_visible": len(os.sched_getaffinity(0)), "random_trials": RANDOM_TRIALS, "max_cycles": MAX_CYCLES, "runs": [],
           "kernels": bq.kernel_figures(lib_path, "align_")}
    for n, pairs, replicas in CASES:
        minima, distinct = distinct_minima(dzo, bq, bh, n, pairs + 1, replicas)
        pairs = len(minima) - 1
        for dtype in ("float64", "float32"):
            dt = np.dtype(dtype)
            ha, hb = minima[:-1].astype(dt), minima[1:].astype(dt)
            a, b = dzo.DeviceArray.from_host(ha), dzo.DeviceArray.from_host(hb)
            device_alignment(dzo, a, b, n)                   # warm-up
            walls, events, r = [], 0.0, None
            for _ in range(args.repeats):
                wall, events, r = device_alignment(dzo, a, b, n)
                walls.append(wall)
            pa, pb = ha.reshape(pairs, 3, n).astype(np.float64), hb.reshape(pairs, 3, n).astype(np.float64)
            raw = np.sqrt((((pa - pa.mean(axis=2, keepdims=True)) - (pb - pb.mean(axis=2, keepdims=True))) ** 2).sum(axis=(1, 2)))
            kinds = np.where(r.best_trials == 0, 0, np.where(r.best_trials <= 4, 1, 2))
            row = {"n_particles": n, "dtype": dtype, "pairs": pairs, "replicas": replicas, "distinct_minima": distinct, "repeats": args.repeats,
                   "device_ms_host_clock_median": 1e3 * float(np.median(walls)), "device_ms_host_clock_all": [1e3 * w for w in walls],
                   "device_ms_events": float(events), "converged": int((r.status == dzo.ALIGN_CONVERGED).sum()),
                   "cycle_limit": int((r.status == dzo.ALIGN_CYCLE_LIMIT).sum()), "failed": int((r.status == dzo.ALIGN_FAILED).sum()),
                   "cycles_histogram": {"min": int(r.cycles.min()), "median": int(np.median(r.cycles)), "max": int(r.cycles.max()),
                                        "counts": np.bincount(r.cycles, minlength=MAX_CYCLES + 1).tolist()},
                   "winning_start_counts": np.bincount(r.best_trials, minlength=5 + RANDOM_TRIALS).tolist(),
                   "winning_start_kind": {"identity": int((kinds == 0).sum()), "principal": int((kinds == 1).sum()), "random": int((kinds == 2).sum())},
                   "median_distance": float(np.median(r.distances)), "median_raw_distance": float(np.median(raw)),
                   "lds_bytes_per_wave": 38 * n + 8}
            print(json.dumps(row), flush=True)
            seconds, host_d, method = host_alignment(ha, hb, n)
            res["host_method"] = method
            tol = 1e-9 * np.maximum(host_d, 1.0)
            row.update(host_ms_once=1e3 * seconds, ratio_host_over_device=1e3 * seconds / row["device_ms_host_clock_median"],
                       host_same=int((np.abs(r.distances - host_d) <= tol).sum()), device_shorter=int((r.distances < host_d - tol).sum()),
                       device_longer=int((r.distances > host_d + tol).sum()))
            if n == 38:
                row["bands"] = {"align_true": band_counts(dzo, a, b, n, dtype, True), "align_false": band_counts(dzo, a, b, n, dtype, False)}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    print(readme_paragraph(res))


if __name__ == "__main__":
    main()
