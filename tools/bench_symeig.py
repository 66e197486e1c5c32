"""Measurement of the batched symmetric eigensolver (dzo_symmetric_batch_eigen, csrc/dzo_symeig.hip) on the device: recorded,
not gated.

    python tools/bench_symeig.py [--out profiles/symeig_bench.json] [--repeats 10] [--baseline-repeats 3]
    python tools/bench_symeig.py --readme profiles/symeig_bench.json      # no device: rewrite the README paragraph from a result

Workload: the tempered replicas of tools/bench_quench.py (256 replicas of the 38-atom Lennard-Jones cluster, fixed seed, 20
batches of 500 steps), quenched by one BatchedLBFGS handle; then the spectrum of the 114 x 114 Hessian of every replica, in fp64
and fp32.

New path: dzo.hessian_spectrum -- dzo_pairwise_batch_hessian into dzo_symmetric_batch_eigen on the device, the eigenvalues and
the sweep counts copied to the host.  Host clock around the call, `repeats` calls after a warm-up; next to it the eigensolver's
kernel alone by the library's HIP events (dzo_profile_*).

Baseline: the path there was before -- dzo.hessian_eigenvalues: every Hessian copied to the host, symmetrised in numpy,
numpy.linalg.eigvalsh matrix after matrix, all 256 run.  Host clock, `baseline-repeats` calls after a warm-up.  How fast that
is depends on the host's LAPACK and its threads; what the process can see of them is recorded.

Recorded with them: the sweeps per instance, and the largest eigenvalue difference between the two paths.  No ratio is asked
of either path.  For information: one row at N = 13, and one on MEMORY storage (3N = 192: N = 64, fp64) so that its cost is
known.
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

MARKERS = ("<!-- symeig-readme -->", "<!-- /symeig-readme -->")


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def spectrum_case(dzo, bq, n, dtype, repeats, baseline_repeats):
    replicas = bq.tempered_replicas(dzo, n, dtype)
    dzo.profile_enable(2)                                    # quench_once reads its launches' times
    _, _, _, opt = bq.quench_once(dzo, replicas, n)
    dzo.profile_enable(0)
    points = opt.points
    storage, ld, lds = dzo.symeig_plan(3 * n, dtype)
    ev = dzo.hessian_spectrum(points, n)                     # warm-up: loads the code object
    dzo.profile_enable(2)
    host, dev = [], []
    for _ in range(repeats):
        dzo.synchronize()
        dzo.profile_reset()
        t0 = time.perf_counter()
        ev = dzo.hessian_spectrum(points, n)
        host.append((time.perf_counter() - t0) * 1e6)
        launches, ms = dzo.profile_table()["symeig"]
        assert launches == 1
        dev.append(ms * 1e3)
    dzo.profile_enable(0)
    h = dzo.DeviceArray((bq.REPLICAS, 3 * n, 3 * n), dtype)
    dzo._check(dzo.lib().dzo_pairwise_batch_hessian(dzo.RADIAL_LENNARD_JONES, n, bq.REPLICAS, dzo._dt(dtype), points.ptr, h.ptr))
    _, _, sweeps = dzo.symmetric_batch_eigen(h, 3 * n)
    row = {"n_particles": n, "n": 3 * n, "dtype": np.dtype(dtype).name, "instances": bq.REPLICAS, "repeats": repeats,
           "storage": "lds" if storage == dzo.SYMEIG_STORAGE_LDS else "memory", "ld": ld, "dynamic_lds_bytes": lds,
           "instances_stuck_after_quench": int(opt.is_stuck.sum()),
           "hessian_spectrum_us_host_clock": stats(host), "symeig_kernel_us_device_events": stats(dev),
           "sweeps": {"min": int(sweeps.min()), "median": float(np.median(sweeps)), "max": int(sweeps.max()),
                      "not_converged": int((sweeps < 0).sum())}}
    if baseline_repeats > 0:
        old = dzo.hessian_eigenvalues(points, n)             # warm-up
        base = []
        for _ in range(baseline_repeats):
            dzo.synchronize()
            t0 = time.perf_counter()
            old = dzo.hessian_eigenvalues(points, n)
            base.append((time.perf_counter() - t0) * 1e6)
        row["hessian_eigenvalues_us_host_clock"] = stats(base)
        row["hessian_eigenvalues_us_per_matrix"] = float(np.median(base)) / bq.REPLICAS
        row["hessian_bytes_copied_to_the_host"] = int(h.nbytes)
        row["largest_eigenvalue_difference"] = float(np.abs(ev - old).max())
        row["largest_eigenvalue"] = float(np.abs(old).max())
        row["ratio_host_clock"] = float(np.median(base)) / float(np.median(host))
        row["device_path_is_faster"] = bool(np.median(host) < np.median(base))
    h.free()
    return row


def sci(x):
    e = int(np.floor(np.log10(abs(x))))
    return "%.1f·10%s" % (x / 10.0 ** e, str(e).translate(str.maketrans("-0123456789", "⁻⁰¹²³⁴⁵⁶⁷⁸⁹")))


def ratio(x):
    return "%.1f" % x if x < 100 else sci(x)


def ms(us):
    return "%.2f ms" % (us / 1e3) if us >= 1e3 else "%.0f µs" % us


def readme_paragraph(res):
    rows = {(r["n_particles"], r["dtype"]): r for r in res["runs"]}
    a, b = rows[(38, "float64")], rows[(38, "float32")]
    small, mem = rows[(13, "float64")], rows[(64, "float64")]
    verdict = ("a ratio of %s" % ratio(a["ratio_host_clock"]) if a["device_path_is_faster"] else
               "the device path is NOT faster at this size (a ratio of %.2f)" % a["ratio_host_clock"])
    text = ("Measured %s on top of commit %s (`profiles/symeig_bench.json`): the spectra of the 114 × 114 Hessians of 256 tempered and "
            "quenched replicas of the 38-atom cluster come from ONE `dzo.hessian_spectrum` call (Hessians and Jacobi sweeps on the device, "
            "eigenvalues copied back) in %s by the host clock in fp64 (eigensolver kernel %s, %d–%d sweeps per instance) and %s in fp32 "
            "(%d–%d sweeps), against %s for the path there was before, `dzo.hessian_eigenvalues`: %.1f MB of Hessians copied to the host and "
            "`numpy.linalg.eigvalsh` matrix after matrix (all 256 run, %s each): %s; %s in fp32. The two spectra differ by at "
            "most %s on eigenvalues up to %.0f. At N = 13 (39 × 39) the call takes %s against %s; on memory storage (N = 64, 192 × 192, fp64) "
            "%s against %s."
            % (res["date"], res["parent_commit"], ms(a["hessian_spectrum_us_host_clock"]["median"]), ms(a["symeig_kernel_us_device_events"]["median"]),
               a["sweeps"]["min"], a["sweeps"]["max"], ms(b["hessian_spectrum_us_host_clock"]["median"]), b["sweeps"]["min"], b["sweeps"]["max"],
               ms(a["hessian_eigenvalues_us_host_clock"]["median"]), a["hessian_bytes_copied_to_the_host"] / 1e6,
               ms(a["hessian_eigenvalues_us_per_matrix"]), verdict,
               ("a ratio of %s" % ratio(b["ratio_host_clock"]) if b["device_path_is_faster"] else "not faster (%.2f)" % b["ratio_host_clock"]),
               sci(a["largest_eigenvalue_difference"]), a["largest_eigenvalue"],
               ms(small["hessian_spectrum_us_host_clock"]["median"]), ms(small["hessian_eigenvalues_us_host_clock"]["median"]),
               ms(mem["hessian_spectrum_us_host_clock"]["median"]), ms(mem["hessian_eigenvalues_us_host_clock"]["median"])))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symeig_bench.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--baseline-repeats", type=int, default=3)
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
    try:
        import threadpoolctl
        blas = [{k: p.get(k) for k in ("internal_api", "version", "num_threads")} for p in threadpoolctl.threadpool_info()]
    except ImportError:
        blas = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit,
           "workload": f"the spectra of the dense Hessians of {bq.REPLICAS} replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps and "
                       "quenched by BatchedLBFGS",
           "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)),
           "host_thread_limits": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}, "host_blas": blas, "runs": [],
           "kernels": bq.kernel_figures(lib_path, "symeig_")}
    for n, dtype in ((38, np.float64), (38, np.float32), (13, np.float64), (64, np.float64)):
        row = spectrum_case(dzo, bq, n, dtype, args.repeats, args.baseline_repeats)
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
