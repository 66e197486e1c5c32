"""Measurement of the batched lowest Hessian mode (dzo_pairwise_batch_lowest_mode, csrc/dzo_lowmode.hip) on the device: recorded,
not gated.

    python tools/bench_lowmode.py [--out profiles/lowmode_bench.json] [--repeats 3]
    python tools/bench_lowmode.py --readme profiles/lowmode_bench.json   # no device: rewrite the README paragraph from a result

Workloads: 256 replicas of the 38-atom Lennard-Jones cluster and 64 replicas of a 200-atom cluster, tempered (fixed seed, 20
batches of 500 steps) and quenched by one BatchedLBFGS handle each.

New path: ONE dzo.lowest_modes call per workload (rigid-body motions projected out, 32 Lanczos vectors per cycle, the default
residual of the element type, starts drawn in the kernel).  Host clock around the call, `repeats` times after a warm-up, median;
next to it the kernel by the library's HIP events (dzo_profile_*), in a run of its own; products and cycles per instance.  The
same call once more in fp64 with the relative residual 1e-6, which is enough for the SIGN of the lowest mode (minimum or saddle).

Baseline at N = 38, same session: dzo.hessian_spectrum, the dense Hessians into the full Jacobi eigensolver on the device, which
returns all 114 eigenvalues where one is wanted.  Baseline at N = 200, where no device path exists (the eigensolver stops at 128
particles): dzo.hessian_eigenvalues, the Hessians copied to the HOST and numpy.linalg.eigvalsh matrix after matrix; how fast
that is depends on the host's numpy and CPU.  Agreement: at an instance the dense spectrum calls a minimum (six eigenvalues
within 1e-5 of the largest around zero, none below), the lowest mode against dense eigenvalue 6.
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

MARKERS = ("<!-- lowmode-readme -->", "<!-- /lowmode-readme -->")
WORKLOADS = [dict(n=38, replicas=256, baseline="hessian_spectrum"), dict(n=200, replicas=64, baseline="hessian_eigenvalues")]
KRYLOV, MAX_CYCLES = 32, 200
SIGN_CHECK_TOL = 1e-6                                        # enough to tell a minimum from a saddle: the sign of the lowest mode


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def spread(v):
    return {"min": int(np.min(v)), "median": float(np.median(v)), "max": int(np.max(v))}


def quenched_replicas(dzo, bq, n, replicas):
    """`replicas` tempered and quenched clusters of n atoms, fp64, on the device (the recipe of tools/bench_quench.py)."""
    from bench_tempering import start_replicas
    radius = 2.25 * (n / 38.0) ** (1.0 / 3.0)
    dev = dzo.DeviceArray.from_host(start_replicas(n, replicas, radius, np.float64).reshape(-1))
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), replicas))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(replicas, 0.05), radius, 1)
    pt.run(bq.STEPS, bq.BATCHES)
    dzo.synchronize()
    dzo.profile_enable(2)                                    # quench_once reads its launches' times
    _, _, _, opt = bq.quench_once(dzo, dev, n)
    dzo.profile_enable(0)
    return opt.points.copy(), int(opt.count_active())


def timed(dzo, call, repeats):
    call()                                                   # warm-up: loads the code objects
    ms, out = [], None
    for _ in range(repeats):
        dzo.synchronize()
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def lowmode_case(dzo, points, n, dtype, repeats, tol=None):
    pts = points if np.dtype(dtype) == points.dtype else dzo.DeviceArray.from_host(points.to_host().astype(dtype))
    tol = dzo.LOWMODE_DEFAULT_RES_TOL[np.dtype(dtype)] if tol is None else tol
    call = lambda: dzo.lowest_modes(pts, n, project_rigid=True, krylov=KRYLOV, max_cycles=MAX_CYCLES, res_tol=tol, seed=1)
    ms, r = timed(dzo, call, repeats)
    dzo.profile_enable(2)
    dzo.profile_reset()
    call()
    table = dzo.profile_table()
    dzo.profile_enable(0)
    row = {"dtype": np.dtype(dtype).name, "krylov": KRYLOV, "max_cycles": MAX_CYCLES, "res_tol": tol, "call_ms_host_clock": stats(ms),
           "kernel_ms_device_events": float(table["lowmode"][1] / table["lowmode"][0]),
           "converged": int((r.status == dzo.LOWMODE_CONVERGED).sum()), "unfinished": int((r.status == dzo.LOWMODE_UNFINISHED).sum()),
           "failed": int((r.status == dzo.LOWMODE_FAILED).sum()), "products_per_instance": spread(r.products), "cycles_per_instance": spread(r.cycles),
           "negative_lowest_modes": int((r.eigenvalues < 0).sum()), "largest_residual": float(np.max(r.residuals))}
    return row, r


def agreement(lam, spectrum):
    """Over the instances the dense spectrum calls a minimum: (how many, the largest |lambda - eigenvalue 6|, the largest eigenvalue)."""
    tol = 1e-5 * spectrum[:, -1]
    minima = (spectrum[:, 0] > -tol) & (np.abs(spectrum[:, :6]) <= tol[:, None]).all(axis=1) & (spectrum[:, 6] > tol)
    diff = np.abs(lam.astype(np.float64) - spectrum[:, 6])[minima]
    return int(minima.sum()), (float(diff.max()) if minima.any() else None), float(spectrum[:, -1].max())


def readme_paragraph(res):
    rows = {r["n_particles"]: r for r in res["runs"]}
    a, b = rows[38], rows[200]
    a64, a32, b64, b32 = a["lowmode"]["float64"], a["lowmode"]["float32"], b["lowmode"]["float64"], b["lowmode"]["float32"]
    asc, bsc = a["lowmode"]["float64_sign_check"], b["lowmode"]["float64_sign_check"]
    text = ("Measured %s on top of commit %s (`profiles/lowmode_bench.json`), rigid-body motions projected out, 32 Lanczos vectors per cycle, "
            "relative residual %.1e (fp64) and %.1e (fp32), starts drawn in the kernel. 256 tempered and quenched replicas of the 38-atom cluster: "
            "ONE `dzo.lowest_modes` call takes %.2f ms by the host clock in fp64 (kernel %.2f ms by device events; %d–%d products in %d–%d cycles "
            "per instance, median %.0f; %d of 256 CONVERGED) and %.2f ms in fp32 (%d–%d products, %d CONVERGED), against %.2f ms for "
            "`dzo.hessian_spectrum` in the same session (dense Hessians and all 114 eigenvalues on the device): a ratio of %.1f in fp64. On the %d "
            "replicas the dense spectrum calls minima the lowest mode differs from dense eigenvalue 6 by at most %.1e (eigenvalues up to %.0f). "
            "64 replicas of a 200-atom cluster, where no dense device path exists (the eigensolver stops at 128 particles): %.2f ms in fp64 (kernel "
            "%.2f ms; %d–%d products, median %.0f; %d of 64 CONVERGED) and %.2f ms in fp32 (%d CONVERGED), against %.0f ms for "
            "`dzo.hessian_eigenvalues`, which copies %.0f MB of Hessians to the HOST and runs `numpy.linalg.eigvalsh` there: the comparison is with "
            "the host, a ratio of %.1f; largest difference from dense eigenvalue 6 over %d minima %.1e. The call returns when its slowest instance "
            "does, and the default residual asks for every digit the element type holds. Asked only for the SIGN of the lowest mode (fp64, relative "
            "residual %.0e): %.2f ms at N = 38 (%d–%d products, median %.0f) and %.2f ms at N = 200 (%d–%d products, median %.0f), with %d and %d "
            "signs different from the full-precision answer. Not measured: other batch sizes, other `krylov`, and how a cycle's time divides "
            "between the products, the reorthogonalisation and the small Jacobi iteration."
            % (res["date"], res["parent_commit"], a64["res_tol"], a32["res_tol"], a64["call_ms_host_clock"]["median"], a64["kernel_ms_device_events"],
               a64["products_per_instance"]["min"], a64["products_per_instance"]["max"], a64["cycles_per_instance"]["min"],
               a64["cycles_per_instance"]["max"], a64["products_per_instance"]["median"], a64["converged"], a32["call_ms_host_clock"]["median"],
               a32["products_per_instance"]["min"], a32["products_per_instance"]["max"], a32["converged"], a["baseline_ms_host_clock"]["median"],
               a["ratio_host_clock_fp64"], a["minima_by_dense_spectrum"], a["largest_difference_from_dense_eigenvalue_6"], a["largest_eigenvalue"],
               b64["call_ms_host_clock"]["median"], b64["kernel_ms_device_events"], b64["products_per_instance"]["min"],
               b64["products_per_instance"]["max"], b64["products_per_instance"]["median"], b64["converged"], b32["call_ms_host_clock"]["median"],
               b32["converged"], b["baseline_ms_host_clock"]["median"], b["baseline_hessian_bytes_copied"] / 1e6, b["ratio_host_clock_fp64"],
               b["minima_by_dense_spectrum"], b["largest_difference_from_dense_eigenvalue_6"], asc["res_tol"], asc["call_ms_host_clock"]["median"],
               asc["products_per_instance"]["min"], asc["products_per_instance"]["max"], asc["products_per_instance"]["median"],
               bsc["call_ms_host_clock"]["median"], bsc["products_per_instance"]["min"], bsc["products_per_instance"]["max"],
               bsc["products_per_instance"]["median"], a["sign_check_disagreements_with_default_tolerance"],
               b["sign_check_disagreements_with_default_tolerance"]))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowmode_bench.json"))
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
           "workload": f"replicas tempered for {bq.BATCHES} batches of {bq.STEPS} steps and quenched by BatchedLBFGS; one lowest_modes call",
           "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)), "repeats": args.repeats, "runs": [],
           "kernels": bq.kernel_figures(lib_path, "lowmode_")}
    for w in WORKLOADS:
        n, replicas = w["n"], w["replicas"]
        points, still_active = quenched_replicas(dzo, bq, n, replicas)
        row = {"n_particles": n, "n": 3 * n, "instances": replicas, "quench_instances_not_stuck": still_active, "lowmode": {}, "baseline": w["baseline"]}
        lam = None
        for dtype in (np.float64, np.float32):
            row["lowmode"][np.dtype(dtype).name], r = lowmode_case(dzo, points, n, dtype, args.repeats)
            if dtype is np.float64:
                lam = r.eigenvalues
        row["lowmode"]["float64_sign_check"], r = lowmode_case(dzo, points, n, np.float64, args.repeats, SIGN_CHECK_TOL)
        row["sign_check_disagreements_with_default_tolerance"] = int(((r.eigenvalues < 0) != (lam < 0)).sum())
        base = getattr(dzo, w["baseline"])
        ms, spectrum = timed(dzo, lambda: base(points, n), args.repeats)
        row["baseline_ms_host_clock"] = stats(ms)
        row["baseline_is_on"] = "device" if w["baseline"] == "hessian_spectrum" else "host (Hessians copied back, numpy.linalg.eigvalsh)"
        row["baseline_hessian_bytes_copied"] = 0 if w["baseline"] == "hessian_spectrum" else int(replicas * (3 * n) ** 2 * 8)
        row["ratio_host_clock_fp64"] = row["baseline_ms_host_clock"]["median"] / row["lowmode"]["float64"]["call_ms_host_clock"]["median"]
        (row["minima_by_dense_spectrum"], row["largest_difference_from_dense_eigenvalue_6"], row["largest_eigenvalue"]) = agreement(lam, spectrum)
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
