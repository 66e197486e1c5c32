"""Measurement of the batched nudged elastic band (dzo_neb_batch_*, csrc/dzo_neb.hip): recorded, not gated.

    python tools/bench_neb.py [--out profiles/neb_bench.json] [--repeats 3]
    python tools/bench_neb.py --readme profiles/neb_bench.json   # no device: rewrite the README paragraph from a result

Per element type (fp64, fp32): 256 bands of 9 images of the 38-atom Lennard-Jones cluster, between the end pairs that
`dzo.connect_saddles` returns for the saddles `dzo.find_saddles_hybrid` finds from the 256 tempered and quenched replicas of
tools/bench_quench.py.  `dzo.ElasticBand` runs to all_done (at most MAX_ITERATIONS iterations, STEPS_PER_CALL per launch): host
clock around the run, `repeats` times after a warm-up, median reported, and the launches by the library's HIP events.

The baseline is the only path there was before: per iteration ONE `dzo.pairwise_batch_energy_gradient` over all 9 * 256 images,
a download, the tangents, forces and the move in vectorised numpy (fp64 sums, numpy's order: the same rule, not the same bits),
and an upload, for as many iterations as the slowest band of the device run took.  Timed once."""
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

MARKERS = ("<!-- neb-readme -->", "<!-- /neb-readme -->")
N, REPLICAS, IMAGES = 38, 256, 9
MAX_ITERATIONS, STEPS_PER_CALL = 6000, 200
SPRING, DT, MAX_MOVE, CLIMB_AFTER = 1.0, 0.02, 0.1, 50
# float32: the tests hold 7-atom bands to 1e-5, the floor the float32 twin reaches THERE; what 38-atom bands reach has not been
# measured, and a residual's rounding grows with the forces it is the difference of, so the timing asks for ten times that
FORCE_TOL = {"float64": 1e-6, "float32": 1e-4}
SEARCH_TOLERANCES = {"float64": (1e-4, 1e-10), "float32": (1e-3, 3e-5)}     # zero_tol, grad_tol: tools/bench_hybridef.py
CONNECT = {"float64": (0.03, 1.4e-4), "float32": (0.03, 8.1e-4)}             # displacement, tol: the structure block of README.md


def numpy_iteration(x, v, e, g, iteration, force_tol, active):
    """The rule of include/dzo.h on all bands at once: x, v, g (B, M, 3N), e (B, M); moves the active bands in place."""
    B, M, n = x.shape
    dp, dm = x[:, 2:] - x[:, 1:-1], x[:, 1:-1] - x[:, :-2]
    ep, e0, em = e[:, 2:, None], e[:, 1:-1, None], e[:, :-2, None]
    hi, lo = np.maximum(np.abs(ep - e0), np.abs(em - e0)), np.minimum(np.abs(ep - e0), np.abs(em - e0))
    mixed = np.where(ep > em, hi * dp + lo * dm, lo * dp + hi * dm)
    t = np.where((ep > e0) & (e0 > em), dp, np.where((ep < e0) & (e0 < em), dm, mixed)).astype(np.float64)
    t /= np.sqrt((t * t).sum(axis=2, keepdims=True))
    gi = g[:, 1:-1].astype(np.float64)
    c = (gi * t).sum(axis=2, keepdims=True)
    w = SPRING * (np.sqrt((dp.astype(np.float64) ** 2).sum(axis=2, keepdims=True)) - np.sqrt((dm.astype(np.float64) ** 2).sum(axis=2, keepdims=True)))
    F = -(gi - c * t) + w * t
    if iteration >= CLIMB_AFTER:
        top = np.argmax(e[:, 1:-1], axis=1)
        rows = np.arange(B)
        F[rows, top] = -gi[rows, top] + 2.0 * c[rows, top] * t[rows, top]
    ff = (F * F).sum(axis=2, keepdims=True)
    active &= np.sqrt(ff.max(axis=1)[:, 0] / n) > force_tol
    F = F.astype(x.dtype)
    vi = v[:, 1:-1]
    p = (vi.astype(np.float64) * F).sum(axis=2, keepdims=True)
    vi = np.where(p > 0, (p / ff) * F, 0.0).astype(x.dtype) + x.dtype.type(DT) * F
    s = x.dtype.type(DT) * vi
    sn = np.sqrt((s.astype(np.float64) ** 2).sum(axis=2, keepdims=True))
    s = np.where(sn > MAX_MOVE, (MAX_MOVE / sn) * s, s).astype(x.dtype)
    x[active, 1:-1] += s[active]
    v[active, 1:-1] = vi[active]


def baseline(dzo, straight, iterations, force_tol):
    """(seconds, bands converged): `iterations` iterations of all bands with the device evaluating and the host doing the rest."""
    band = straight.copy()
    B, M, n = band.shape
    gdev = dzo.DeviceArray((B * M, n), band.dtype)
    x, v = band.to_host().reshape(B, M, n), np.zeros((B, M, n), dtype=band.dtype)
    active = np.ones(B, dtype=bool)
    dzo.synchronize()
    t0 = time.perf_counter()
    for it in range(iterations):
        e = dzo.pairwise_batch_energy_gradient(band, N, gdev).reshape(B, M)
        g = gdev.to_host().reshape(B, M, n)
        numpy_iteration(x, v, e, g, it, force_tol, active)
        band.upload(x)
    dzo.synchronize()
    return time.perf_counter() - t0, int((~active).sum())


def device_run(dzo, straight, force_tol):
    band = straight.copy()
    dzo.synchronize()
    dzo.profile_reset()
    t0 = time.perf_counter()
    neb = dzo.ElasticBand(band, N, IMAGES, SPRING, DT, MAX_MOVE, force_tol=force_tol, climb_after=CLIMB_AFTER)
    neb.run(MAX_ITERATIONS, STEPS_PER_CALL)
    wall = time.perf_counter() - t0
    table = dzo.profile_table()
    return wall, table.get("neb_step", (0, 0.0)), neb


def readme_paragraph(res):
    out = ["Measured %s on top of commit %s (`profiles/neb_bench.json`): %d bands of %d images of the %d-atom cluster between the end pairs "
           "`dzo.connect_saddles` returns, `dzo.ElasticBand` (spring %g, dt %g, max_move %g, climbing after %d iterations) run to all_done with "
           "one host wait per %d iterations, at most %d." % (res["date"], res["parent_commit"], res["bands"], IMAGES, N, SPRING, DT, MAX_MOVE,
                                                            CLIMB_AFTER, STEPS_PER_CALL, MAX_ITERATIONS)]
    for r in res["runs"]:
        it = r["iterations_per_band_min_median_max"]
        out.append("**%s** (`force_tol = %g`): %.0f ms by the host clock (median of %d; %d launches, %.0f ms by device events), %d of %d bands "
                   "CONVERGED, %d FAILED, after %d / %d / %d iterations per band (min / median / max); dynamic LDS %d bytes per band. The path "
                   "there was before (`dzo.pairwise_batch_energy_gradient` over all %d images, download, numpy, upload, per iteration) for the same "
                   "%d iterations: %.0f ms (once), %d bands converged; ratio %.1f." % (
                       r["dtype"], r["force_tol"], r["device_ms_host_clock_median"], r["repeats"], r["launches"], r["device_ms_events"], r["converged"],
                       res["bands"], r["failed"], it[0], it[1], it[2], r["lds_bytes"], IMAGES * res["bands"], r["baseline_iterations"],
                       r["baseline_ms_host_clock_once"], r["baseline_converged"], r["ratio_baseline_over_device"]))
    out.append("Not measured: other N, other image counts and batch sizes, the block shape and the device-memory storage, other springs and time "
               "steps, and how an iteration's time divides between the evaluations and the band arithmetic. Out of scope: rigid and permutational "
               "alignment of arbitrary end pairs (callers pass ends in a common frame, which `connect_saddles` output is), the doubly-nudged "
               "spring term, L-BFGS on the band, radials other than Lennard-Jones.")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neb_bench.json"))
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
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit, "n_particles": N,
           "n_images": IMAGES, "bands": REPLICAS, "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)), "runs": [],
           "kernels": bq.kernel_figures(lib_path, "neb_")}
    for dtype in ("float64", "float32"):
        dt = np.dtype(dtype)
        minima = bh.tempered_and_quenched(dzo, bq, N, REPLICAS, dt)
        dzo.quench_to_rest(minima, N)
        zero_tol, grad_tol = SEARCH_TOLERANCES[dtype]
        saddles = minima.copy()
        search = dzo.find_saddles_hybrid(saddles, N, kick=0.05, grad_tol=grad_tol, max_steps=300, zero_tol=zero_tol)
        modes = dzo.DeviceArray((REPLICAS, 3 * N), dt, ptr=search.ptr(dzo.HYBRIDEF_MODES), owner=False).copy()
        search.close()
        displacement, tol = CONNECT[dtype]
        paths = dzo.connect_saddles(saddles, modes, N, displacement, tol)
        ends = paths.ends
        a, b = ends.view(0, (REPLICAS, 3 * N)), ends.view(REPLICAS * 3 * N, (REPLICAS, 3 * N))
        straight = dzo.interpolate_band(a, b, N, IMAGES)
        force_tol = FORCE_TOL[dtype]
        device_run(dzo, straight, force_tol)[2].close()     # warm-up
        walls, neb, events = [], None, None
        for _ in range(args.repeats):
            if neb is not None:
                neb.close()
            wall, events, neb = device_run(dzo, straight, force_tol)
            walls.append(wall)
        status, counts = neb.status, neb.iteration_counts
        row = {"dtype": dtype, "force_tol": force_tol, "repeats": args.repeats, "device_ms_host_clock_median": 1e3 * float(np.median(walls)),
               "device_ms_host_clock_all": [1e3 * w for w in walls], "launches": int(events[0]), "device_ms_events": float(events[1]),
               "converged": int((status == dzo.NEB_CONVERGED).sum()), "failed": int((status == dzo.NEB_FAILED).sum()),
               "iterations_per_band_min_median_max": [int(counts.min()), int(np.median(counts)), int(counts.max())],
               "lds_bytes": dzo.neb_plan(N, IMAGES, dt)[2], "degenerate_end_pairs": int(paths.degenerate.sum())}
        neb.close()
        print(json.dumps(row), flush=True)
        iterations = int(counts.max())
        seconds, converged = baseline(dzo, straight, iterations, force_tol)
        row.update(baseline_iterations=iterations, baseline_ms_host_clock_once=1e3 * seconds, baseline_converged=converged,
                   ratio_baseline_over_device=1e3 * seconds / row["device_ms_host_clock_median"])
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
