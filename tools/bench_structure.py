"""Measurement of the structure unit (dzo_structure_batch_fingerprint / _classify, csrc/dzo_structure.hip) and of
`dzo.connect_saddles` on the device: recorded, not gated.

    python tools/bench_structure.py [--out profiles/structure_bench.json] [--repeats 3]
    python tools/bench_structure.py --readme profiles/structure_bench.json   # no device: rewrite the README paragraph from a result

Per element type (fp64, fp32), on the 38-atom Lennard-Jones cluster:

(c) guidance for `tol`, measured first because the rest needs a `tol`: among the 256 tempered and quenched replicas of
    tools/bench_quench.py and the 4096 best points of (a) together (all brought to rest by `dzo.quench_to_rest`), the largest
    relative fingerprint distance (max_i |a_i - b_i| / max(1, |a_i|, |b_i|), what `tol` is compared with) between two instances that energy and
    `dzo.hessian_spectrum` agree are the same minimum, and the smallest between two instances of different energy.  `tol` for
    (a), (b) and (d) is the geometric mean of the two when they are a factor 100 apart, else nothing is recommended.
(a) `dzo.structure_fingerprints` + `dzo.classify_structures` on those 256 minima and on the BEST_POINTS of a 4096-walker basin
    hopping run, against the path there was before: download the points, the vectorised numpy fingerprint and the Python greedy
    loop of tests/structure_twin.py.
(b) the same on the end points of `dzo.find_saddles_hybrid` from the 256 minima; the number of distinct saddles among the
    CONVERGED ones with a negative lowest mode.
(d) `dzo.connect_saddles` on those saddles for displacement 1e-3, 3e-3, 1e-2, 3e-2, 1e-1: the share of saddles with two
    different ends, the share of ends not at rest after max_steps = 2000, the wall time.

Host clock around the calls, `repeats` times after a warm-up, median reported; next to it the three launches by the library's
HIP events (dzo_profile_*), in a run of their own.  The numpy baseline and the sweep are timed once: they take seconds.
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

MARKERS = ("<!-- structure-readme -->", "<!-- /structure-readme -->")
N, REPLICAS, WALKERS, HOPS = 38, 256, 4096, 16
KERNELS = ("structure_fingerprint", "structure_compare", "structure_label")
DISPLACEMENTS = (1e-3, 3e-3, 1e-2, 3e-2, 1e-1)
# two instances are "the same minimum" when their energies and their Hessian spectra agree to these (absolute, relative to the
# largest eigenvalue), and "of different energy" when the energies differ by more than the first
# fp32: 64 units in the last place of an energy of 170 (a row of 38 terms and a sum of 38 rows), and spectra of points that are
# right to some 1e-3 only
SAME = {"float64": (1e-8, 1e-5), "float32": (6.5e-4, 1e-2)}
SEARCH_TOLERANCES = {"float64": (1e-4, 1e-10), "float32": (1e-3, 3e-5)}     # zero_tol, grad_tol: tools/bench_hybridef.py


def median(v):
    return float(np.median(np.asarray(v)))


def tol_guidance(dzo, points, dtype):
    """`points`: the quenched replicas and the basin-hopping walkers' best points together, at rest."""
    fp, e = dzo.structure_fingerprints(points, N)
    F, e = fp.to_host().astype(np.float64), e.astype(np.float64)
    spectra = dzo.hessian_spectrum(dzo.DeviceArray.from_host(points.to_host().astype(np.float64)), N)
    e_tol, s_tol = SAME[dtype]
    top = np.abs(spectra).max()
    largest_same, smallest_different, same_pairs, different_pairs, other_spectrum = None, None, 0, 0, 0
    for k in range(len(e) - 1):
        rest = slice(k + 1, None)
        d = np.max(np.abs(F[rest] - F[k]) / np.maximum(1.0, np.maximum(np.abs(F[rest]), np.abs(F[k]))), axis=1)
        close = np.abs(e[rest] - e[k]) <= e_tol
        alike = np.abs(spectra[rest] - spectra[k]).max(axis=1) / top <= s_tol
        same, different = close & alike, ~close & np.isfinite(d)
        same_pairs, different_pairs, other_spectrum = same_pairs + int(same.sum()), different_pairs + int(different.sum()), other_spectrum + int((close & ~alike).sum())
        if same.any():
            largest_same = max(largest_same or 0.0, float(d[same].max()))
        if different.any():
            smallest_different = min(smallest_different or np.inf, float(d[different].min()))
    ratio = smallest_different / largest_same if largest_same and smallest_different else None
    row = {"instances": int(len(e)), "same_minimum_means": {"energies_within": e_tol, "spectra_within_relative": s_tol},
           "pairs_same_minimum": same_pairs, "pairs_of_different_energy": different_pairs, "pairs_same_energy_other_spectrum": other_spectrum,
           "largest_distance_same_minimum": largest_same, "smallest_distance_different_energy": smallest_different, "ratio": ratio}
    row["recommended_tol"] = float(np.sqrt(largest_same * smallest_different)) if ratio and ratio >= 100 else None
    return row


def identify(dzo, st, points, tol, repeats, baseline=True):
    """Times fingerprint + classify of `points` on the device and, once, the numpy path; the labels of both."""
    def device():
        dzo.synchronize()
        t0 = time.perf_counter()
        fp, e = dzo.structure_fingerprints(points, N)
        labels, reps = dzo.classify_structures(fp, tol)
        return (time.perf_counter() - t0) * 1e3, labels, reps, e

    device()                                                 # warm-up: loads the code objects
    runs = [device() for _ in range(repeats)]
    _, labels, reps, e = runs[-1]
    dzo.profile_enable(2)
    dzo.profile_reset()
    device()
    table = dzo.profile_table()
    dzo.profile_enable(0)
    row = {"instances": int(len(labels)), "tol": tol, "device_ms_host_clock_median": median([r[0] for r in runs]), "repeats": repeats,
           "launches_us_device_events": {k: 1e3 * table[k][1] / table[k][0] for k in KERNELS},
           "distinct": int(len(reps)), "not_finite": int((labels < 0).sum()), "largest_class": int(np.bincount(labels[labels >= 0]).max())}
    if baseline:
        t0 = time.perf_counter()
        host = points.to_host().reshape(len(labels), 3 * N)
        F, _ = st.fingerprints(host, N, host.dtype)
        twin_labels, _ = st.classify(F, tol)
        row["numpy_ms_host_clock_once"] = (time.perf_counter() - t0) * 1e3
        row["ratio_numpy_over_device"] = row["numpy_ms_host_clock_once"] / row["device_ms_host_clock_median"]
        row["labels_equal_the_numpy_path"] = bool(np.array_equal(labels, twin_labels))
    return row, labels, reps, e


def sweep(dzo, saddles, modes, is_saddle, tol):
    rows = []
    for d in DISPLACEMENTS:
        dzo.synchronize()
        t0 = time.perf_counter()
        paths = dzo.connect_saddles(saddles, modes, N, d, tol)
        wall = (time.perf_counter() - t0) * 1e3
        two = (paths.edges >= 0).all(axis=1) & ~paths.degenerate
        rows.append({"displacement": d, "wall_ms_once": wall, "saddles": int(is_saddle.sum()),
                     "share_of_saddles_with_two_different_ends": float(two[is_saddle].mean()) if is_saddle.any() else None,
                     "share_of_saddles_with_both_ends_in_one_minimum": float(paths.degenerate[is_saddle].mean()) if is_saddle.any() else None,
                     "share_of_ends_not_at_rest": float((~paths.end_stuck).mean()), "distinct_minima": int(len(paths.minimum_energies)),
                     "distinct_edges": len({tuple(sorted(e)) for e in paths.edges[is_saddle & two].tolist()})})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def readme_paragraph(res):
    out = ["Measured %s on top of commit %s on the 38-atom cluster (`profiles/structure_bench.json`)." % (res["date"], res["parent_commit"])]
    for r in res["runs"]:
        g, a, w, b = r["tol_guidance"], r["minima_256"], r["basin_hopping_best_4096"], r["saddles_256"]
        out.append("**%s.** `tol`: copies of one minimum (by energy and `dzo.hessian_spectrum`) are at most %.1e apart, two minima of "
                   "different energy at least %.1e (ratio %.0f); %s" % (
                       r["dtype"], g["largest_distance_same_minimum"], g["smallest_distance_different_energy"], g["ratio"],
                       "`tol = %.1e`, their geometric mean, is used below." % r["tol"] if g["recommended_tol"] else
                       "LESS THAN A FACTOR 100 APART: no value is recommended; %.1e, a tenth of the smaller, is used below and splits copies." % r["tol"]))
        for name, x in (("(a) the 256 quenched replicas", a), ("the 4096 BEST_POINTS of %d basin hops" % res["basin_hops"], w), ("(b) the 256 search ends", b)):
            k = x["launches_us_device_events"]
            out.append("%s: %d distinct, fingerprint + classify %.2f ms by the host clock (median of %d; launches by device events: %.0f + %.0f "
                       "+ %.0f µs), download + numpy + greedy loop %.0f ms (once), ratio %.0f, labels equal: %s." % (
                           name, x["distinct"], x["device_ms_host_clock_median"], x["repeats"], k["structure_fingerprint"], k["structure_compare"],
                           k["structure_label"], x["numpy_ms_host_clock_once"], x["ratio_numpy_over_device"], x["labels_equal_the_numpy_path"]))
        out.append("Of the %d CONVERGED ends with a negative lowest mode, %d are distinct saddles." % (b["saddles"], b["distinct_saddles"]))
        out.append("(d) `connect_saddles` (max_steps 2000), displacement / saddles with two different ends / ends not at rest / wall: " + "; ".join(
            "%g / %.0f %% / %.0f %% / %.0f ms" % (s["displacement"], 100 * s["share_of_saddles_with_two_different_ends"], 100 * s["share_of_ends_not_at_rest"],
                                              s["wall_ms_once"]) for s in r["displacement_sweep"]) + ".")
    out.append("Not measured: other N, other potentials, and mirror-image pairs (which the fingerprint cannot tell apart).")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    ap.add_argument("--readme", default=None, metavar="JSON", help="rewrite the README paragraph from this result and exit (no device)")
    args = ap.parse_args()
    if args.readme:
        write_readme(json.load(open(args.readme)))
        return
    import bench_hybridef as bh
    import bench_quench as bq
    import structure_twin as st
    from bench_tempering import start_replicas
    from dzo_loader import dzo
    lib_path = dzo.build()
    import torch  # noqa: F401  (loads the HIP runtime first)
    dzo.init(0)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": dzo.device_info(), "date": time.strftime("%Y-%m-%d"), "parent_commit": args.commit or commit, "n_particles": N,
           "basin_hops": HOPS, "numpy": np.__version__, "host_cpus_visible": len(os.sched_getaffinity(0)), "runs": [],
           "kernels": bq.kernel_figures(lib_path, "struct")}
    for dtype in ("float64", "float32"):
        minima = bh.tempered_and_quenched(dzo, bq, N, REPLICAS, np.dtype(dtype))
        at_rest = dzo.quench_to_rest(minima, N)
        starts = start_replicas(N, WALKERS, 2.25, np.dtype(dtype))
        walkers = dzo.DeviceArray.from_host(starts.reshape(-1))
        hopping = dzo.BasinHopping(walkers, N, np.full(WALKERS, 1.0 / 0.8), np.full(WALKERS, 0.35), 2.25, 0.01, 10, 400, 1)
        hopping.hop(HOPS, adapt=False, hops_per_launch=8, wait=True)
        best = dzo.DeviceArray((WALKERS, 3 * N), np.dtype(dtype), ptr=hopping.ptr(dzo.BASIN_HOPPING_BEST_POINTS), owner=False).copy()
        hopping.close()
        best_at_rest = dzo.quench_to_rest(best, N)
        guidance = tol_guidance(dzo, dzo.DeviceArray.from_host(np.concatenate([minima.to_host().ravel(), best.to_host().ravel()])), dtype)
        # nothing to recommend: a tenth of the smallest distance between minima of different energy, which merges none of them
        # and splits copies of one minimum that are further apart than that
        tol = guidance["recommended_tol"] or guidance["smallest_distance_different_energy"] / 10.0
        row = {"dtype": dtype, "tol": tol, "tol_guidance": guidance, "minima_at_rest": int(at_rest.sum()), "best_points_at_rest": int(best_at_rest.sum())}
        print(json.dumps(row), flush=True)
        row["minima_256"], _, _, _ = identify(dzo, st, minima, tol, args.repeats)
        row["basin_hopping_best_4096"], _, _, best_e = identify(dzo, st, best, tol, args.repeats)
        row["basin_hopping_best_4096"]["lowest_energy"] = float(np.nanmin(best_e))
        zero_tol, grad_tol = SEARCH_TOLERANCES[dtype]
        saddles = minima.copy()
        search = dzo.find_saddles_hybrid(saddles, N, kick=0.05, grad_tol=grad_tol, max_steps=300, zero_tol=zero_tol)
        is_saddle = (search.status == dzo.HYBRIDEF_CONVERGED) & (search.eigenvalues.astype(np.float64) < -zero_tol)
        modes = dzo.DeviceArray((REPLICAS, 3 * N), np.dtype(dtype), ptr=search.ptr(dzo.HYBRIDEF_MODES), owner=False).copy()
        search.close()
        row["saddles_256"], labels, _, _ = identify(dzo, st, saddles, tol, args.repeats)
        row["saddles_256"]["saddles"] = int(is_saddle.sum())
        row["saddles_256"]["distinct_saddles"] = int(len(np.unique(labels[is_saddle & (labels >= 0)])))
        print(json.dumps(row), flush=True)
        row["displacement_sweep"] = sweep(dzo, saddles, modes, is_saddle, tol)
        res["runs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    print(readme_paragraph(res))


if __name__ == "__main__":
    main()
