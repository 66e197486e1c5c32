"""Measurement of the connect cycle (`dzo.connect_pathways`, `dzo.band_candidates`, csrc/dzo_pathway.hip): recorded, not gated.

    python tools/bench_pathways.py [--out profiles/pathways_bench.json] [--sizes 38,200] [--cycles 4,4] [--repeats 5]
    python tools/bench_pathways.py --readme profiles/pathways_bench.json   # no device: rewrite the README paragraph from a result

The pairs of tools/bench_align.py: distinct structure k with k + 1 of tempered and quenched replicas, in fp64, 256 pairs at N = 38
and 64 pairs at N = 200.  Per size:

* one `dzo.connect_pathways` call (9 images, 600 band iterations, the structure block's `tol` and `displacement`): how many pairs
  are connected after each cycle, the size of the database, and each cycle's time by phase;
* `dzo.band_candidates` on the bands of the first cycle's kind (the pairs aligned, interpolated, iterated 600 times) against the
  path there was before: download the band and its energies, then numpy (the same rule, vectorised over the bands);
* at N = 38, the figure of the `align-readme` block again in the same session: `dzo.connect_minima(align=True)`.

And the two small systems of tests/test_gpu_pathway.py, whose counts the tests print and do not assert: LJ13 (eight pairs among
the five lowest minima, four cycles) and LJ7 in float32 (six pairs, three cycles)."""
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

MARKERS = ("<!-- pathways-readme -->", "<!-- /pathways-readme -->")
IMAGES, BAND_ITERATIONS, DISPLACEMENT = 9, 600, 0.03         # displacement: the structure block of README.md


def host_candidates(band_dev, energies_dev, n, m):
    """(seconds, count, points, tangents): the path there was before.  Download, then the rule in numpy over all bands at once."""
    t0 = time.perf_counter()
    e = energies_dev.to_host()
    x = band_dev.to_host().reshape(len(e), m, 3 * n)
    mask = (e[:, 1:-1] > e[:, :-2]) & (e[:, 1:-1] >= e[:, 2:])
    b, i = np.nonzero(mask)
    i = i + 1
    dp, dm = x[b, i + 1] - x[b, i], x[b, i] - x[b, i - 1]
    ar, al = np.abs(e[b, i + 1] - e[b, i]), np.abs(e[b, i - 1] - e[b, i])
    hi, lo = np.maximum(ar, al), np.minimum(ar, al)
    up = (e[b, i + 1] > e[b, i - 1])[:, None]
    t = np.where(up, hi[:, None] * dp + lo[:, None] * dm, lo[:, None] * dp + hi[:, None] * dm)
    t /= np.sqrt((t * t).sum(axis=1, keepdims=True))
    points = x[b, i].copy()
    return time.perf_counter() - t0, len(b), points, t


def candidate_timing(dzo, a, b, n, repeats):
    aligned = dzo.align_pairs(a, b, n).aligned
    band = dzo.interpolate_band(a, aligned, n, IMAGES)
    neb = dzo.ElasticBand(band, n, IMAGES, force_tol=0.0)
    neb.run(BAND_ITERATIONS, 200)
    neb.close()
    energies = dzo.DeviceArray.from_host(dzo.pairwise_batch_energy_gradient(band, n).reshape(-1, IMAGES))
    dzo.band_candidates(band, n, IMAGES, energies=energies)  # warm-up
    walls = []
    for _ in range(repeats):
        dzo.synchronize()
        t0 = time.perf_counter()
        cand = dzo.band_candidates(band, n, IMAGES, energies=energies)
        walls.append(time.perf_counter() - t0)
    dzo.profile_reset()
    dzo.band_candidates(band, n, IMAGES, energies=energies)
    events = dzo.profile_table().get("pathway_candidates", (0, 0.0))[1]
    host_candidates(band, energies, n, IMAGES)               # warm-up
    host = [host_candidates(band, energies, n, IMAGES) for _ in range(repeats)]
    seconds, (_, count, points, tangents) = float(np.median([h[0] for h in host])), host[-1]
    worst = float(np.abs(cand.tangents.to_host() - tangents).max()) if count == cand.count and count else None
    return {"bands": int(band.shape[0]), "candidates": cand.count, "device_ms_host_clock_median": 1e3 * float(np.median(walls)),
            "device_ms_events": float(events), "host_ms_median": 1e3 * seconds, "host_count": count,
            "ratio_host_over_device": seconds / float(np.median(walls)), "same_points": bool(count == cand.count and np.array_equal(points, cand.points.to_host())),
            "largest_tangent_difference": worst}


def cycle_rows(res):
    return [{k: (v if k != "seconds" else {p: round(s, 4) for p, s in v.items()}) for k, v in c.items()} for c in res.cycles]


def small_systems(dzo):
    import pathway_cases as pc
    out = {}
    minima = pc.lj13_minima(dzo)
    first, second = zip(*pc.LJ13_PAIRS)
    b = pc.moved(minima[list(second)], np.random.default_rng(13))
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(minima[list(first)]), dzo.DeviceArray.from_host(b), 13, IMAGES, tol=1e-5, displacement=0.02,
                               band_iterations=BAND_ITERATIONS, max_cycles=4, quench_options=dict(max_steps=4000))
    out["lj13_float64"] = {"pairs": len(res.connected), "connected": int(res.connected.sum()), "cycles": cycle_rows(res)}
    minima = pc.lj7_minima(dzo)
    first, second = zip(*[(i, j) for i in range(4) for j in range(i + 1, 4)])
    for dtype, options in (("float64", dict(tol=1e-5)), ("float32", dict(tol=1e-3, grad_tol=3e-5, zero_tol=1e-3))):
        a = minima[list(first)].astype(dtype)
        b = pc.moved(minima[list(second)], np.random.default_rng(77)).astype(dtype)
        res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(b), 7, IMAGES, displacement=0.02, band_iterations=BAND_ITERATIONS,
                                   max_cycles=3, align=dict(random_trials=25), quench_options=dict(max_steps=4000), **options)
        out["lj7_" + dtype] = {"pairs": len(res.connected), "connected": int(res.connected.sum()), "cycles": cycle_rows(res),
                               "saddle_energies": [round(float(e), 6) for e in res.saddle_energies]}
    return out


def readme_paragraph(res):
    out = ["Measured %s on top of commit %s (`profiles/pathways_bench.json`): the pairs of the `align-readme` block (distinct structure k with "
           "k + 1), one `dzo.connect_pathways` call in float64 with %d images, %d band iterations per cycle, `tol = %g`, `displacement = %g`, "
           "`max_attempts = 2`." % (res["date"], res["parent_commit"], IMAGES, BAND_ITERATIONS, res["tol"], DISPLACEMENT)]
    for r in res["runs"]:
        cyc = r["cycles"]
        out.append("**N = %d**, %d pairs, %d cycles allowed (the index of a saddle %s): connected after each cycle %s of %d; database %s minima "
                   "and %s saddles; bands / candidates / saddles kept per cycle %s; seconds per cycle %s (distances / search / align / band / "
                   "candidates / refine / connect: %s); the whole call %.1f s."
                   % (r["n_particles"], r["pairs"], r["max_cycles"], "checked by `hessian_spectrum`" if r["index_checked"] else "NOT checked",
                      " / ".join(str(c["connected"]) for c in cyc), r["pairs"], " / ".join(str(c["minima"]) for c in cyc),
                      " / ".join(str(c["saddles"]) for c in cyc), "; ".join("%d / %d / %d" % (c["bands"], c["candidates"], c["new_saddles"]) for c in cyc),
                      " / ".join("%.1f" % sum(c["seconds"].values()) for c in cyc),
                      "; ".join(" / ".join("%.2f" % c["seconds"].get(p, 0.0) for p in ("distances", "search", "align", "band", "candidates", "refine", "connect")) for c in cyc),
                      r["wall_seconds"]))
        t = r["candidate_timing"]
        out.append("`dzo.band_candidates` on %d such bands (%d candidates): %.3f ms by the host clock (median of %d; %.3f ms by device events for "
                   "the three launches), download + numpy %.2f ms (median of as many), ratio %.1f, the same candidates: %s."
                   % (t["bands"], t["candidates"], t["device_ms_host_clock_median"], res["repeats"], t["device_ms_events"], t["host_ms_median"],
                      t["ratio_host_over_device"], t["same_points"]))
        if "connect_minima_align_true" in r:
            c = r["connect_minima_align_true"]
            out.append("`dzo.connect_minima(align=True)` on the same pairs in the same session (`force_tol = 1e-06`, at most 6000 iterations): %d bands "
                       "CONVERGED, %d FAILED, %d still ACTIVE, so it names %d saddles." % (c["converged"], c["failed"], c["active"], c["refined_saddles"]))
    s = res.get("small_systems")
    if s:
        out.append("The small systems of tests/test_gpu_pathway.py: LJ13, %d of %d pairs connected after %d cycles (per cycle %s); LJ7 float64 %d of "
                   "%d; LJ7 float32 (`grad_tol = 3e-5`, `zero_tol = 1e-3`, `tol = 1e-3`) %d of %d."
                   % (s["lj13_float64"]["connected"], s["lj13_float64"]["pairs"], len(s["lj13_float64"]["cycles"]),
                      " / ".join(str(c["connected"]) for c in s["lj13_float64"]["cycles"]), s["lj7_float64"]["connected"], s["lj7_float64"]["pairs"],
                      s["lj7_float32"]["connected"], s["lj7_float32"]["pairs"]))
    out.append("Not measured: float32 at these sizes (the structure block says why its minima are not identified reliably), other image counts, band "
               "lengths, `max_attempts` and alignment options, the cycle without the gradient descent of the ends (`descent_steps = 0`; every "
               "figure here has the default of 2000), cycles beyond the ones allowed here, how many of the connections are the lowest "
               "ones the landscape has, and how the host side of a cycle (the graph search, numpy gathers, uploads) divides. Out of scope: "
               "several atom species, a disconnectivity graph, rate constants.")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathways_bench.json"))
    ap.add_argument("--sizes", default="38,200")
    ap.add_argument("--cycles", default="4,4", help="max_cycles per size")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the commit this tree sits on, where the tree carries no git metadata")
    ap.add_argument("--readme", default=None, metavar="JSON", help="rewrite the README paragraph from this result and exit (no device)")
    args = ap.parse_args()
    if args.readme:
        write_readme(json.load(open(args.readme)))
        return
    import bench_align as ba
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
           "images": IMAGES, "band_iterations": BAND_ITERATIONS, "tol": ba.STRUCTURE_TOL, "displacement": DISPLACEMENT, "repeats": args.repeats,
           "runs": [], "kernels": bq.kernel_figures(lib_path, "pathcand_")}
    sizes = [int(s) for s in args.sizes.split(",") if s]
    limits = dict(zip(sizes, [int(s) for s in args.cycles.split(",")]))
    for n, pairs, replicas in ba.CASES:
        if n not in sizes:
            continue
        minima, distinct = ba.distinct_minima(dzo, bq, bh, n, pairs + 1, replicas)
        pairs = len(minima) - 1
        a, b = dzo.DeviceArray.from_host(minima[:-1]), dzo.DeviceArray.from_host(minima[1:])
        t0 = time.perf_counter()
        r = dzo.connect_pathways(a, b, n, IMAGES, tol=ba.STRUCTURE_TOL, displacement=DISPLACEMENT, band_iterations=BAND_ITERATIONS,
                                 max_cycles=limits[n])
        wall = time.perf_counter() - t0
        row = {"n_particles": n, "dtype": "float64", "pairs": pairs, "distinct_minima": distinct, "max_cycles": limits[n],
               "index_checked": 3 * n <= dzo.SYMEIG_MAX_N, "wall_seconds": wall, "connected": int(r.connected.sum()), "cycles": cycle_rows(r),
               "minima": r.graph.n_minima, "saddles": r.graph.n_saddles,
               "path_lengths": np.bincount([len(p) // 2 for p in r.paths if p is not None]).tolist(),
               "median_barrier": float(np.nanmedian(r.barriers)) if r.connected.any() else None}
        print(json.dumps(row), flush=True)
        row["candidate_timing"] = candidate_timing(dzo, a, b, n, args.repeats)
        print(json.dumps(row["candidate_timing"]), flush=True)
        if n == 38:
            row["connect_minima_align_true"] = ba.band_counts(dzo, a, b, n, "float64", True)
            print(json.dumps(row["connect_minima_align_true"]), flush=True)
        res["runs"].append(row)
    res["small_systems"] = small_systems(dzo)
    print(json.dumps(res["small_systems"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    print(readme_paragraph(res))


if __name__ == "__main__":
    main()
