"""What the device tests of the connect cycle (tests/test_gpu_pathway.py) and tools/bench_pathways.py share: the small
Lennard-Jones workloads (the four minima of LJ7, low minima of LJ13), random rigid motions and relabellings, and the checks
of a reported pathway that do not go through the library: the Lennard-Jones energy and gradient in numpy, fp64, and a steepest
descent on them.  A helper module like the *_twin.py files (no fixtures; imported by name)."""
import numpy as np

LJ7_MINIMA = (-16.505384, -15.935043, -15.593211, -15.533060)        # Tsai & Jordan 1993
LJ7_SADDLES = (-15.44473, -15.31986, -15.28342)                      # the three the float64 CPU restatement of the cycle found
LJ13_ICOSAHEDRON = -44.326801
LJ13_PAIRS = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 3), (3, 4))   # among the five lowest minima; ends are shared


# ------------------------------------------------------------------------------ Lennard-Jones in numpy, many points at once
def energy_gradient(points):
    """(E (K,), g (K, 3N)) of the points (K, 3N), [x | y | z] each, in fp64: E = sum_{i<j} 4 (r^-12 - r^-6)."""
    p = np.asarray(points, dtype=np.float64)
    k, n3 = p.shape
    x = p.reshape(k, 3, n3 // 3)
    d = x[:, :, :, None] - x[:, :, None, :]
    r2 = (d * d).sum(axis=1) + np.eye(n3 // 3)[None]
    inv6 = 1.0 / (r2 * r2 * r2)
    off = 1.0 - np.eye(n3 // 3)[None]
    e = 0.5 * (4.0 * (inv6 * inv6 - inv6) * off).sum(axis=(1, 2))
    w = -24.0 * (2.0 * inv6 * inv6 - inv6) / r2 * off
    return e, (w[:, None, :, :] * d).sum(axis=3).reshape(k, n3)


def steepest_descent(points, grad_tol=1e-5, max_iterations=60000):
    """Every point of (K, 3N) down its own gradient until max |g| <= grad_tol: x <- x - s g with a step of its own per point,
    grown by 1.25 after a step that lowered the energy and halved (the step not taken) after one that did not, so the energy
    of every point falls monotonically and the point stays in the basin it started in as far as a first-order method can
    tell.  Returns (points, energies, largest |g| component per point)."""
    x = np.array(points, dtype=np.float64)
    e, g = energy_gradient(x)
    s = np.full(len(x), 1e-3)
    for _ in range(max_iterations):
        if np.abs(g).max() <= grad_tol:
            break
        trial = x - s[:, None] * g
        et, gt = energy_gradient(trial)
        ok = et < e
        x[ok], e[ok], g[ok] = trial[ok], et[ok], gt[ok]
        s = np.where(ok, 1.25 * s, 0.5 * s)
    return x, e, np.abs(g).max(axis=1)


# ------------------------------------------------------------------------------ inputs
def moved(points, rng):
    """Every point of (K, 3N) rotated, translated and relabelled at random: the same structures in other frames."""
    p = np.asarray(points)
    k, n3 = p.shape
    out = np.empty_like(p)
    for i in range(k):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        xyz = p[i].reshape(3, n3 // 3).T.astype(np.float64)
        xyz = xyz[rng.permutation(n3 // 3)] @ q.T + rng.uniform(-2.0, 2.0, size=3)
        out[i] = xyz.T.reshape(n3).astype(p.dtype)
    return out


def quenched(dzo, starts, n):
    """The starts (K, 3n) quenched to rest on the device in fp64: (points, energies, at rest)."""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(starts, dtype=np.float64))
    rest = dzo.quench_to_rest(dev, n, max_steps=4000)
    return dev.to_host().reshape(len(starts), 3 * n), dzo.pairwise_batch_energy_gradient(dev, n), rest


def lj7_minima(dzo, seed=7, starts=256):
    """The four minima of LJ7 as a (4, 21) fp64 array, in the order of LJ7_MINIMA: random starts quenched on the device, the
    first one at rest within 1e-5 of each energy."""
    rng = np.random.default_rng(seed)
    points, energies, rest = quenched(dzo, rng.normal(size=(starts, 21)) * 0.55, 7)
    rows = []
    for target in LJ7_MINIMA:
        hit = np.flatnonzero(rest & (np.abs(energies - target) <= 1e-5))
        assert len(hit), (target, np.unique(np.round(energies[rest], 4)))
        rows.append(points[hit[0]])
    return np.stack(rows)


def lj13_minima(dzo, count=5, replicas=64, seed=13):
    """The `count` lowest distinct minima of LJ13 among tempered and quenched replicas, the icosahedron first: (count, 39)."""
    n, radius = 13, 2.25 * (13 / 38.0) ** (1.0 / 3.0)
    rng = np.random.default_rng(seed)
    starts = np.empty((replicas, 3, n))
    for k in range(replicas):                                # standard-normal points redrawn until they lie inside the sphere
        for i in range(n):
            while True:
                p = rng.standard_normal(3) * radius / 2.25
                if (p * p).sum() < radius * radius:
                    starts[k, :, i] = p
                    break
    dev = dzo.DeviceArray.from_host(starts.reshape(-1))
    beta = np.exp(np.linspace(-np.log(0.05), -np.log(0.35), replicas))
    pt = dzo.ParallelTempering(dev, n, beta, np.full(replicas, 0.05), radius, 1)
    pt.run(500, 20)
    dzo.synchronize()
    pt.close()
    rest = dzo.quench_to_rest(dev, n, max_steps=4000)
    _, reps, _, energies = dzo.unique_structures(dev, n, 1e-5)
    points = dev.to_host().reshape(replicas, 3 * n)
    energy_of = {int(r): float(e) for r, e in zip(reps, energies)}
    keep = sorted((r for r in energy_of if rest[r] and np.isfinite(energy_of[r])), key=energy_of.get)
    assert len(keep) >= count, (len(keep), count)
    rows = points[keep[:count]]
    lowest = energy_gradient(rows[:1])[0][0]
    assert abs(lowest - LJ13_ICOSAHEDRON) <= 1e-5, lowest
    return rows


# ------------------------------------------------------------------------------ the checks of a result
def check_pathways(dzo, res, n, displacement, zero_tol, known_saddles=None):
    """Every path ``res`` (a ``PathwayConnections``) reports is a chain of transition states: per saddle on a path, index 1 and
    six zero modes by ``hessian_spectrum`` at ``zero_tol``; stationary by the numpy gradient; where ``known_saddles`` is
    given, its energy within 1e-4 of one of them, or else verified here as another saddle (the same two checks, which do not
    depend on the list); and a numpy steepest descent from saddle +- displacement * mode lands within 1e-5 of the numpy energies
    of its two neighbours on the path.  The barrier of a connected pair is the highest saddle on its path minus the energy of
    its first end.  Returns the number of distinct saddles checked."""
    paths = [p for p in res.paths if p is not None and len(p) > 1]
    on_paths = sorted({s for p in paths for s in p[1::2]})
    for k, p in enumerate(res.paths):
        assert (p is not None) == bool(res.connected[k])
        if p is None:
            assert np.isnan(res.barriers[k])
            continue
        assert p[0] == res.pairs[k][0] and p[-1] == res.pairs[k][1] and len(p) % 2 == 1
        for i, s, j in zip(p[0::2], p[1::2], p[2::2]):
            assert (i, s, j) in res.graph.edges or (j, s, i) in res.graph.edges, (i, s, j)
        top = max([res.saddle_energies[s] for s in p[1::2]], default=res.minimum_energies[p[0]])
        assert res.barriers[k] == top - res.minimum_energies[p[0]], (k, res.barriers[k])
    if not on_paths:
        return 0
    saddles = res.saddles.to_host().reshape(-1, 3 * n)[on_paths]
    modes = res.saddle_modes.to_host().reshape(-1, 3 * n)[on_paths].astype(np.float64)
    dtype = saddles.dtype
    spectrum = dzo.hessian_spectrum(dzo.DeviceArray.from_host(saddles), n)
    negatives, zeros = dzo.morse_index(spectrum, zero_tol)
    assert negatives.tolist() == [1] * len(on_paths) and zeros.tolist() == [6] * len(on_paths), (negatives, zeros, spectrum[:, :8])
    e_np, g_np = energy_gradient(saddles)
    # what the refinement's tolerance leaves (1e-10 in fp64, 3e-5 in fp32), with room for the rounding of the coordinates to T
    assert np.abs(g_np).max() <= (1e-8 if dtype == np.float64 else 1e-3), np.abs(g_np).max()
    pairs_count = n * (n - 1) // 2
    e_round = 1e-9 if dtype == np.float64 else 16 * pairs_count * float(np.finfo(np.float32).eps)   # a few ulps per pair term
    assert np.abs(e_np - res.saddle_energies[on_paths]).max() <= e_round
    minima_np = energy_gradient(res.minima.to_host().reshape(-1, 3 * n))[0]
    assert np.abs(minima_np - res.minimum_energies).max() <= e_round
    if known_saddles is not None:
        for e in e_np:
            if np.abs(e - np.array(known_saddles)).min() > 1e-4:
                print("another saddle of the system, verified above as index 1 and stationary: %.6f" % e)
    ends = np.concatenate([saddles.astype(np.float64) + displacement * modes, saddles.astype(np.float64) - displacement * modes])
    _, landed, g_left = steepest_descent(ends)
    assert g_left.max() <= 1e-5, g_left.max()
    k = len(on_paths)
    row = {s: i for i, s in enumerate(on_paths)}
    for p in paths:
        for i, s, j in zip(p[0::2], p[1::2], p[2::2]):
            want = sorted([minima_np[i], minima_np[j]])
            got = sorted([landed[row[s]], landed[k + row[s]]])
            assert np.abs(np.array(got) - np.array(want)).max() <= 1e-5, (s, got, want)
    return k
