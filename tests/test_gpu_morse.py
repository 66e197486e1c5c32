"""The Morse radials (DZO_RADIAL_MORSE_RHO6, DZO_RADIAL_MORSE_RHO14) through every unit that takes ``radial``, on the device,
against the high-precision twin of tests/morse_twin.py and its derived bound (the device's exp is not correctly rounded, so
nothing here is replayed bit for bit against numpy; device against device is).  Every comparison with the twin prints its
largest error / bound ratio and records it in profiles/morse_parity.json when the module has run.

The single-set sizes up to 257 run the WAVE shape of csrc/dzo_pairwise.hip (every N <= 2048 does) and are checked in every
entry; N_TILE = 2053 = 8 x 256 + 5 runs the TILE shape with a partial last tile and a split j range (9 row blocks are far
fewer than the CUs), with the energy summed over all rows by the twin and gradient and product checked on a subset of rows,
so that the longdouble sums stay cheap."""
import functools
import json
import os

import numpy as np
import pytest

import modefollow_twin as mft
import morse_method_twin as mm
import morse_twin as mt
import pairwise_twin as tw
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
RADIALS = {6: getattr(dzo, "RADIAL_MORSE_RHO6", 2), 14: getattr(dzo, "RADIAL_MORSE_RHO14", 3)}    # (without them: every test fails)
RHOS = [6, 14]
DTYPES = [np.float64, np.float32]
NS = [1, 2, 3, 38, 63, 64, 65, 257]
N_TILE = 2053
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    if RATIOS:
        path = os.path.join(ROOT, "profiles", "morse_parity.json")
        out = {"exp_ulps_assumed": mt.EXP_ULPS, "device": dzo.device_info().get("name", "?"),
               "largest_error_over_bound": {k: round(v, 6) for k, v in sorted(RATIOS.items())}}
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


# ------------------------------------------------------------------------------ helpers
def _name(dtype):
    return np.dtype(dtype).name


def _within(test, what, got, want, bound):
    """|got - want| <= bound entry by entry; the largest ratio is printed and recorded under the test's name."""
    got, want, bound = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(bound, dtype=LD)
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(np.max(ratio)) if ratio.size else 0.0
    RATIOS[test] = max(RATIOS.get(test, 0.0), worst)
    print(f"{test} {what}: worst error / bound = {worst:.4f}")
    assert np.all(err <= bound), (test, what, worst, np.argwhere(~(err <= bound))[:5].tolist())


@functools.lru_cache(maxsize=None)
def _config(n, dtype, seed=None):
    """x, y, z, u, v, w as fp64 arrays holding values of ``dtype``: the twin sees exactly what the device sees."""
    seed = n if seed is None else seed
    xyz = tw.lattice(n, seed) if seed != n else tw.cluster(n, seed=n)
    uvw = np.random.default_rng(1000 + seed).normal(size=(3, n))
    return tuple(np.asarray(a, dtype=dtype).astype(np.float64) for a in (*xyz, *uvw))


def _split(p):
    p = np.asarray(p, dtype=np.float64)
    n = len(p) // 3
    return p[:n], p[n:2 * n], p[2 * n:]


def _dev(arrays, dtype):
    n = len(arrays[0])
    buf = dzo.DeviceArray.from_host(np.concatenate(arrays), dtype=dtype)
    return buf, [buf.view(k * n, n) for k in range(len(arrays))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


@functools.lru_cache(maxsize=None)
def _ico_starts(dtype, count=4, seed=13):
    """Jittered icosahedra with vertices one pair distance from the centre, as values of ``dtype``: (count, 39)."""
    ico = np.concatenate(tw.icosahedron13()) / 1.08
    starts = np.tile(ico, (count, 1)) + np.random.default_rng(seed).uniform(-0.05, 0.05, size=(count, 39))
    return np.asarray(starts, dtype=dtype).astype(np.float64)


def _quench(points, n, radial, cls="lbfgs", launches=200):
    """Steps 50 at a time until all are stuck; returns (handle, energies after every launch, done).  A stuck L-BFGS instance
    need not be at rest: the reference's L-BFGS has no curvature safeguard, and after a pair with s.y < 0 its search can halve
    the step to nothing on a slope (dzo.quench_to_rest has the story).  So, as there, a FRESH BatchedLBFGS handle takes over
    when all are stuck, until one ends with the bits of the energies it began with; the trace runs through all the handles."""
    make = (lambda: dzo.BatchedLBFGS(points, n, 0.01, 10, radial=radial)) if cls == "lbfgs" else (lambda: dzo.BatchedAdGD(points, n, 0.01, radial=radial))
    opt = make()
    trace, done, began = [opt.current_objective_values.copy()], False, opt.current_objective_values.copy()
    for _ in range(launches):
        done = opt.step(50)
        trace.append(opt.current_objective_values.copy())
        if done and (cls != "lbfgs" or np.array_equal(_bits(trace[-1]), _bits(began))):
            break
        if done:
            opt.close()
            opt, done = make(), False
            began = opt.current_objective_values.copy()
            assert np.array_equal(_bits(began), _bits(trace[-1]))       # a handle begins where the last one ended
    return opt, np.array(trace), done


@functools.lru_cache(maxsize=None)
def _minima13(rho, dtype):
    """Four quenched 13-atom minima as a host array (4, 39) of ``dtype``."""
    pts = dzo.DeviceArray.from_host(_ico_starts(dtype).ravel(), dtype=dtype)
    assert dzo.quench_to_rest(pts, 13, radial=RADIALS[rho]).all()
    return pts.to_host().reshape(4, 39)


@functools.lru_cache(maxsize=None)
def _minimum65(rho, dtype):
    x, y, z = _config(65, dtype)[:3]
    pts = dzo.DeviceArray.from_host(np.concatenate([x, y, z]), dtype=dtype)
    assert dzo.quench_to_rest(pts, 65, max_steps=6000, radial=RADIALS[rho]).all()
    return pts.to_host().reshape(1, 195)


def _gradient_noise(points, n, rho, dtype):
    """rms over the entries of the derived bound of the device gradient at the points: what a device gradient norm cannot go below."""
    out = 0.0
    for p in np.atleast_2d(points):
        b = mt.bound("gradient", dtype, *_split(p), rho)
        out = max(out, float(np.sqrt((b * b).mean())))
    return out


# ------------------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_dimer_at_the_pair_minimum_is_exact(rho, dtype):
    """Two particles exactly 1 apart on the x axis: r = 1, a = 0, t = exp(0) = 1; energy fma(1, 1, -2) = -1, first 0,
    second rho^2 / 2, every operation exact."""
    radial = RADIALS[rho]
    zero2 = np.zeros(2)
    keep, (x, y, z, u, v, w) = _dev([np.array([0.0, 1.0]), zero2, zero2, np.array([1.0, 0.0]), zero2, zero2], dtype)
    assert dzo.pairwise_radial_energy(x, y, z, radial=radial) == -1.0
    g = dzo.DeviceArray.from_host(np.full(6, 7.0), dtype=dtype)
    dzo.pairwise_radial_gradient_(*(g.view(2 * k, 2) for k in range(3)), x, y, z, radial=radial)
    assert np.all(g.to_host() == 0)
    p = dzo.DeviceArray.zeros(6, dtype)
    dzo.pairwise_radial_hvp_(*(p.view(2 * k, 2) for k in range(3)), x, y, z, u, v, w, radial=radial)
    assert p.to_host().tolist() == [2.0 * rho * rho, -2.0 * rho * rho, 0, 0, 0, 0]
    pts = keep.view(0, 6)
    gb = dzo.DeviceArray.from_host(np.full(6, 7.0), dtype=dtype)
    e = dzo.pairwise_batch_energy_gradient(pts, 2, gb, radial=radial)
    assert e.tolist() == [-1.0] and np.all(gb.to_host() == 0)
    h = dzo.pairwise_batch_hessian(pts, 2, radial=radial)[0]
    assert h[0, 0] == 2.0 * rho * rho and h[1, 1] == 2.0 * rho * rho and h[0, 1] == -2.0 * rho * rho and h[1, 0] == -2.0 * rho * rho
    assert np.all(h[2:, :] == 0) and np.all(h[:, 2:] == 0)     # f = 0 at the minimum: no transverse stiffness


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_one_particle_has_no_energy(rho, dtype):
    radial = RADIALS[rho]
    keep, (x, y, z) = _dev([np.array([0.3]), np.array([-0.2]), np.array([1.5])], dtype)
    assert dzo.pairwise_radial_energy(x, y, z, radial=radial) == 0.0
    g = dzo.DeviceArray.from_host(np.full(3, 7.0), dtype=dtype)
    dzo.pairwise_radial_gradient_(*(g.view(k, 1) for k in range(3)), x, y, z, radial=radial)
    assert np.all(g.to_host() == 0)
    gb = dzo.DeviceArray.from_host(np.full(3, 7.0), dtype=dtype)
    assert dzo.pairwise_batch_energy_gradient(keep, 1, gb, radial=radial).tolist() == [0.0] and np.all(gb.to_host() == 0)
    assert dzo.pairwise_radial_energy_delta(x, y, z, 0, 1.0, 1.0, 1.0, radial=radial) == 0.0


# ------------------------------------------------------------------------------ 2. the single-set functions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n", NS)
def test_single_set_functions_within_the_bound(n, rho, dtype):
    radial, test = RADIALS[rho], f"single_set[{n}-{rho}-{_name(dtype)}]"
    cfg = _config(n, dtype)
    x, y, z, u, v, w = cfg
    keep, (dx, dy, dz, du, dv, dw) = _dev(cfg, dtype)
    e = dzo.pairwise_radial_energy(dx, dy, dz, radial=radial)
    _within(test, "energy", e, mt.energy(x, y, z, rho), mt.bound("energy", dtype, x, y, z, rho))
    g = dzo.DeviceArray.zeros(3 * n, dtype)
    dzo.pairwise_radial_gradient_(*(g.view(k * n, n) for k in range(3)), dx, dy, dz, radial=radial)
    _within(test, "gradient", g.to_host().reshape(3, n), mt.gradient(x, y, z, rho), mt.bound("gradient", dtype, x, y, z, rho))
    p = dzo.DeviceArray.zeros(3 * n, dtype)
    dzo.pairwise_radial_hvp_(*(p.view(k * n, n) for k in range(3)), dx, dy, dz, du, dv, dw, radial=radial)
    _within(test, "hvp", p.to_host().reshape(3, n), mt.hvp(x, y, z, u, v, w, rho), mt.bound("hvp", dtype, x, y, z, rho, u, v, w))
    for i in sorted({0, n // 2, n - 1}):
        new = tuple(float(np.asarray(c[i] + s, dtype=dtype)) for c, s in ((x, 0.1), (y, -0.05), (z, 0.07)))
        d = dzo.pairwise_radial_energy_delta(dx, dy, dz, i, *new, radial=radial)
        _within(test, f"delta i={i}", d, mt.energy_delta(x, y, z, i, *new, rho), mt.bound("delta", dtype, x, y, z, rho, i=i, new=new))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_single_set_functions_in_the_tile_shape(rho, dtype):
    """N > 2048: pairwise_tile_kernel in its three modes, the partial last tile, the split of the j range and
    pairwise_finish_rows_kernel.  Rows: the first and last of the first tile, the first of the second, the last full tile's
    last, the partial tile's, and 24 drawn ones."""
    n, radial, test = N_TILE, RADIALS[rho], f"tile_shape[{N_TILE}-{rho}-{_name(dtype)}]"
    cfg = _config(n, dtype)
    x, y, z, u, v, w = cfg
    rows = np.unique(np.concatenate([[0, 255, 256, 1791, 1792, 2047, 2048, n - 1], np.random.default_rng(n).integers(0, n, 24)]))
    keep, (dx, dy, dz, du, dv, dw) = _dev(cfg, dtype)
    e = dzo.pairwise_radial_energy(dx, dy, dz, radial=radial)
    be, want = mt.bound("energy", dtype, x, y, z, rho, with_value=True)
    _within(test, "energy", e, want, be)
    g = dzo.DeviceArray.zeros(3 * n, dtype)
    dzo.pairwise_radial_gradient_(*(g.view(k * n, n) for k in range(3)), dx, dy, dz, radial=radial)
    _within(test, "gradient", g.to_host().reshape(3, n)[:, rows], mt.gradient(x, y, z, rho, rows), mt.bound("gradient", dtype, x, y, z, rho, rows=rows))
    p = dzo.DeviceArray.zeros(3 * n, dtype)
    dzo.pairwise_radial_hvp_(*(p.view(k * n, n) for k in range(3)), dx, dy, dz, du, dv, dw, radial=radial)
    _within(test, "hvp", p.to_host().reshape(3, n)[:, rows], mt.hvp(x, y, z, u, v, w, rho, rows), mt.bound("hvp", dtype, x, y, z, rho, u, v, w, rows=rows))
    i = n - 1
    new = tuple(float(np.asarray(c[i] + s_, dtype=dtype)) for c, s_ in ((x, 0.1), (y, -0.05), (z, 0.07)))
    d = dzo.pairwise_radial_energy_delta(dx, dy, dz, i, *new, radial=radial)
    _within(test, f"delta i={i}", d, mt.energy_delta(x, y, z, i, *new, rho), mt.bound("delta", dtype, x, y, z, rho, i=i, new=new))


# ------------------------------------------------------------------------------ 3. the batched evaluation, products and Hessians
def _batch_points(n, dtype):
    cfgs = [_config(n, dtype, seed=n + 7000 * k) if k else _config(n, dtype) for k in range(3)]
    return cfgs, np.stack([np.concatenate(c[:3]) for c in cfgs]), np.stack([np.concatenate(c[3:]) for c in cfgs])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300])
def test_batched_evaluation_and_products_within_the_bound(n, rho, dtype):
    radial, test = RADIALS[rho], f"batched[{n}-{rho}-{_name(dtype)}]"
    cfgs, pts, dirs = _batch_points(n, dtype)
    P, D = dzo.DeviceArray.from_host(pts.ravel(), dtype=dtype), dzo.DeviceArray.from_host(dirs.ravel(), dtype=dtype)
    G = dzo.DeviceArray.zeros(pts.size, dtype)
    E = dzo.pairwise_batch_energy_gradient(P, n, G, radial=radial)
    G = G.to_host().reshape(3, 3 * n)
    prod, curv = dzo.pairwise_batch_hvp(P, D, n, curvatures=True, radial=radial)
    prod = prod.to_host().reshape(3, 3 * n)
    u64 = LD(2.0) ** -53
    for b, (x, y, z, u, v, w) in enumerate(cfgs):
        _within(test, f"energy[{b}]", E[b], mt.energy(x, y, z, rho), mt.bound("energy", dtype, x, y, z, rho))
        _within(test, f"gradient[{b}]", G[b].reshape(3, n), mt.gradient(x, y, z, rho), mt.bound("gradient", dtype, x, y, z, rho))
        want, bp = mt.hvp(x, y, z, u, v, w, rho), mt.bound("hvp", dtype, x, y, z, rho, u, v, w)
        _within(test, f"hvp[{b}]", prod[b].reshape(3, n), want, bp)
        d = np.stack([u, v, w]).astype(LD)
        # u.Hu from the device's own products, in fp64: the products' bound through |u|, and 3n fp64 roundings of the dot
        _within(test, f"u.Hu[{b}]", curv[b, 0], (d * want).sum(), (np.abs(d) * bp).sum() + (3 * n + 2) * u64 * np.abs(d * want).sum())
        _within(test, f"u.u[{b}]", curv[b, 1], (d * d).sum(), (3 * n + 2) * u64 * (d * d).sum())
        # the same instance alone: device against device, bit for bit
        one_p, one_d = dzo.DeviceArray.from_host(pts[b], dtype=dtype), dzo.DeviceArray.from_host(dirs[b], dtype=dtype)
        one_g = dzo.DeviceArray.zeros(3 * n, dtype)
        one_e = dzo.pairwise_batch_energy_gradient(one_p, n, one_g, radial=radial)
        one_prod, one_curv = dzo.pairwise_batch_hvp(one_p, one_d, n, curvatures=True, radial=radial)
        assert np.array_equal(_bits(one_e), _bits(E[b:b + 1])) and np.array_equal(_bits(one_g.to_host()), _bits(G[b]))
        assert np.array_equal(_bits(one_prod.to_host().ravel()), _bits(prod[b])) and np.array_equal(_bits(one_curv[0]), _bits(curv[b]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128])
def test_batched_hessians_within_the_bound(n, rho, dtype):
    radial, test = RADIALS[rho], f"hessian[{n}-{rho}-{_name(dtype)}]"
    cfgs, pts, _ = _batch_points(n, dtype)
    H = dzo.pairwise_batch_hessian(dzo.DeviceArray.from_host(pts.ravel(), dtype=dtype), n, radial=radial)
    for b, (x, y, z, _, _, _) in enumerate(cfgs):
        # the device layout is [column, row]; the twin's matrix and its bound are symmetric
        _within(test, f"[{b}]", H[b].T, mt.hessian(x, y, z, rho), mt.bound("hessian", dtype, x, y, z, rho))
        alone = dzo.pairwise_batch_hessian(dzo.DeviceArray.from_host(pts[b], dtype=dtype), n, radial=radial)[0]
        assert np.array_equal(_bits(alone), _bits(H[b]))


# ------------------------------------------------------------------------------ 4. the selector selects
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_radials_three_energies_and_a_handle_keeps_its_own(dtype):
    x, y, z = _config(38, dtype)[:3]
    pts = np.concatenate([x, y, z])
    P = dzo.DeviceArray.from_host(pts, dtype=dtype)
    e = [dzo.pairwise_batch_energy_gradient(P, 38, radial=r)[0] for r in (dzo.RADIAL_LENNARD_JONES, RADIALS[6], RADIALS[14])]
    assert len(set(float(v) for v in e)) == 3, e
    assert e[0] == dzo.pairwise_batch_energy_gradient(P, 38)[0]                        # the default is Lennard-Jones
    for k, rho in ((1, 6), (2, 14)):
        _within(f"selector[{_name(dtype)}]", f"rho={rho}", e[k], mt.energy(x, y, z, rho), mt.bound("energy", dtype, x, y, z, rho))
    # a Morse handle, then a Lennard-Jones handle created and stepped on the same stream, then the Morse handle steps:
    # the bits of a Morse handle that never saw the other one
    start = _ico_starts(dtype)
    for cls, args in ((dzo.BatchedLBFGS, (0.01, 10)), (dzo.BatchedAdGD, (0.01,))):
        a_pts, c_pts = (dzo.DeviceArray.from_host(start.ravel(), dtype=dtype) for _ in range(2))
        a = cls(a_pts, 13, *args, radial=RADIALS[6])
        lj = cls(dzo.DeviceArray.from_host(start.ravel() * 1.08, dtype=dtype), 13, *args, radial=dzo.RADIAL_LENNARD_JONES)
        lj.step(5)
        a.step(5)
        c = cls(c_pts, 13, *args, radial=RADIALS[6])
        c.step(5)
        assert np.array_equal(_bits(a.current_points), _bits(c.current_points))
        assert np.array_equal(_bits(a.current_objective_values), _bits(c.current_objective_values))
        for b, p in enumerate(a.current_points.astype(np.float64)):
            _within(f"selector[{_name(dtype)}]", f"{cls.__name__}[{b}]", a.current_objective_values[b], mt.energy(*_split(p), 6),
                    mt.bound("energy", dtype, *_split(p), 6))
        assert not np.array_equal(lj.current_objective_values, a.current_objective_values)


# ------------------------------------------------------------------------------ 5. quench
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("cls", ["lbfgs", "adgd"])
def test_quench_descends_to_the_icosahedron_and_to_rest(cls, rho, dtype):
    """A stuck instance is one whose search found no lower energy, and the search compares energies that carry an error of at
    most B each (the derived bound of the energy at the end point).  Both quenches end on a search along -g that halves its
    step until the energy falls or the step is nothing: AdGD always, and the L-BFGS quench because it ends with a fresh handle,
    whose first direction is the gradient's, changing nothing.  Along -g the energy falls by t g.g - t t g.Hg / 2, at most
    G = (g.g)^2 / (2 g.Hg) at t* = g.g / g.Hg; the halving search tries a step within a factor 2 of t* (its first trial,
    0.01 / |g| for the fresh L-BFGS handle, is far above t* for these gradients; AdGD's own step is near 1 / (2 L) along its
    path, t* / 2), where the fall is 3 G / 4 at least.  The device cannot miss a fall above 2 B, so at rest 3 G / 4 <= 2 B:
    "rounding level for T" is G <= 8 B / 3, with g and H the twin's at the end point.  The ratio G / (8 B / 3) is recorded with
    the parity figures.  The N = 13 energies are then within 3 B of the twin's icosahedron in either type (what is left to
    gain along the softest direction, and B of evaluation), and within a relative 1e-9 in fp64."""
    radial, test = RADIALS[rho], f"quench[{cls}-{rho}-{_name(dtype)}]"
    x65 = np.concatenate(_config(65, dtype)[:3])
    for n, start in ((13, _ico_starts(dtype)), (65, x65[None, :])):
        pts = dzo.DeviceArray.from_host(start.ravel(), dtype=dtype)
        opt, trace, done = _quench(pts, n, radial, cls, launches=400)
        assert done and opt.is_stuck.all(), (n, opt.iteration_counts)
        assert np.all(np.diff(trace.astype(np.float64), axis=0) <= 0), (n, trace)
        for b, p in enumerate(opt.current_points.astype(np.float64)):
            xyz = _split(p)
            B = mt.bound("energy", dtype, *xyz, rho)
            _within(test, f"N={n} energy[{b}]", opt.current_objective_values[b], mt.energy(*xyz, rho), B)
            g = mt.gradient(*xyz, rho).astype(np.float64).ravel()
            gHg = float(g @ mm.hessian(p, rho) @ g)
            assert gHg > 0, (n, b, gHg)
            gain = float(g @ g) ** 2 / (2 * gHg)
            RATIOS[test + " G / (8 B / 3)"] = max(RATIOS.get(test + " G / (8 B / 3)", 0.0), gain / float(8 * B / 3))
            print(f"{test} N={n}[{b}]: twin |g|_max = {np.abs(g).max():.3e}, G = {gain:.3e}, 8 B / 3 = {float(8 * B / 3):.3e}")
            assert gain <= 8 * B / 3, (n, b, gain, float(B))
            if n == 13:
                want = mt.relaxed_icosahedron(rho)[1]
                assert abs(float(opt.current_objective_values[b]) - want) <= 3 * B, (b, opt.current_objective_values[b], want, float(B))
        if n == 13 and dtype == np.float64:
            want = mt.relaxed_icosahedron(rho)[1]
            assert np.all(np.abs(opt.current_objective_values - want) <= 1e-9 * abs(want)), (opt.current_objective_values, want)


# ------------------------------------------------------------------------------ 6. tempering
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_tempering_energies_are_those_of_the_replicas(rho, dtype):
    radial, steps = RADIALS[rho], 300
    x65 = np.concatenate(_config(65, dtype)[:3])
    for n, start, beta, radius in ((13, _ico_starts(dtype), [8.0, 5.0, 3.0, 2.0], 3.0), (65, np.stack([x65, x65]), [8.0, 3.0], 9.0)):
        r = len(beta)
        rep = dzo.DeviceArray.from_host(start.ravel(), dtype=dtype)
        pt = dzo.ParallelTempering(rep, n, beta, [0.08] * r, radius, base_seed=5, radial=radial)
        trace = dzo.DeviceArray.zeros(steps * r, dtype)
        pt.temper(steps, trace)
        last = trace.to_host().reshape(r, steps)[:, -1]
        coords = pt.coordinates.astype(np.float64)
        assert np.all((coords ** 2).sum(axis=1) < radius * radius)
        acc, rej = pt.num_accept, pt.num_reject
        assert np.all(acc + rej == steps) and np.all(acc > 0) and np.all(acc < steps), (acc, rej)
        for k in range(r):
            xyz = coords[k]
            _within(f"tempering[{rho}-{_name(dtype)}]", f"N={n} replica {k}", last[k], mt.energy(*xyz, rho),
                    steps * mt.bound("energy", dtype, *xyz, rho))
        # the quench of the replicas runs under the handle's radial
        energies, minima, opt = pt.quench(max_steps=4000)
        assert opt.is_stuck.all()
        for k, p in enumerate(minima.to_host().reshape(r, 3 * n).astype(np.float64)):
            _within(f"tempering[{rho}-{_name(dtype)}]", f"N={n} quenched replica {k}", energies[k], mt.energy(*_split(p), rho),
                    mt.bound("energy", dtype, *_split(p), rho))


# ------------------------------------------------------------------------------ 7. basin hopping
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_basin_hopping_best_energies_are_those_of_the_best_points(rho, dtype):
    walkers = dzo.DeviceArray.from_host(_ico_starts(dtype, 8, 29).ravel(), dtype=dtype)
    bh = dzo.BasinHopping(walkers, 13, [2.0] * 8, [0.3] * 8, 3.0, base_seed=3, radial=RADIALS[rho])
    first = bh.energies.copy()
    bh.hop(4, adapt=True, hops_per_launch=4)
    best, points = bh.best_energies, bh.best_points.astype(np.float64)
    assert bh.hop_counts.tolist() == [4] * 8 and np.all(bh.num_accept + bh.num_reject == 4)
    assert np.all(best <= first), (best, first)
    for b in range(8):
        _within(f"basin_hopping[{rho}-{_name(dtype)}]", f"walker {b}", best[b], mt.energy(*_split(points[b]), rho),
                mt.bound("energy", dtype, *_split(points[b]), rho))
    cur = bh.current_points.astype(np.float64)
    for b in range(8):
        _within(f"basin_hopping[{rho}-{_name(dtype)}]", f"current {b}", bh.energies[b], mt.energy(*_split(cur[b]), rho),
                mt.bound("energy", dtype, *_split(cur[b]), rho))


# ------------------------------------------------------------------------------ 8. second order
def _spectrum_tolerance(p, rho, dtype):
    """|lambda_device - lambda_twin| <= |H_device - H_twin|_2 (Weyl) + the eigensolver's own error.  The first is at most the
    Frobenius norm of the Hessian bound; cyclic Jacobi is backward stable to (sweeps <= 30) x 3n roundings of |H|_2."""
    xyz = _split(p)
    lam = np.linalg.eigvalsh(mt.hessian(*xyz, rho).astype(np.float64))
    bh = mt.bound("hessian", dtype, *xyz, rho)
    return lam, float(np.sqrt((bh * bh).sum())), 30 * len(p) * float(mt.EPS[np.dtype(dtype)]) * max(abs(lam[0]), abs(lam[-1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_spectra_lowest_modes_and_polish_at_the_minima(rho, dtype):
    radial, test = RADIALS[rho], f"second_order[{rho}-{_name(dtype)}]"
    for n, minima in ((13, _minima13(rho, dtype)), (65, _minimum65(rho, dtype))):
        P = dzo.DeviceArray.from_host(minima.ravel(), dtype=dtype)
        spectrum = dzo.hessian_spectrum(P, n, radial=radial)
        res_tol = dzo.LOWMODE_DEFAULT_RES_TOL[np.dtype(dtype)]
        modes = dzo.lowest_modes(P, n, radial=radial)
        assert modes.status.tolist() == [dzo.LOWMODE_CONVERGED] * len(minima), (modes.status, modes.residuals)
        softest = np.inf
        for b, p in enumerate(minima.astype(np.float64)):
            lam, dh, solver = _spectrum_tolerance(p, rho, dtype)
            _within(test, f"N={n} spectrum[{b}]", spectrum[b], lam, dh + solver)
            # a Ritz value lies within its residual of an eigenvalue; the residual asked for is res_tol x the largest eigenvalue
            _within(test, f"N={n} lowest mode[{b}]", modes.eigenvalues[b], lam[6], dh + 2 * res_tol * lam[-1])
            assert np.abs(lam[:6]).max() <= dh + solver + 1e-3 * lam[6] and lam[6] > 0, lam[:8]
            softest = min(softest, lam[6])
        # zero_tol: a tenth of the softest vibration of the twin; grad_tol: what the device gradient can resolve, 1e-10 at least
        grad_tol = max(1e-10, 2 * _gradient_noise(minima.astype(np.float64), n, rho, dtype))
        polished = dzo.polish_minima(P, n, grad_tol=grad_tol, max_steps=30, zero_tol=0.1 * softest, radial=radial)
        assert polished.status.tolist() == [dzo.MODEFOLLOW_CONVERGED] * len(minima), (polished.status, polished.grms, grad_tol)
        assert polished.index.tolist() == [0] * len(minima) and polished.zeros.tolist() == [6] * len(minima), (polished.index, polished.zeros)
        for b, p in enumerate(polished.current_points.astype(np.float64)):
            g = mt.gradient(*_split(p), rho).astype(np.float64)
            assert np.sqrt((g * g).mean()) <= grad_tol + _gradient_noise(p, n, rho, dtype)
        polished.close()


# ------------------------------------------------------------------------------ 9. saddle searches
SADDLE_N, SADDLE_KICK, SADDLE_SEEDS = 7, 0.05, range(8)


@functools.lru_cache(maxsize=None)
def _minima7(rho, dtype):
    """Eight minima of 7 atoms: the starts of tests/modefollow_twin.random_start quenched to rest on the device, first under
    rho = 6 and from there under rho (a random start falls apart into fragments under the short-ranged rho = 14: minima with more
    than six zero modes, from which the twin of the method finds saddles for half of the starts only): (8, 21)."""
    starts = np.stack([mft.random_start(SADDLE_N, seed) for seed in SADDLE_SEEDS])
    pts = dzo.DeviceArray.from_host(np.asarray(starts, dtype=dtype).astype(np.float64).ravel(), dtype=dtype)
    for stage in sorted({6, rho}):
        assert dzo.quench_to_rest(pts, SADDLE_N, max_steps=6000, radial=RADIALS[stage]).all()
    return pts.to_host().reshape(8, 3 * SADDLE_N)


def _saddle_tolerances(minima, rho, dtype):
    """(zero_tol, grad_tol, gradient noise).  zero_tol: the interface's 1e-4 in fp64; in fp32 the zero modes of a 21 x 21 Hessian
    with eigenvalues up to 2000 come out within some 21 eps 2000 = 5e-3 of zero, and 0.05 leaves a factor ten (the softest
    saddle curvature the twin meets from these starts is -0.22).  grad_tol: four times what the device gradient resolves."""
    noise = _gradient_noise(minima.astype(np.float64), SADDLE_N, rho, dtype)
    return (1e-4 if dtype == np.float64 else 0.05), max(1e-10, 4 * noise), noise


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_find_saddles_ends_on_saddles_the_twin_confirms(rho, dtype):
    """Kick, seeds and N are chosen with tests/morse_method_twin.follow, which in fp64 ends on an index-1 saddle from 8 of
    these 8 minima for rho = 6 and for rho = 14 (in 8 to 30 steps); at least half of the device's searches must."""
    minima = _minima7(rho, dtype)
    zero_tol, grad_tol, noise = _saddle_tolerances(minima, rho, dtype)
    P = dzo.DeviceArray.from_host(minima.ravel(), dtype=dtype)
    saddles, polished = dzo.find_saddles(P, SADDLE_N, kick=SADDLE_KICK, grad_tol=grad_tol, max_steps=300, zero_tol=zero_tol, radial=RADIALS[rho])
    status, index, points = saddles.status, saddles.index, saddles.current_points.astype(np.float64)
    done = np.flatnonzero(status == dzo.MODEFOLLOW_CONVERGED)
    print(f"find_saddles rho={rho} {_name(dtype)}: status {status.tolist()}, index {index.tolist()}, steps {saddles.iteration_counts.tolist()}")
    assert len(done) >= 4, status
    for b in done:
        g = mt.gradient(*_split(points[b]), rho).astype(np.float64)
        assert np.sqrt((g * g).mean()) <= grad_tol + noise, (b, np.sqrt((g * g).mean()))
        lam = np.linalg.eigvalsh(mm.hessian(points[b], rho))
        assert int((lam < -zero_tol).sum()) == index[b] and int((np.abs(lam) <= zero_tol).sum()) == saddles.zeros[b], (b, lam[:9], index[b])
        _within(f"find_saddles[{rho}-{_name(dtype)}]", f"energy[{b}]", saddles.energies[b], mt.energy(*_split(points[b]), rho),
                mt.bound("energy", dtype, *_split(points[b]), rho))
    saddles.close(); polished.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_find_saddles_hybrid_ends_on_saddles_the_twin_confirms(rho, dtype):
    """As above with tests/morse_method_twin.hybrid (the exact lowest mode in place of the Lanczos refinement): 8 of 8 for both
    ranges, in 7 to 14 steps."""
    minima = _minima7(rho, dtype)
    zero_tol, grad_tol, noise = _saddle_tolerances(minima, rho, dtype)
    P = dzo.DeviceArray.from_host(minima.ravel(), dtype=dtype)
    search = dzo.find_saddles_hybrid(P, SADDLE_N, kick=SADDLE_KICK, grad_tol=grad_tol, max_steps=300, zero_tol=zero_tol, radial=RADIALS[rho])
    status, lam_dev, points = search.status, search.eigenvalues.astype(np.float64), search.current_points.astype(np.float64)
    done = np.flatnonzero(status == dzo.HYBRIDEF_CONVERGED)
    print(f"find_saddles_hybrid rho={rho} {_name(dtype)}: status {status.tolist()}, eigenvalues {lam_dev.round(4).tolist()}, "
          f"steps {search.iteration_counts.tolist()}")
    assert len(done) >= 4, status
    for b in done:
        g = mt.gradient(*_split(points[b]), rho).astype(np.float64)
        assert np.sqrt((g * g).mean()) <= grad_tol + noise, (b, np.sqrt((g * g).mean()))
        lam, _ = mm.lowest_vibration(points[b], rho)
        # the reported index: the sign of the lowest vibration (negative: a saddle), and its value to the mode's tolerance
        assert (lam_dev[b] < -zero_tol) == (lam < -zero_tol), (b, lam_dev[b], lam)
        top = np.linalg.eigvalsh(mm.hessian(points[b], rho))[-1]
        assert abs(lam_dev[b] - lam) <= 1e-3 * top + zero_tol, (b, lam_dev[b], lam)
        _within(f"find_saddles_hybrid[{rho}-{_name(dtype)}]", f"energy[{b}]", search.energies[b], mt.energy(*_split(points[b]), rho),
                mt.bound("energy", dtype, *_split(points[b]), rho))
    search.close()


# ------------------------------------------------------------------------------ 10. structures and bands
def _rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_fingerprints_sum_to_the_energy_and_know_a_moved_copy(rho, dtype):
    radial, test = RADIALS[rho], f"structure[{rho}-{_name(dtype)}]"
    eps = float(mt.EPS[np.dtype(dtype)])
    for n, base in ((13, _minima13(rho, dtype)[0]), (65, np.concatenate(_config(65, dtype)[:3]))):
        c = base.astype(np.float64).reshape(3, n)
        moved = (_rotation(n) @ c)[:, np.random.default_rng(n).permutation(n)] + np.array([[0.25], [-0.5], [0.125]])
        other = c * 1.02
        pts = np.asarray(np.stack([c.ravel(), moved.ravel(), other.ravel()]), dtype=dtype).astype(np.float64)
        fp, e = dzo.structure_fingerprints(dzo.DeviceArray.from_host(pts.ravel(), dtype=dtype), n, radial=radial)
        f = fp.to_host().reshape(3, 2 * n).astype(np.float64)
        assert np.array_equal(_bits(e), _bits(dzo.pairwise_batch_energy_gradient(dzo.DeviceArray.from_host(pts.ravel(), dtype=dtype), n, radial=radial)))
        for b in range(3):
            xyz = _split(pts[b])
            rows = np.sort(mt.row_energies(*xyz, rho))
            brow = mt.bound("rows", dtype, *xyz, rho)
            # a per-particle energy is e_i = sum_{j != i} e(r2_ij) (include/dzo.h), sorted: each within the largest row bound
            # of the twin's; their sum is twice the energy
            _within(test, f"N={n} per-particle[{b}]", f[b, :n], rows, brow.max())
            _within(test, f"N={n} sum[{b}]", 0.5 * f[b, :n].astype(LD).sum(), mt.energy(*xyz, rho),
                    0.5 * (brow.sum() + n * LD(2.0) ** -53 * np.abs(rows).sum()))
        # the moved copy: its coordinates are rounded to T after the motion (eps |x| each, so 2 sqrt(3) eps R per distance and
        # |dE/dr| = 2 rho t |t - 1| <= rho / 2 per pair), on top of twice the rows' bound
        xyz = _split(pts[0])
        R = float(np.abs(pts[:2]).max())
        S = np.abs(mt._pairs(*xyz, rho)[5]).sum(axis=1).max()
        slack = 2 * float(mt.bound("rows", dtype, *xyz, rho).max()) + n * rho * 2 * np.sqrt(3.0) * eps * R
        tol = 2 * slack / max(1.0, float(S)) + 16 * eps
        labels, reps = dzo.classify_structures(fp, tol)
        print(f"{test} N={n}: tol {tol:.3e}, labels {labels.tolist()}")
        assert labels[1] == labels[0] and labels[2] != labels[0], (labels, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rho", RHOS)
def test_elastic_band_between_a_minimum_and_its_neighbour(rho, dtype):
    """A saddle of 7 atoms from find_saddles, its two minima from connect_saddles, a band of 5 images between them, 50
    iterations: no band FAILED, and the image energies are the twin's energies of the images."""
    radial = RADIALS[rho]
    minima = _minima7(rho, dtype)
    zero_tol, grad_tol, noise = _saddle_tolerances(minima, rho, dtype)
    P = dzo.DeviceArray.from_host(minima.ravel(), dtype=dtype)
    saddles, polished = dzo.find_saddles(P, SADDLE_N, kick=SADDLE_KICK, grad_tol=grad_tol, max_steps=300, zero_tol=zero_tol, radial=radial)
    ok = np.flatnonzero((saddles.status == dzo.MODEFOLLOW_CONVERGED) & (saddles.index == 1))
    assert len(ok) >= 1, (saddles.status, saddles.index)
    k, n3 = int(ok[0]), 3 * SADDLE_N
    point = dzo.DeviceArray.from_host(saddles.current_points[k], dtype=dtype)
    mode = dzo.DeviceArray.from_host(saddles.follow[k], dtype=dtype)
    tol = 1e-5 if dtype == np.float64 else 1e-2
    paths = dzo.connect_saddles(point, mode, SADDLE_N, 0.03, tol, radial=radial)
    assert paths.end_stuck.all(), paths.end_stuck
    a, b = paths.ends.view(0, (1, n3)), paths.ends.view(n3, (1, n3))
    band = dzo.interpolate_band(a, b, SADDLE_N, 5)
    neb = dzo.ElasticBand(band, SADDLE_N, 5, force_tol=1e-6 if dtype == np.float64 else 1e-5, radial=radial)
    neb.step(50)
    assert neb.status[0] != dzo.NEB_FAILED, neb.status
    # an iteration evaluates the images and then moves them: the energies of the band as it stands after 50 iterations are
    # those the next iteration reports (a band that has converged is not moved any more and reports the energies it has)
    images = neb.images[0].astype(np.float64)
    neb.step(1)
    assert neb.status[0] != dzo.NEB_FAILED, neb.status
    energies = neb.energies[0]
    for m in range(5):
        _within(f"band[{rho}-{_name(dtype)}]", f"image {m}", energies[m], mt.energy(*_split(images[m]), rho),
                mt.bound("energy", dtype, *_split(images[m]), rho))
    se = paths.saddle_energies[0]
    _within(f"band[{rho}-{_name(dtype)}]", "saddle", se, mt.energy(*_split(saddles.current_points[k].astype(np.float64)), rho),
            mt.bound("energy", dtype, *_split(saddles.current_points[k].astype(np.float64)), rho))
    assert se >= max(energies[0], energies[-1]) - 2 * float(mt.bound("energy", dtype, *_split(images[0]), rho))
    neb.close(); saddles.close(); polished.close()
