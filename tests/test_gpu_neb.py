"""The batched nudged elastic band on the device (csrc/dzo_neb.hip) against its CPU twin (tests/neb_twin.py).

1. ONE iteration from a band and velocities the test supplies (``dzo_neb_batch_apply``), at N = 3, 4, 64 and 65 (the wave/block
   seam), 256 and 257 (one or two particles per thread) and 1024 (the maximum, device-memory storage in fp64; batch 1 and three
   images there, so that the longdouble twin stays quick), with 3 images (one interior image), 4, 6 (the second turn of the first
   two waves) and, at N = 4, 32; batch 3, both element types.  The images are jittered lattice clusters, the configurations take
   the climbing and the plain force, zero and random velocities, and a move cap below and above the move:

   * E and g equal ``dzo_pairwise_batch_energy_gradient`` with ``==``;
   * status, climbing image and highest image equal the twin's; the inputs are checked (on the twin's values) to sit more than
     1e-6 relative away from what could flip a branch: the energies the tangent and the highest image are chosen from, v.F at 0
     (as a cosine), |s| at max_move, the residual at force_tol;
   * the new band, the velocities, the forces and the tangents against the twin run in fp64 on the same inputs.  The tolerance
     is not fixed in advance: per shape it is 4 x the largest difference, over the configurations and bands of the shape,
     between the twin run in T and the twin run in the next wider format on the same inputs (fp32 against fp64; fp64 against
     numpy.longdouble), the factor 4 for the differing summation orders: the method of tests/test_gpu_hybridef.py;
   * band 1 alone gives the bits it gives inside the batch;
   * a converged band and a NaN band do not move and leave their neighbours' bits alone;
   * a separate test asserts on the twin that the shapes together take all four tangent branches, both forces, p > 0 and p <= 0,
     and moves below and above the cap.

2. The handle: (a) k iterations in one call or in k calls, and the interpolation against the twin with ``==``; (b) LJ7, five
   images, three bands against the twin and an independently found saddle; (c) LJ13, nine images, four bands; (d) fp32; (e)
   N = 130, the block shape end to end; (f) error codes and every ``what``; (g) the plain-C example.

MEASURED on an MI355X (the largest allowed and the largest seen over the 20 shapes; the test prints them per shape with ``-s``):
   fp64: band 4.1e-15 allowed, velocities 1.7e-13, forces 6.2e-12, tangents 9.5e-14; seen 0 in all four at every shape: the
   device has the bits of the fp64 twin, whose energies and gradients carry the device's fused pair terms and order of sums.
   fp32: band 2.0e-06 allowed, 5.0e-07 seen; velocities 3.7e-05, 9.1e-06; forces 1.1e-03, 2.6e-04 (forces of some 5 sqrt(3N));
   tangents 3.8e-05, 9.4e-06.  At every shape the seen value is a quarter of the allowed one: the device has the bits of the
   fp32 twin there too, and what is seen is the twin's own distance from its fp64 run.
   The handle: the LJ7 bands converge in 879, 520 and 618 iterations, the twin in the same; climbing images with a true gradient
   rms of 1e-14, a lowest mode of -10.0 to -9.9, and the energy of the independently found saddle to 1.8e-15 (1.1e-12 allowed).
   LJ13: 3513, 3199, 4654 and 3893 iterations, energies to 1.4e-14 of the saddles' (2.1e-12 to 3.7e-12 allowed).  fp32 at
   force_tol 1e-5 converges on all three LJ7 bands.  N = 130: residual 1.80 at iteration 0, 0.076 after 200.
"""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import modefollow_twin as mt
import neb_twin as nb
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ZERO_TOL = 1e-4
# (N, images)
SHAPES = [(3, 3), (3, 4), (3, 6), (4, 3), (4, 4), (4, 6), (4, 32), (64, 3), (64, 4), (64, 6), (65, 3), (65, 4), (65, 6), (256, 3), (256, 4),
          (256, 6), (257, 3), (257, 4), (257, 6), (1024, 3)]
# (climb, scale of the random velocities, max_move, spring).  Lattice clusters feel forces of some 5 sqrt(3N): from rest a move
# is dt^2 |F| ~ 2e-3 sqrt(3N), which 10 is above; with velocities of scale 1 it is dt |v| ~ 0.02 sqrt(3N), which 1e-3 is below.
CONFIGS = [(True, 0.0, 10.0, 1.0), (False, 1.0, 1e-3, 1.0), (True, 1.0, 10.0, 5.0)]
# LJ13: the first four of the seeds of tests/test_hybridef_twin.py on whose end pair the CPU twin converges within 6000 iterations
# (it does on 4, 5, 11, 12, 16 and 18 of the sixteen, in 1878 to 4704; on the others the path passes a third minimum or is still
# creeping at 6000, and one band fails when two images meet)
LJ7_SEEDS, LJ13_SEEDS = (1, 2, 3), (4, 5, 11, 12)
# added to the lattice seeds of a particle count: with the plain seeds two neighbouring images of 257 particles have energies
# 9e-8 apart (relative), too close for the tangent branch to be the same in every format
SEED_SHIFT = {257: 500}
SEEN = {}


def _batch(n):
    return 1 if n == 1024 else 3


def _configs(n):
    return CONFIGS[:2] if n == 1024 else CONFIGS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _inputs(n, m, dtype):
    """Bands (batch, m, 3n) of jittered lattice clusters (one jitter per image: neighbours differ by up to 0.1 per coordinate)
    and the velocities of unit scale, rounded to ``dtype``."""
    dt = np.dtype(dtype)
    bands = np.stack([np.stack([np.concatenate(tw.lattice(n, seed=1000 * n + 40 * b + i + SEED_SHIFT.get(n, 0))) for i in range(m)]) for b in range(_batch(n))])
    vel = np.random.default_rng(7 * n + m).normal(size=bands.shape)
    vel[:, 0] = vel[:, -1] = 0.0
    out = bands.astype(dt), vel.astype(dt)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _twin_runs(n, m, dtype):
    """The twin on every configuration and band of a shape, computed once: {(config, b): the fp64 run}, and the shape's
    tolerances, 4 x the largest difference between the twin run in T and in the next wider format, per compared array."""
    dt = np.dtype(dtype)
    wider = np.float64 if dt == np.float32 else np.longdouble
    bands, vel = _inputs(n, m, dtype)
    refs, diff = {}, dict(band=0.0, velocities=0.0, F=0.0, tau=0.0)
    for c, (climb, vscale, max_move, spring) in enumerate(_configs(n)):
        for b in range(_batch(n)):
            args = dict(spring=spring, max_move=max_move, force_tol=0.0, climb=climb)
            v = (vel[b].astype(np.float64) * vscale).astype(dt)
            in_t, in_wide = nb.iterate(bands[b], v, dtype=dt, **args), nb.iterate(bands[b], v, dtype=wider, **args)
            refs[c, b] = in_t if dt == np.float64 else in_wide
            assert in_t["status"] == in_wide["status"] == nb.ACTIVE
            assert in_t["climbing"] == in_wide["climbing"] and in_t["highest"] == in_wide["highest"] and in_t["hit"] == in_wide["hit"]
            for key in diff:
                diff[key] = max(diff[key], float(np.abs(in_t[key].astype(wider) - in_wide[key]).max()))
    return refs, {key: 4.0 * d for key, d in diff.items()}


def _check_margins(twin):
    for name, value, threshold in twin["branches"]:
        scale = max(abs(value), abs(threshold)) if threshold != 0 else max(abs(value), 1.0 if name == "p" else 0.0)
        assert abs(value - threshold) > 1e-6 * scale, (name, value, threshold)


def _apply(bands, vel, dtype, config, force_tol=0.0):
    """The device call on host arrays (batch, m, 3n).  Returns the record dict with ``band`` and ``velocities`` (moved) and
    ``before`` (the DeviceArray of the band as given) added."""
    dt = np.dtype(dtype)
    batch, m, n3 = bands.shape
    climb, vscale, max_move, spring = config
    bdev = dzo.DeviceArray.from_host(np.ascontiguousarray(bands, dtype=dt))
    before = bdev.copy()
    vdev = dzo.DeviceArray.from_host(np.ascontiguousarray((np.asarray(vel, dtype=np.float64) * vscale).astype(dt)))
    r = dzo.neb_apply(bdev, vdev, n3 // 3, m, spring=spring, dt=0.02, max_move=max_move, force_tol=force_tol, climb=climb)
    r.update(band=bdev.to_host().reshape(batch, m, n3), velocities=vdev.to_host().reshape(batch, m, n3), before=before)
    return r


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_one_iteration_from_a_supplied_band(n, m, dtype):
    dt = np.dtype(dtype)
    batch = _batch(n)
    bands, vel = _inputs(n, m, dtype)
    refs, tol = _twin_runs(n, m, dtype)
    seen = dict.fromkeys(tol, 0.0)
    for c, config in enumerate(_configs(n)):
        r = _apply(bands, vel, dt, config)
        # E and g: the bits of the evaluation entry point, every image as an instance of its own
        gdev = dzo.DeviceArray((batch * m, 3 * n), dt)
        e = dzo.pairwise_batch_energy_gradient(r["before"], n, gdev)
        assert _same_bits(r["energies"].reshape(-1), e.reshape(-1)) and _same_bits(r["gradients"].reshape(batch * m, 3 * n), gdev.to_host())
        for b in range(batch):
            twin = refs[c, b]
            _check_margins(twin)
            assert r["status"][b] == twin["status"] == nb.ACTIVE
            assert r["climbing_images"][b] == twin["climbing"] and r["highest_images"][b] == twin["highest"], (c, b)
            for key, got in (("band", r["band"]), ("velocities", r["velocities"]), ("F", r["forces"]), ("tau", r["tangents"])):
                d = float(np.abs(got[b].astype(np.float64) - twin[key].astype(np.float64)).max())
                seen[key] = max(seen[key], d)
                assert d <= tol[key], (key, c, b, d, tol[key])
            assert np.all(r["forces"][b][[0, -1]] == 0) and np.all(r["force_rms"][b][[0, -1]] == 0)
            assert np.allclose(r["force_rms"][b], twin["frms"], rtol=1e-5) and np.isclose(r["residuals"][b], twin["residual"], rtol=1e-5)
            assert _same_bits(r["band"][b][[0, -1]], bands[b][[0, -1]])
        if batch > 1:                                        # band 1 alone
            alone = _apply(bands[1:2], vel[1:2], dt, config)
            for key in ("band", "velocities", "forces", "tangents", "energies", "gradients", "force_rms", "residuals"):
                assert _same_bits(alone[key][0], r[key][1]), (key, c)
    SEEN[n, m, dtype] = (tol, seen)
    print("N", n, "M", m, dtype, "allowed", {k: "%.2e" % v for k, v in tol.items()}, "seen", {k: "%.2e" % v for k, v in seen.items()})


def test_the_shapes_take_every_branch():
    """On the twin: all four tangent branches, both forces, both signs of v.F, moves below and above the cap."""
    hit = set()
    for n, m in SHAPES:
        if n <= 65:
            for twin in _twin_runs(n, m, "float64")[0].values():
                hit |= twin["hit"]
    assert hit == {"tangent0", "tangent1", "tangent2", "tangent3", "climbing", "plain", "p>0", "p<=0", "capped", "uncapped"}, hit


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [4, 65])
def test_converged_and_nan_bands_do_not_move_and_do_not_disturb(n, dtype):
    """Band 0 is a lattice band, band 1 a dilute one (spacing 3: forces of some 1e-3, below force_tol = 0.05), band 2 has a NaN."""
    dt = np.dtype(dtype)
    m, config = 4, CONFIGS[2]
    bands, vel = (a.copy() for a in _inputs(n, m, dtype))
    bands[1] = np.stack([np.concatenate(tw.lattice(n, seed=5 + i, spacing=3.0)) for i in range(m)]).astype(dt)
    bands[2, 1, 0] = np.nan
    r = _apply(bands, vel, dt, config, force_tol=0.05)
    assert r["status"].tolist() == [nb.ACTIVE, nb.CONVERGED, nb.FAILED], (r["status"], r["residuals"])
    vgiven = (vel.astype(np.float64) * config[1]).astype(dt)
    for b in (1, 2):
        assert _same_bits(r["band"][b], bands[b]) and _same_bits(r["velocities"][b], vgiven[b])
    assert r["residuals"][1] <= 0.05 < r["residuals"][0]
    alone = _apply(bands[0:1], vel[0:1], dt, config, force_tol=0.05)
    for key in ("band", "velocities", "forces", "tangents", "energies", "force_rms", "residuals"):
        assert _same_bits(alone[key][0], r[key][0]), key
    assert not _same_bits(r["band"][0], bands[0])


# ------------------------------------------------------------------------------ the handle
def _ends(n, seeds, dtype=np.float64):
    a, b, saddles, minima = nb.end_pairs(n, seeds)
    return (dzo.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype)), dzo.DeviceArray.from_host(np.ascontiguousarray(b, dtype=dtype)), saddles,
            minima)


def test_seven_iterations_in_one_call_or_in_seven_and_the_interpolation():
    n, m = 7, 5
    a, b, _, _ = _ends(n, LJ7_SEEDS)
    straight = dzo.interpolate_band(a, b, n, m).to_host()
    ah, bh = a.to_host(), b.to_host()
    for k in range(3):
        assert _same_bits(straight[k], nb.interpolate(ah[k], bh[k], m, np.float64)), k
        assert _same_bits(straight[k][0], ah[k]) and _same_bits(straight[k][-1], bh[k])
    results = []
    for calls in ((7,), (1,) * 7):
        band = dzo.DeviceArray.from_host(straight)
        neb = dzo.ElasticBand(band, n, m, force_tol=1e-6, climb_after=3)
        for k in calls:
            neb.step(k)
        results.append([neb.read(w) for w in range(11)])
        neb.close()
    assert results[0][dzo.NEB_ITERATION_COUNTS].tolist() == [7] * 3 and results[0][dzo.NEB_CLIMBING_IMAGES].min() >= 1
    assert not _same_bits(results[0][dzo.NEB_BAND], straight)
    for what, (x, y) in enumerate(zip(*results)):
        assert _same_bits(x, y), what


@functools.lru_cache(maxsize=None)
def _lj7_twin(dtype, force_tol):
    a, b, _, _ = nb.end_pairs(7, LJ7_SEEDS)
    return [nb.run(nb.interpolate(a[k], b[k], 5, dtype), force_tol=force_tol, max_iterations=2000, dtype=dtype) for k in range(3)]


def _independent_saddles(minima, n):
    """The saddles ``find_saddles_hybrid`` reaches from the minima at grad_tol = 1e-10: (points, energies, spectra)."""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(minima, dtype=np.float64))
    search = dzo.find_saddles_hybrid(dev, n, kick=0.05, grad_tol=1e-10, max_steps=300, zero_tol=ZERO_TOL)
    assert search.status.tolist() == [dzo.HYBRIDEF_CONVERGED] * len(minima) and np.all(search.eigenvalues < -ZERO_TOL)
    search.close()
    return dev.to_host(), dzo.pairwise_batch_energy_gradient(dev, n), dzo.hessian_spectrum(dev, n)


def _energy_rounding(point):
    """The rounding term of an fp64 energy, measured as in 1: 4 x the difference between the energy twin in fp64 and in
    longdouble at the point."""
    return 4.0 * abs(float(np.longdouble(nb.energy_gradient(point, np.float64)[0]) - nb.energy_gradient(point, np.longdouble)[0]))


def _check_climbing_images(neb, n, m, force_tol, saddle_points, saddle_energies, spectra):
    """Stationarity, the sign of the lowest mode and the energy of every band's climbing image.  The energy bound is the
    second-order one, E - E* <= 1/2 |g|^2 / min|lam_nonzero| with |g|^2 = 3N force_tol^2, plus one rounding term for each of
    the two device energies compared: E at the climbing image and E* at the saddle."""
    batch = neb.batch
    images, climbing, energies = neb.images, neb.climbing_images, neb.energies
    tops = np.stack([images[b, climbing[b]] for b in range(batch)])
    low = dzo.lowest_modes(dzo.DeviceArray.from_host(tops), n)
    for b in range(batch):
        g = tw.gradient_f64(tops[b])
        grms = np.sqrt((g * g).sum() / (3 * n))
        nonzero = np.abs(spectra[b])[np.abs(spectra[b]) > ZERO_TOL]
        bound = 0.5 * 3 * n * force_tol ** 2 / nonzero.min() + _energy_rounding(tops[b]) + _energy_rounding(saddle_points[b])
        print("band", b, "image", climbing[b], "grms", grms, "lowest mode", low.eigenvalues[b], "E - E*", energies[b, climbing[b]] - saddle_energies[b],
              "bound", bound)
        assert grms <= force_tol and low.eigenvalues[b] < -ZERO_TOL
        assert abs(energies[b, climbing[b]] - saddle_energies[b]) <= bound, (b, energies[b, climbing[b]], saddle_energies[b], bound)


def test_lj7_bands_end_on_the_saddle_that_joins_their_ends():
    n, m, force_tol = 7, 5, 1e-6
    a, b, _, minima = _ends(n, LJ7_SEEDS)
    twin = _lj7_twin(np.float64, force_tol)
    assert [t["status"] for t in twin] == [nb.CONVERGED] * 3
    neb = dzo.ElasticBand(dzo.interpolate_band(a, b, n, m), n, m, force_tol=force_tol)
    neb.run(2000)
    print("iterations", neb.iteration_counts.tolist(), "twin", [t["iterations"] for t in twin], "residuals", neb.residuals.tolist())
    assert neb.status.tolist() == [t["status"] for t in twin] and neb.climbing_images.tolist() == [t["climbing"] for t in twin]
    assert neb.iteration_counts.max() <= 2000 and np.all(neb.residuals <= force_tol)
    saddle_points, saddle_energies, spectra = _independent_saddles(minima, n)
    _check_climbing_images(neb, n, m, force_tol, saddle_points, saddle_energies, spectra)
    neb.close()


def test_lj13_bands_of_nine_images():
    n, m, force_tol = 13, 9, 1e-6
    a, b, _, minima = _ends(n, LJ13_SEEDS)
    neb = dzo.ElasticBand(dzo.interpolate_band(a, b, n, m), n, m, force_tol=force_tol)
    neb.run(6000, 500)
    print("iterations", neb.iteration_counts.tolist(), "residuals", neb.residuals.tolist(), "climbing", neb.climbing_images.tolist())
    assert neb.status.tolist() == [nb.CONVERGED] * 4 and neb.iteration_counts.max() <= 6000
    saddle_points, saddle_energies, spectra = _independent_saddles(minima, n)
    _check_climbing_images(neb, n, m, force_tol, saddle_points, saddle_energies, spectra)
    neb.close()


def test_fp32_bands_converge_at_the_tolerance_the_fp32_twin_reaches():
    """``neb_twin.FP32_FORCE_TOL`` is the first of 1e-5, 3e-5, 1e-4, ... at which the float32 twin converges on all three LJ7
    bands within 2000 iterations (tests/test_neb_twin.py finds it)."""
    n, m = 7, 5
    a, b, _, _ = _ends(n, LJ7_SEEDS, np.float32)
    neb = dzo.ElasticBand(dzo.interpolate_band(a, b, n, m), n, m, force_tol=nb.FP32_FORCE_TOL)
    neb.run(2000)
    print("iterations", neb.iteration_counts.tolist(), "residuals", neb.residuals.tolist())
    assert neb.energies.dtype == np.float32 and neb.status.tolist() == [nb.CONVERGED] * 3 and np.all(neb.residuals <= nb.FP32_FORCE_TOL)
    neb.close()


def test_block_shape_end_to_end_on_130_atoms():
    """One band between the two ends of a saddle of 130 atoms: not FAILED after 200 iterations, the residual lower than at
    iteration 0."""
    n, m = 130, 5
    dev = dzo.DeviceArray.from_host(np.concatenate(tw.lattice(n, seed=40))[None])
    dzo.quench_to_rest(dev, n)
    search = dzo.find_saddles_hybrid(dev, n, kick=0.05, grad_tol=1e-10, max_steps=400, zero_tol=ZERO_TOL)
    assert search.status.tolist() == [dzo.HYBRIDEF_CONVERGED]
    modes = dzo.DeviceArray((1, 3 * n), np.float64, ptr=search.ptr(dzo.HYBRIDEF_MODES), owner=False)
    paths = dzo.connect_saddles(dev, modes, n, 0.03, 1e-4)
    search.close()
    assert dzo.neb_plan(n, m, np.float64)[0] == dzo.NEB_SHAPE_BLOCK
    ends = paths.ends
    neb = dzo.ElasticBand(dzo.interpolate_band(ends.view(0, (1, 3 * n)), ends.view(3 * n, (1, 3 * n)), n, m), n, m, force_tol=1e-6)
    neb.step(1)
    first = neb.residuals[0]
    neb.step(200)
    print("residual", first, "->", neb.residuals[0], "status", neb.status.tolist(), "energies", neb.energies.tolist())
    assert neb.status[0] != nb.FAILED and neb.residuals[0] < first and np.isfinite(neb.energies).all()
    neb.close()


def test_connect_minima_returns_saddles_and_barriers():
    n, m = 7, 5
    a, b, saddles, _ = _ends(n, LJ7_SEEDS)
    c = dzo.connect_minima(a, b, n, m, force_tol=1e-6)
    e_saddle = np.array([mt.energy_gradient(s, np.float64)[0] for s in saddles])
    assert c.converged.tolist() == [0, 1, 2] and c.saddle_status.tolist() == [dzo.HYBRIDEF_CONVERGED] * 3 and np.all(c.saddle_eigenvalues < -ZERO_TOL)
    assert np.allclose(c.saddle_energies, e_saddle, atol=1e-9) and np.all(c.barriers > 0)
    assert np.allclose(c.barriers, c.saddle_energies[:, None] - c.energies[:, [0, -1]])


def test_error_codes_and_every_what():
    L = dzo.lib()
    n, m, batch = 5, 4, 2
    host = np.stack([np.stack([np.concatenate(tw.lattice(n, seed=10 * k + i)) for i in range(m)]) for k in range(batch)])
    band = dzo.DeviceArray.from_host(host)
    vel = dzo.DeviceArray.zeros(host.shape)
    h = ctypes.c_void_p()

    def create(radial=0, n_=n, m_=m, batch_=batch, dtype=dzo.F64, p=band.ptr, spring=1.0, dt=0.02, max_move=0.1, tol=1e-6, climb=1, after=50, out=None):
        return L.dzo_neb_batch_create(radial, n_, m_, batch_, dtype, p, spring, dt, max_move, tol, climb, after, ctypes.byref(h) if out is None else out)

    assert create(radial=7) == 1 and create(dtype=9) == 1 and create(n_=0) == 1 and create(batch_=0) == 1 and create(p=None) == 1
    assert create(m_=2) == 1 and b"n_images" in L.dzo_last_error() and create(m_=33) == 1
    assert create(spring=0.0) == 1 and create(dt=0.0) == 1 and create(max_move=-1.0) == 1 and create(tol=-1e-9) == 1 and create(after=-1) == 1
    assert L.dzo_neb_batch_create(0, n, m, batch, dzo.F64, band.ptr, 1.0, 0.02, 0.1, 1e-6, 1, 50, None) == 1
    assert create(n_=1025) == 5 and b"1024" in L.dzo_last_error()
    assert create(p=host.ctypes.data) == 3
    assert create() == 0 and h.value
    assert L.dzo_neb_batch_step(h, -1, None) == 1 and L.dzo_neb_batch_step(None, 1, None) == 1
    assert L.dzo_neb_batch_count_active(h, None) == 1 and L.dzo_neb_batch_read(h, 0, None) == 1
    out = np.zeros(host.size)
    assert L.dzo_neb_batch_read(h, 11, out.ctypes.data) == 1 and L.dzo_neb_batch_read(h, -1, out.ctypes.data) == 1
    p = ctypes.c_void_p()
    assert L.dzo_neb_batch_get_ptr(h, 11, ctypes.byref(p)) == 1 and L.dzo_neb_batch_get_ptr(h, 0, None) == 1
    climbing = np.zeros(batch, dtype=np.int32)
    assert L.dzo_neb_batch_read(h, dzo.NEB_CLIMBING_IMAGES, climbing.ctypes.data) == 0 and climbing.tolist() == [-1] * batch
    assert L.dzo_neb_batch_step(h, 0, None) == 0 and L.dzo_neb_batch_step(h, 2, None) == 0
    for what in range(11):
        assert L.dzo_neb_batch_read(h, what, out.ctypes.data) == 0, what
        assert L.dzo_neb_batch_get_ptr(h, what, ctypes.byref(p)) == 0 and p.value, what
    assert L.dzo_neb_batch_get_ptr(h, dzo.NEB_BAND, ctypes.byref(p)) == 0 and p.value == band.ptr                   # aliased: the caller's
    active = ctypes.c_int64(-1)
    assert L.dzo_neb_batch_count_active(h, ctypes.byref(active)) == 0 and active.value == batch
    assert L.dzo_neb_batch_destroy(h) == 0 and L.dzo_neb_batch_destroy(None) == 0

    a = dzo.DeviceArray.from_host(host[:, 0].copy())
    assert L.dzo_neb_batch_interpolate(n, 2, batch, dzo.F64, a.ptr, a.ptr, band.ptr) == 1 and L.dzo_neb_batch_interpolate(n, m, batch, 9, a.ptr, a.ptr, band.ptr) == 1
    assert L.dzo_neb_batch_interpolate(n, m, batch, dzo.F64, None, a.ptr, band.ptr) == 1 and L.dzo_neb_batch_interpolate(1025, m, batch, dzo.F64, a.ptr, a.ptr, band.ptr) == 5
    assert L.dzo_neb_batch_interpolate(n, m, batch, dzo.F64, host.ctypes.data, a.ptr, band.ptr) == 3
    band.upload(host)

    st = dzo.DeviceArray.from_host(np.zeros(batch, dtype=np.int32))

    def apply(radial=0, n_=n, m_=m, batch_=batch, dtype=dzo.F64, p=band.ptr, v=vel.ptr, spring=1.0, dt=0.02, max_move=0.1, tol=0.0, status=st.ptr):
        return L.dzo_neb_batch_apply(radial, n_, m_, batch_, dtype, p, v, spring, dt, max_move, tol, 1, None, None, None, None, None, None, None, None, status)

    assert apply(radial=7) == 1 and apply(dtype=9) == 1 and apply(n_=0) == 1 and apply(m_=2) == 1 and apply(batch_=0) == 1
    assert apply(p=None) == 1 and apply(v=None) == 1 and apply(status=None) == 1
    assert apply(spring=0.0) == 1 and apply(dt=-1.0) == 1 and apply(max_move=0.0) == 1 and apply(tol=-1.0) == 1 and apply(n_=1025) == 5
    assert apply(p=host.ctypes.data) == 3 and apply(v=host.ctypes.data) == 3 and apply(status=host.ctypes.data) == 3
    assert apply(tol=1e9) == 0 and st.to_host().tolist() == [nb.CONVERGED] * batch and _same_bits(band.to_host(), host)
    assert apply() == 0 and st.to_host().tolist() == [nb.ACTIVE] * batch and not _same_bits(band.to_host(), host)
    with pytest.raises(TypeError):
        dzo.ElasticBand(band, n, m)                          # force_tol has no default


def test_lj_band_example_prints_ok(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_band")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout and "barrier" in r.stdout, r.stderr
