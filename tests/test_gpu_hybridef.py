"""Batched hybrid eigenvector following on the device (csrc/dzo_hybridef.hip) against its CPU twin (tests/hybridef_twin.py).

1. ONE step from a mode the test supplies (``dzo_hybridef_batch_apply``; u and lam are the lowest eigenpair of the projected
   dense fp64 Hessian of ``lowmode_twin.dense_truth``, so nothing here depends on the device's Lanczos iteration), at N = 3
   (3N - 6 = 3, the fewest), 4, 64 and 65 (the wave/block seam), 256 and 257 (one or two particles per thread) and 1024 (the
   maximum; batch 2 and at most one tangent step there, so that the longdouble twin stays quick), batch 3, both element types,
   0, 1 and 3 tangent steps through either count, max_step below and above the uphill step, tangent_cap below and above the
   tangent step:

   * E and g equal ``dzo_pairwise_batch_energy_gradient`` with ``==``;
   * status and tangent steps equal the twin's exactly; the inputs are checked (on the twin's values) to sit more than 1e-6
     relative away from what could flip a branch: a at zero_tol, |h| at max_step, s.y at 0 (as a cosine), dn at the cap,
     sqrt(pp / n) and grms at grad_tol;
   * the new point and F against the twin run in fp64 on the same inputs.  The tolerance is not fixed in advance: it is
     4 x the largest difference, over the configurations and instances of a shape, between the twin run in T and the twin run
     in the next wider format on the same inputs (fp32 against fp64; fp64 against numpy.longdouble), the factor 4 for the
     differing summation orders: the method of tests/test_gpu_modefollow.py.  Measured on an MI355X: see MEASURED below;
   * instance 1 alone gives the bits it gives inside the batch;
   * a converged instance and a NaN instance do not move and leave their neighbours' bits alone.

2. The handle: (a) transition states from the 16 asymmetric LJ13 minima, (b) N = 38 through ``find_saddles_hybrid``, (c) N = 130,
   above the ceiling of the dense search, (d) batching of the steps, (e) fp32, (f) error codes and every ``what``, (g) the
   plain-C example.

MEASURED on an MI355X (the largest allowed and the largest seen over the shapes; the test prints them per shape and instance):
   fp64: point 9.9e-15 allowed (N = 3), 1.8e-15 seen (N = 1024, where 6.8e-15 is allowed); F 1.0e-14 allowed, 3.6e-15 seen.
   fp32: point 8.2e-06 allowed (N = 3), 2.1e-06 seen; F 4.6e-06 allowed, 2.3e-06 seen (both at N = 1024).
   The tightest shape is N = 64 in fp64: 2.6e-15 allowed for the point, 4.4e-16 seen.
   The handle: 16 of 16 LJ13 searches end on index-1 saddles in 11 to 83 steps (the twin: 16, in 11 to 87); 8 of 8 at N = 38 in
   52 to 131 steps; both at N = 130, in 141 and 45 steps, with index 1 by the host spectrum.
"""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import hessian_twin as ht
import hybridef_twin as hy
import lowmode_twin as lt
import modefollow_twin as mt
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ZERO_TOL = 1e-4
SHAPES = [3, 4, 64, 65, 256, 257, 1024]
# (tangent_steps, tangent_steps_convex, sign given to lam, max_step, tangent_cap, tangent_first).  At these lattice points
# |h| is some 0.01 to 0.5: 1e-3 is below and 10 above it.  The first tangent step is tangent_first |p| with |p| ~ 5 sqrt(3N):
# with tangent_first 0.01 a cap of 0.05 is below it, with 1e-4 a cap of 1e3 above; the test asserts that both caps scaled the
# step in some configurations and not in others.  A positive lam takes the convex count.
CONFIGS = [(0, 3, -1, 1e-3, 0.05, 0.01), (1, 0, -1, 10.0, 0.05, 0.01), (0, 1, +1, 10.0, 1e3, 1e-4), (3, 0, -1, 1e-3, 0.05, 1e-4)]
SEEN = {}                                                    # dtype -> [allowed point, seen point, allowed F, seen F], printed


def _configs(n):
    return CONFIGS[:3] if n == 1024 else CONFIGS


def _batch(n):
    return 2 if n == 1024 else 3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _lowest_mode(p):
    """(u, lam): the lowest eigenpair of the projected dense fp64 Hessian at the point, u of unit length."""
    return _lowest_mode_of(tuple(np.asarray(p, dtype=np.float64).tolist()))


@functools.lru_cache(maxsize=None)
def _lowest_mode_of(p):
    ev, H, Pm = lt.dense_truth(p, np.float64)
    w, V = np.linalg.eigh(Pm @ H @ Pm)
    k = int(np.argmin(np.abs(w - ev[0])))
    return V[:, k] / np.linalg.norm(V[:, k]), float(w[k])


@functools.lru_cache(maxsize=None)
def _inputs(n, dtype):
    """Jittered lattice clusters of n particles rounded to ``dtype`` and their lowest modes, rounded likewise: points (b, 3n),
    u (b, 3n), lam (b,)."""
    dt = np.dtype(dtype)
    pts, us, lams = [], [], []
    for b in range(_batch(n)):
        p = np.concatenate(tw.lattice(n, seed=100 * n + b))
        u, lam = _lowest_mode(p)                             # of the fp64 point, for both element types: an input like any other
        pts.append(p.astype(dt)); us.append(u.astype(dt)); lams.append(lam)
    out = np.stack(pts), np.stack(us), np.array(lams).astype(dt)
    for a in out:
        a.setflags(write=False)
    return out


def _twin_args(config):
    ts, tsc, sign, max_step, cap, first = config
    return dict(max_step=max_step, tangent_steps=ts, tangent_steps_convex=tsc, tangent_cap=cap, tangent_first=first, zero_tol=ZERO_TOL, grad_tol=0.0)


@functools.lru_cache(maxsize=None)
def _twin_runs(n, dtype):
    """The twin on every configuration and instance of a shape, computed once: {(config, b): the fp64 run}, and the shape's two
    tolerances: 4 x the largest difference between the twin run in T and in the next wider format, for the point and for F."""
    dt = np.dtype(dtype)
    wider = np.float64 if dt == np.float32 else np.longdouble
    points, u, lam = _inputs(n, dtype)
    refs, diff_x, diff_f = {}, 0.0, 0.0
    for c, config in enumerate(_configs(n)):
        for b in range(_batch(n)):
            l = config[2] * abs(lam[b])
            in_t, in_wide = hy.step(points[b], u[b], l, dtype=dt, **_twin_args(config)), hy.step(points[b], u[b], l, dtype=wider, **_twin_args(config))
            refs[c, b] = in_t if dt == np.float64 else in_wide
            assert in_t["status"] == in_wide["status"] == hy.ACTIVE and in_t["tangent"] == in_wide["tangent"]
            diff_x = max(diff_x, float(np.abs(in_t["point"].astype(wider) - in_wide["point"]).max()))
            diff_f = max(diff_f, float(abs(wider(in_t["F"]) - in_wide["F"])))
    return refs, 4.0 * diff_x, 4.0 * diff_f


def _check_margins(twin):
    for name, value, threshold in twin["branches"]:
        assert abs(value - threshold) > 1e-6 * max(abs(value), abs(threshold)), (name, value, threshold)


def _apply(points, u, lam, dtype, config, grad_tol=0.0):
    """The device call on host arrays.  Returns the record dict with ``point`` added."""
    dt = np.dtype(dtype)
    batch, n3 = points.shape
    ts, tsc, sign, max_step, cap, first = config
    pdev = dzo.DeviceArray.from_host(np.ascontiguousarray(points, dtype=dt))
    r = dzo.hybridef_apply(pdev, np.ascontiguousarray(lam, dtype=dt), np.ascontiguousarray(u, dtype=dt), n3 // 3, max_step, ts, tsc, cap, first,
                           ZERO_TOL, grad_tol)
    r.update(point=pdev.to_host().reshape(batch, n3))
    return r


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", SHAPES)
def test_one_step_from_a_supplied_mode(n, dtype):
    dt = np.dtype(dtype)
    batch = _batch(n)
    points, u, lam = _inputs(n, dtype)
    refs, tol_x, tol_f = _twin_runs(n, dtype)
    e_ref = dzo.pairwise_batch_energy_gradient(dzo.DeviceArray.from_host(points), n, gref := dzo.DeviceArray((batch, 3 * n), dt))
    g_ref = gref.to_host()
    seen = SEEN.setdefault(dtype, [0.0, 0.0, 0.0, 0.0])
    capped_h, capped_t = set(), set()
    for c, config in enumerate(_configs(n)):
        lam_c = (config[2] * np.abs(lam)).astype(dt)
        dev = _apply(points, u, lam_c, dt, config)
        assert np.array_equal(dev["energies"], e_ref) and np.array_equal(dev["gradients"], g_ref)
        for b in range(batch):
            ref = refs[c, b]
            _check_margins(ref)
            assert (dev["status"][b], dev["tangent_steps"][b]) == (ref["status"], ref["tangent"]), (c, b, dev["status"][b], dev["tangent_steps"][b])
            assert ref["tangent"] == (config[0] if config[2] < 0 else config[1])
            assert dev["grms"][b] == pytest.approx(ref["grms"], rel=1e-5 if dt == np.float32 else 1e-12)
            err_x = float(np.abs(dev["point"][b].astype(np.float64) - ref["point"].astype(np.float64)).max())
            err_f = abs(float(dev["projections"][b]) - float(ref["F"]))
            print("N %d config %d b %d %s: point allowed %.3e seen %.3e, F allowed %.3e seen %.3e, h %.4g" % (n, c, b, dtype, tol_x, err_x, tol_f,
                                                                                                             err_f, dev["uphill_steps"][b]))
            seen[:] = [max(seen[0], tol_x), max(seen[1], err_x), max(seen[2], tol_f), max(seen[3], err_f)]
            assert err_x <= tol_x and err_f <= tol_f, (c, b, err_x, tol_x, err_f, tol_f)
            assert float(dev["uphill_steps"][b]) == pytest.approx(float(ref["h"]), rel=1e-3 if dt == np.float32 else 1e-9)
            branch = dict((k, (v, t)) for k, v, t in ref["branches"] if k in ("h",))
            capped_h.add((config[3] < 1, bool(branch["h"][0] > branch["h"][1])))
            capped_t.update(v > t for k, v, t in ref["branches"] if k == "dn")
            if abs(float(ref["h"])) == config[3]:
                assert abs(float(dev["uphill_steps"][b])) == dt.type(config[3])
        if c == 1:                                           # instance 1 alone: the same bits
            alone = _apply(points[1:2], u[1:2], lam_c[1:2], dt, config)
            for key in ("point", "projections", "uphill_steps", "gradients", "energies", "grms"):
                assert _same_bits(alone[key][0], dev[key][1]), key
            assert (alone["status"][0], alone["tangent_steps"][0]) == (dev["status"][1], dev["tangent_steps"][1])
    # the caps scale the step where they are meant to and nowhere else
    assert {(True, True), (False, False)} <= capped_h and (False, True) not in capped_h, capped_h
    assert capped_t == {True, False}, capped_t
    print("so far", dtype, "allowed/seen point %.3e %.3e, F %.3e %.3e" % tuple(seen))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_converged_and_nan_instances_do_not_move_and_do_not_disturb(dtype):
    dt = np.dtype(dtype)
    n = 13
    minimum = np.array(ht.polished_minimum(tw.icosahedron13))
    points = np.stack([np.concatenate(tw.lattice(n, seed=7)), minimum, np.concatenate(tw.lattice(n, seed=8)),
                       np.concatenate(tw.lattice(n, seed=9))]).astype(dt)
    modes = [_lowest_mode(p.astype(np.float64)) for p in points]
    u, lam = np.stack([m[0] for m in modes]).astype(dt), np.array([m[1] for m in modes]).astype(dt)
    points[3, 5] = np.nan
    grad_tol = 1e-8 if dt == np.float64 else 1e-3           # above the minimum's grms in T, far below the lattices'
    config = (3, 3, -1, 0.1, 0.05, 0.01)
    dev = _apply(points, u, lam, dt, config, grad_tol=grad_tol)
    assert dev["status"].tolist() == [hy.ACTIVE, hy.CONVERGED, hy.ACTIVE, hy.FAILED], (dev["status"], dev["grms"])
    assert _same_bits(dev["point"][1], points[1]) and _same_bits(dev["point"][3], points[3])
    assert dev["grms"][1] <= grad_tol and dev["uphill_steps"][[1, 3]].tolist() == [0, 0] and dev["tangent_steps"].tolist() == [3, 0, 3, 0]
    for b in (0, 2):
        alone = _apply(points[b:b + 1], u[b:b + 1], lam[b:b + 1], dt, config, grad_tol=grad_tol)
        assert _same_bits(alone["point"][0], dev["point"][b]) and not _same_bits(dev["point"][b], points[b])
    bad_mode = lam.copy()
    bad_mode[0] = np.inf
    dev = _apply(points[:1], u[:1], bad_mode[:1], dt, config)
    assert dev["status"].tolist() == [hy.FAILED] and _same_bits(dev["point"][0], points[0])


# ------------------------------------------------------------------------------ 2. the handle
SADDLE_SEEDS = [1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 14, 16, 17, 18, 19, 20]


@functools.lru_cache(maxsize=None)
def _asymmetric_minima():
    """The 16 asymmetric minima of LJ13 of tests/test_gpu_modefollow.py: the twin's polish of random starts."""
    out = []
    for seed in SADDLE_SEEDS:
        r = mt.run(mt.random_start(13, seed), max_steps=400)
        assert r["status"] == mt.CONVERGED and r["index"] == 0 and r["zeros"] == 6
        out.append(r["point"].copy())
    return np.stack(out)


def _quenched(starts, n):
    """The starts (batch, 3n) quenched by one BatchedLBFGS to all_stuck: the DeviceArray that holds them."""
    dev = dzo.DeviceArray.from_host(np.ascontiguousarray(starts, dtype=np.float64))
    q = dzo.BatchedLBFGS(dev, n, 0.01, 10)
    done, launches = q.count_active() == 0, 0
    while not done and launches < 400:
        done = q.step(50)
        launches += 1
    assert done, "the quench did not end stuck"
    q.close()
    return dev


def _index_and_zeros(p):
    lam = ht.spectrum_of(p)
    return int((lam < -ZERO_TOL).sum()), int((np.abs(lam) <= ZERO_TOL).sum())


def test_saddle_search_finds_transition_states_of_lj13():
    """From the 16 minima kicked by 0.05 along their lowest non-zero mode.  The twin finds 16 (tests/test_hybridef_twin.py), so
    the device must find 14."""
    kicked = [mt.kicked(p, 0, 0.05, ZERO_TOL) for p in _asymmetric_minima()]
    dev = dzo.DeviceArray.from_host(np.stack([k[0] for k in kicked]))
    search = dzo.HybridModeFollowing(dev, 13, np.stack([k[1] for k in kicked]), zero_tol=ZERO_TOL, grad_tol=1e-10)
    search.run(200)
    status, lam, points, steps = search.status, search.eigenvalues, search.current_points, search.iteration_counts
    good = 0
    for b in range(16):
        if status[b] != hy.CONVERGED:
            continue
        g = tw.gradient_f64(points[b])
        assert np.sqrt((g * g).sum() / 39) <= 2e-10 and lam[b] < -ZERO_TOL
        good += _index_and_zeros(points[b]) == (1, 6)
    print("twin", hy.TWIN_FOUND[0], "device", good, "steps", steps.tolist(), "products", search.products.tolist(), "evaluations",
          search.evaluations.tolist())
    assert good >= hy.TWIN_FOUND[0] - 2, (status, lam)
    assert steps.max() <= 200 and np.all(search.products >= steps) and np.all(search.evaluations >= steps)
    search.close()


def test_find_saddles_hybrid_on_38_atoms():
    n, batch = 38, 8
    dev = _quenched(np.stack([np.concatenate(tw.jittered(tw.octahedron38(), 30 + k)) for k in range(batch)]), n)
    search = dzo.find_saddles_hybrid(dev, n, kick=0.05, grad_tol=1e-10, max_steps=300, zero_tol=ZERO_TOL)
    status, points = search.status, search.current_points
    found = [status[b] == hy.CONVERGED and _index_and_zeros(points[b]) == (1, 6) for b in range(batch)]
    print("found", found, "steps", search.iteration_counts.tolist(), "products", search.products.tolist())
    assert sum(found) >= 6 and search.iteration_counts.max() <= 300
    search.close()


def test_saddles_of_130_atoms_above_the_dense_ceiling():
    """No assertion on the barrier: a search may cross into a lower basin and end on a saddle below its start."""
    n = 130
    assert n > dzo.MODEFOLLOW_MAX_PARTICLES
    dev = _quenched(np.stack([np.concatenate(tw.lattice(n, seed=40 + k)) for k in range(2)]), n)
    search = dzo.find_saddles_hybrid(dev, n, kick=0.05, grad_tol=1e-10, max_steps=400, zero_tol=ZERO_TOL)
    lam, res = search.eigenvalues, search.mode_residuals
    print("status", search.status.tolist(), "lam", lam.tolist(), "steps", search.iteration_counts.tolist(), "products", search.products.tolist(),
          "evaluations", search.evaluations.tolist(), "grms", search.grms.tolist())
    assert search.status.tolist() == [hy.CONVERGED] * 2 and np.all(lam < -ZERO_TOL) and search.iteration_counts.max() <= 400
    ev = dzo.hessian_eigenvalues(dev, n)
    for b in range(2):
        index = int((ev[b] < -ZERO_TOL).sum())
        print("instance", b, "index", index, "lowest", ev[b][:3].tolist())
        assert index >= 1
        # a Rayleigh quotient lies within its residual of an eigenvalue; it was taken on the lowest mode
        assert abs(lam[b] - ev[b][0]) <= res[b] + 1e-9 * np.abs(ev[b]).max(), (lam[b], ev[b][0], res[b])
    search.close()


@pytest.mark.parametrize("n", [13, 70])
def test_three_steps_in_one_call_or_in_three_give_the_same_bits(n):
    starts = np.stack([np.concatenate(tw.lattice(n, seed=60 + k)) for k in range(4)])
    results = []
    for calls in ((3,), (1, 1, 1)):
        dev = dzo.DeviceArray.from_host(starts)
        search = dzo.HybridModeFollowing(dev, n, None, zero_tol=ZERO_TOL, grad_tol=1e-10, seed=5)   # the first modes are drawn
        for k in calls:
            search.step(k)
        results.append([search.read(w) for w in range(14)])
        search.close()
    assert results[0][dzo.HYBRIDEF_ITERATION_COUNTS].tolist() == [3] * 4
    assert not _same_bits(results[0][dzo.HYBRIDEF_POINTS], starts)
    assert np.all(results[0][dzo.HYBRIDEF_PRODUCTS] >= 3) and np.all(results[0][dzo.HYBRIDEF_EVALUATIONS] >= 3)
    for what, (a, b) in enumerate(zip(*results)):
        assert _same_bits(a, b), what


def test_fp32_search_reaches_the_floor_of_its_element_type():
    """grad_tol is 4 x the grms the fp32 twin bottoms out at on the same starts (the smallest grms of 60 of its steps with
    grad_tol = 0).  Measured: the twin's floors are 2.4e-06 to 3.6e-06 over the four instances (grad_tol 1.5e-05); the device
    ends at 9.8e-06 to 1.4e-05 after 9 to 27 steps.  zero_tol is 1e-3: in fp32 the rigid-body eigenvalues are zeros to some 1e-4
    only."""
    n, batch = 13, 4
    kicked = [mt.kicked(p, 0, 0.05, ZERO_TOL) for p in _asymmetric_minima()[:batch]]
    floors = []
    for x, v in kicked:
        x, u, floor = x.astype(np.float32), v.astype(np.float32), np.inf
        for _ in range(60):
            m = lt.lowest_mode(x, np.float32, True, 8, 2, 1e-3, start=u)
            r = hy.step(x, m.vector, m.eigenvalue, zero_tol=1e-3, dtype=np.float32)
            x, u, floor = r["point"], m.vector, min(floor, r["grms"])
        floors.append(floor)
    grad_tol = 4.0 * max(floors)
    print("fp32 twin floors", min(floors), max(floors), "grad_tol", grad_tol)
    dev = dzo.DeviceArray.from_host(np.stack([k[0] for k in kicked]).astype(np.float32))
    search = dzo.HybridModeFollowing(dev, n, np.stack([k[1] for k in kicked]).astype(np.float32), zero_tol=1e-3, grad_tol=grad_tol)
    search.run(200)
    print("fp32 device grms", search.grms.tolist(), "steps", search.iteration_counts.tolist(), "lam", search.eigenvalues.tolist())
    assert search.status.tolist() == [hy.CONVERGED] * batch and np.all(search.eigenvalues < -1e-3)
    assert search.energies.dtype == np.float32 and search.iteration_counts.min() >= 1 and np.all(search.grms <= grad_tol)
    points = search.current_points.astype(np.float64)
    for b in range(batch):
        lam = ht.spectrum_of(points[b])
        assert (lam < -1e-3).sum() == 1
    search.close()


def test_error_codes_and_every_what():
    L = dzo.lib()
    n, batch = 5, 2
    pts = dzo.DeviceArray.from_host(np.stack([np.concatenate(tw.lattice(n, seed=k)) for k in range(batch)]))
    dirs = dzo.DeviceArray.from_host(np.stack([_lowest_mode(p)[0] for p in pts.to_host()]))
    h = ctypes.c_void_p()
    host = np.zeros(3 * n * batch)

    def create(radial=0, n_=n, batch_=batch, dtype=dzo.F64, p=pts.ptr, d=dirs.ptr, max_step=0.1, ts=10, tsc=2, cap=0.05, first=0.01, krylov=8,
               cycles=1, mode_tol=1e-3, zero_tol=1e-4, grad_tol=1e-10, seed=0, out=None):
        return L.dzo_hybridef_batch_create(radial, n_, batch_, dtype, p, d, max_step, ts, tsc, cap, first, krylov, cycles, mode_tol, zero_tol, grad_tol,
                                           seed, ctypes.byref(h) if out is None else out)

    assert create(radial=7) == 1 and create(dtype=9) == 1 and create(n_=0) == 1 and create(batch_=0) == 1 and create(p=None) == 1
    assert create(n_=2) == 1 and b"3 particles" in L.dzo_last_error()
    assert create(max_step=0.0) == 1 and create(ts=-1) == 1 and create(tsc=-1) == 1 and create(cap=0.0) == 1 and create(first=0.0) == 1
    assert create(krylov=1) == 1 and create(krylov=33) == 1 and create(cycles=0) == 1 and create(mode_tol=-1.0) == 1
    assert create(mode_tol=float("inf")) == 1 and create(zero_tol=-1e-9) == 1 and create(grad_tol=-1e-9) == 1
    assert L.dzo_hybridef_batch_create(0, n, batch, dzo.F64, pts.ptr, None, 0.1, 10, 2, 0.05, 0.01, 8, 1, 1e-3, 1e-4, 1e-10, 0, None) == 1
    assert create(n_=1025) == 5 and b"1024" in L.dzo_last_error()
    assert create(p=host.ctypes.data) == 3 and create(d=host.ctypes.data) == 3
    assert create() == 0 and h.value
    assert L.dzo_hybridef_batch_step(h, -1, None) == 1 and L.dzo_hybridef_batch_step(None, 1, None) == 1
    assert L.dzo_hybridef_batch_set_directions(h, None) == 1 and L.dzo_hybridef_batch_set_directions(h, host.ctypes.data) == 3
    assert L.dzo_hybridef_batch_set_directions(None, dirs.ptr) == 1 and L.dzo_hybridef_batch_set_directions(h, dirs.ptr) == 0
    assert L.dzo_hybridef_batch_count_active(h, None) == 1 and L.dzo_hybridef_batch_read(h, 0, None) == 1
    out = np.zeros(3 * n * batch)
    assert L.dzo_hybridef_batch_read(h, 14, out.ctypes.data) == 1 and L.dzo_hybridef_batch_read(h, -1, out.ctypes.data) == 1
    p = ctypes.c_void_p()
    assert L.dzo_hybridef_batch_get_ptr(h, 14, ctypes.byref(p)) == 1 and L.dzo_hybridef_batch_get_ptr(h, 0, None) == 1
    assert L.dzo_hybridef_batch_step(h, 0, None) == 0 and L.dzo_hybridef_batch_step(h, 2, None) == 0
    for what in range(14):
        assert L.dzo_hybridef_batch_read(h, what, out.ctypes.data) == 0, what
        assert L.dzo_hybridef_batch_get_ptr(h, what, ctypes.byref(p)) == 0 and p.value, what
    assert L.dzo_hybridef_batch_get_ptr(h, dzo.HYBRIDEF_POINTS, ctypes.byref(p)) == 0 and p.value == pts.ptr      # aliased: the caller's
    active = ctypes.c_int64(-1)
    assert L.dzo_hybridef_batch_count_active(h, ctypes.byref(active)) == 0 and 0 <= active.value <= batch
    assert L.dzo_hybridef_batch_destroy(h) == 0 and L.dzo_hybridef_batch_destroy(None) == 0
    assert create(d=None) == 0 and L.dzo_hybridef_batch_step(h, 1, None) == 0 and L.dzo_hybridef_batch_destroy(h) == 0   # drawn first modes

    # apply
    lam = dzo.DeviceArray.from_host(np.full(batch, -1.0))
    st = dzo.DeviceArray.from_host(np.zeros(batch, dtype=np.int32))

    def apply(radial=0, n_=n, batch_=batch, dtype=dzo.F64, p=pts.ptr, l=lam.ptr, u=dirs.ptr, max_step=0.1, ts=1, tsc=1, cap=0.05, first=0.01,
              zero_tol=1e-4, grad_tol=0.0, status=st.ptr):
        return L.dzo_hybridef_batch_apply(radial, n_, batch_, dtype, p, l, u, max_step, ts, tsc, cap, first, zero_tol, grad_tol, None, None, None,
                                          None, None, status, None)

    assert apply(radial=7) == 1 and apply(dtype=9) == 1 and apply(n_=0) == 1 and apply(n_=2) == 1 and apply(batch_=0) == 1
    assert apply(p=None) == 1 and apply(l=None) == 1 and apply(u=None) == 1 and apply(status=None) == 1
    assert apply(max_step=0.0) == 1 and apply(ts=-1) == 1 and apply(cap=-1.0) == 1 and apply(first=0.0) == 1 and apply(zero_tol=-1.0) == 1
    assert apply(grad_tol=-1.0) == 1 and apply(n_=1025) == 5
    assert apply(p=host.ctypes.data) == 3 and apply(l=host.ctypes.data) == 3 and apply(u=host.ctypes.data) == 3 and apply(status=host.ctypes.data) == 3
    before = pts.to_host()
    assert apply(grad_tol=1e9) == 0 and st.to_host().tolist() == [hy.CONVERGED] * batch and _same_bits(pts.to_host(), before)
    assert apply() == 0 and st.to_host().tolist() == [hy.ACTIVE] * batch and not _same_bits(pts.to_host(), before)


def test_lj_saddle_large_example_prints_ok(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_saddle_large")
    r = subprocess.run([exe, "150", "4"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout and "barrier" in r.stdout, r.stderr
