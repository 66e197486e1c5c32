"""Batched eigenvector following on the device (csrc/dzo_modefollow.hip) against its CPU twin (tests/modefollow_twin.py).

1. ONE step from modes the test supplies (``dzo_modefollow_batch_apply``; the modes are ``numpy.linalg.eigh`` of the twin
   Hessian, so nothing here depends on the device eigensolver), at N = 2, 3 (fewest non-zero modes), 21, 22 (n = 63, 66: across
   a wave), 85, 86 (n = 255, 258: across the block) and 128 (n = 384, the maximum), batch 3, both element types, target index
   0 and 1, start modes 0 and 1, with and without a followed vector, with the cap scaling the step and not:

   * E and g equal ``dzo_pairwise_batch_energy_gradient`` with ``==``;
   * index, zeros, followed mode and status equal the twin's exactly; the inputs are checked (on the twin's values) to sit
     more than 1e-6 relative away from what could flip them: an eigenvalue at +-zero_tol, two equal largest overlaps, and
     -- for N >= 3 -- two equal non-zero eigenvalues (N = 2 is a diatomic: its two rotations share one eigenvalue by symmetry,
     which is harmless here because the modes are supplied and chosen by position);
   * the new point and F against the twin run in fp64 on the same inputs.  The tolerance is not fixed in advance: it is
     4 x the largest difference, over the configurations and instances of a shape, between the twin run in T and the twin run
     in the next wider format on the same inputs (fp32 against fp64; fp64 against numpy.longdouble, because an fp64 run
     measured against an fp64 run shows no rounding at all), the factor 4 for the differing summation orders.  Measured on an MI355X, the largest over the shapes
     (at N = 86): fp64, twin difference 4.4e-15 (point) and 5.4e-14 (F), so 1.8e-14 and 2.2e-13 allowed, 4.2e-15 and 2.1e-14
     seen; fp32, twin difference 2.4e-06 and 2.1e-05, so 9.6e-06 and 8.5e-05 allowed, 9.5e-07 and 2.2e-05 seen.  The
     tightest shape is N = 2 in fp64: 2.6e-16 allowed for the point, 1.4e-17 seen;
   * an instance gives the same bits alone and inside the batch;
   * a converged instance does not move; a NaN coordinate gives FAILED, no move, and leaves its neighbours' bits alone.

2. The handle: (a) polish of quenched clusters, (b) transition states from asymmetric LJ13 minima, (c) batching, the two
   storages of the eigensolver and fp32, (d) error codes and every ``what``.
"""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import hessian_twin as ht
import modefollow_twin as mt
import pairwise_twin as tw
from build_checks import link_example
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ZERO_TOL = 1e-4
SHAPES = [2, 3, 21, 22, 85, 86, 128]
BATCH = 3
# (target_index, start_mode, followed vector set, max_step): 0.05 is below and 1e3 above every step length of these inputs
CONFIGS = [(0, 0, False, 0.05), (0, 0, False, 1e3), (1, 0, False, 0.05), (1, 1, False, 1e3), (1, 0, True, 1e3), (1, 1, True, 0.05)]
SEEN = {}                                                    # dtype -> [allowed point, seen point, allowed F, seen F], printed


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _inputs(n, dtype):
    """Three different jittered lattice clusters of n particles rounded to ``dtype`` and their modes (eigh of the fp64 twin
    Hessian at the rounded point, rounded to ``dtype``): points (3, 3n), lam (3, 3n), V (3, 3n, 3n) with V[b][:, k]."""
    dt = np.dtype(dtype)
    pts, lams, vecs = [], [], []
    for b in range(BATCH):
        p = np.concatenate(tw.lattice(n, seed=100 * n + b)).astype(dt)
        lam, V = mt.modes(p.astype(np.float64))
        pts.append(p); lams.append(lam.astype(dt)); vecs.append(V.astype(dt))
    out = np.stack(pts), np.stack(lams), np.stack(vecs)
    for a in out:
        a.setflags(write=False)
    return out


def _follow_vectors(V, lam, start_mode):
    """A followed vector per instance that is no eigenvector: mostly the mode two places above the start_mode-th non-zero
    one, with a share of its neighbours."""
    n = V.shape[1]
    w = np.zeros((len(V), n), dtype=V.dtype)
    for b in range(len(V)):
        nonzero = np.flatnonzero(np.abs(lam[b]) > V.dtype.type(ZERO_TOL))
        k = [nonzero[min(start_mode + j, len(nonzero) - 1)] for j in (2, 1, 3)]
        w[b] = V[b][:, k[0]] - V.dtype.type(0.4) * V[b][:, k[1]] + V.dtype.type(0.3) * V[b][:, k[2]]
    return w


def _check_margins(n, lam, twin):
    """The integer records cannot flip: on the twin's values."""
    a = np.abs(lam.astype(np.float64))
    assert np.all(np.abs(a - ZERO_TOL) > 1e-6 * ZERO_TOL), "an eigenvalue within 1e-6 relative of zero_tol"
    nz = np.sort(a[a > ZERO_TOL])
    if n >= 3 and len(nz) > 1:
        assert np.all(np.diff(nz) > 1e-6 * nz[1:]), "two non-zero eigenvalues within 1e-6 relative of a tie"
    if twin["overlaps"] is not None:
        ov = np.sort(twin["overlaps"][a > ZERO_TOL])
        assert len(ov) < 2 or ov[-1] - ov[-2] > 1e-6 * ov[-1], "the two largest overlaps within 1e-6 relative of a tie"


@functools.lru_cache(maxsize=None)
def _twin_runs(n, dtype):
    """The twin on every configuration and instance of a shape, computed once: {(config, b): the fp64 run}, and the shape's
    two tolerances: 4 x the largest difference, over the shape's configurations and instances, between the twin run in T and
    the twin run in the next wider format, for the new point and for F."""
    dt = np.dtype(dtype)
    wider = np.float64 if dt == np.float32 else np.longdouble
    points, lam, V = _inputs(n, dtype)
    refs, diff_x, diff_f = {}, 0.0, 0.0
    for config, (target, start, with_w, max_step) in enumerate(CONFIGS):
        w = _follow_vectors(V, lam, start) if with_w else None
        for b in range(BATCH):
            args = dict(w=None if w is None else w[b], w_set=with_w, target_index=target, start_mode=start, max_step=max_step, zero_tol=ZERO_TOL,
                        grad_tol=0.0)
            in_t, in_wide = mt.step(points[b], lam[b], V[b], dtype=dt, **args), mt.step(points[b], lam[b], V[b], dtype=wider, **args)
            refs[config, b] = in_t if dt == np.float64 else in_wide
            assert in_t["status"] == in_wide["status"] and in_t["followed"] == in_wide["followed"]
            if in_t["status"] == mt.ACTIVE:
                diff_x = max(diff_x, float(np.abs(in_t["point"].astype(wider) - in_wide["point"]).max()))
                diff_f = max(diff_f, float(np.abs(in_t["F"].astype(wider) - in_wide["F"]).max()))
    return refs, 4.0 * diff_x, 4.0 * diff_f


def _apply(points, lam, V, dtype, target_index, start_mode, max_step, grad_tol=0.0, w=None):
    """The device call on host arrays (V[b][:, k] the vector of eigenvalue k).  Returns the record dict with ``point``, ``w``
    and ``w_set`` added."""
    dt = np.dtype(dtype)
    batch, n3 = points.shape
    pdev = dzo.DeviceArray.from_host(np.ascontiguousarray(points, dtype=dt))
    vdev = dzo.DeviceArray.from_host(np.ascontiguousarray(V.transpose(0, 2, 1), dtype=dt))   # [b, k, :]
    follow = dzo.DeviceArray.from_host(np.zeros((batch, n3), dtype=dt) if w is None else np.ascontiguousarray(w, dtype=dt))
    fset = dzo.DeviceArray.from_host(np.full(batch, 0 if w is None else 1, dtype=np.int32))
    r = dzo.modefollow_apply(pdev, np.ascontiguousarray(lam, dtype=dt), vdev, n3 // 3, target_index, start_mode, max_step, ZERO_TOL, grad_tol,
                             follow if target_index == 1 else None, fset if target_index == 1 else None)
    r.update(point=pdev.to_host().reshape(batch, n3), w=follow.to_host().reshape(batch, n3), w_set=fset.to_host())
    return r


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("config", range(len(CONFIGS)))
@pytest.mark.parametrize("n", SHAPES)
def test_one_step_from_supplied_modes(n, config, dtype):
    dt = np.dtype(dtype)
    target, start, with_w, max_step = CONFIGS[config]
    points, lam, V = _inputs(n, dtype)
    w = _follow_vectors(V, lam, start) if with_w else None
    dev = _apply(points, lam, V, dt, target, start, max_step, w=w)
    refs, tol_x, tol_f = _twin_runs(n, dtype)
    e_ref = dzo.pairwise_batch_energy_gradient(dzo.DeviceArray.from_host(points), n, gref := dzo.DeviceArray((BATCH, 3 * n), dt))
    assert np.array_equal(dev["energies"], e_ref) and np.array_equal(dev["gradients"], gref.to_host())
    seen = SEEN.setdefault(dtype, [0.0, 0.0, 0.0, 0.0])
    capped = []
    for b in range(BATCH):
        ref = refs[config, b]
        _check_margins(n, lam[b], ref)
        got = (dev["status"][b], dev["index"][b], dev["zeros"][b], dev["followed_mode"][b])
        assert got == (ref["status"], ref["index"], ref["zeros"], ref["followed"]), (b, got, ref["status"], ref["index"], ref["zeros"], ref["followed"])
        assert dev["grms"][b] == pytest.approx(ref["grms"], rel=1e-5 if dt == np.float32 else 1e-12)
        if ref["status"] != mt.ACTIVE:                       # N = 2 has one non-zero mode beyond the rotations' pair
            assert _same_bits(dev["point"][b], points[b]) and dev["step_lengths"][b] == 0.0
            continue
        err_x = float(np.abs(dev["point"][b].astype(np.float64) - ref["point"]).max())
        err_f = float(np.abs(dev["projections"][b].astype(np.float64) - ref["F"]).max())
        print("N %d b %d %s: point allowed %.3e seen %.3e, F allowed %.3e seen %.3e, step %.4g" % (n, b, dtype, tol_x, err_x, tol_f, err_f,
                                                                                                 dev["step_lengths"][b]))
        seen[:] = [max(seen[0], tol_x), max(seen[1], err_x), max(seen[2], tol_f), max(seen[3], err_f)]
        assert err_x <= tol_x and err_f <= tol_f, (b, err_x, tol_x, err_f, tol_f)
        assert dev["step_lengths"][b] == pytest.approx(ref["step_length"], rel=1e-4 if dt == np.float32 else 1e-10)
        capped.append(ref["step_length"] == max_step)
        if target == 1:
            assert dev["w_set"][b] == 1 and _same_bits(dev["w"][b], V[b][:, ref["followed"]].copy())
    if n >= 3:                                               # (a diatomic near its bond length takes shorter steps than 0.05)
        assert all(capped) if max_step < 1 else not any(capped)   # the cap scales the step in one half of the configurations only
    print("so far", dtype, "allowed/seen point %.3e %.3e, F %.3e %.3e" % tuple(seen))
    # instance 1 alone: the same bits
    alone = _apply(points[1:2], lam[1:2], V[1:2], dt, target, start, max_step, w=None if w is None else w[1:2])
    for key in ("point", "projections", "gradients", "energies", "grms", "step_lengths", "w"):
        assert _same_bits(alone[key][0], dev[key][1]), key
    assert (alone["status"][0], alone["followed_mode"][0]) == (dev["status"][1], dev["followed_mode"][1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_converged_and_nan_instances_do_not_move_and_do_not_disturb(dtype):
    dt = np.dtype(dtype)
    n = 13
    minimum = np.array(ht.polished_minimum(tw.icosahedron13))
    points = np.stack([np.concatenate(tw.lattice(n, seed=7)), minimum, np.concatenate(tw.lattice(n, seed=8)),
                       np.concatenate(tw.lattice(n, seed=9))]).astype(dt)
    points[3, 5] = np.nan
    modes = [mt.modes(np.nan_to_num(p.astype(np.float64))) for p in points]
    lam, V = np.stack([m[0] for m in modes]).astype(dt), np.stack([m[1] for m in modes]).astype(dt)
    grad_tol = 1e-8 if dt == np.float64 else 1e-3           # above the minimum's grms in T, far below the lattices'
    dev = _apply(points, lam, V, dt, 0, 0, 0.2, grad_tol=grad_tol)
    assert dev["status"].tolist() == [mt.ACTIVE, mt.CONVERGED, mt.ACTIVE, mt.FAILED], (dev["status"], dev["grms"])
    assert _same_bits(dev["point"][1], points[1]) and _same_bits(dev["point"][3], points[3])
    assert dev["grms"][1] <= grad_tol and dev["step_lengths"][1] == 0 and dev["step_lengths"][3] == 0
    assert dev["index"][1] == 0 and dev["zeros"][1] == 6 and dev["followed_mode"].tolist() == [-1] * 4
    for b in (0, 2):
        alone = _apply(points[b:b + 1], lam[b:b + 1], V[b:b + 1], dt, 0, 0, 0.2, grad_tol=grad_tol)
        assert _same_bits(alone["point"][0], dev["point"][b]) and not _same_bits(dev["point"][b], points[b])


# ------------------------------------------------------------------------------ 2. the handle
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


def _polish_starts(n, batch):
    """What the quench is given: at N = 13 the 16 asymmetric minima below, at N = 38 the truncated octahedron, every coordinate
    displaced by a uniform +-0.05 (seeded).  (From a random start the quench can end stuck far from any minimum.)"""
    if n == 13:
        base = _asymmetric_minima()[:batch]
        return base + np.random.default_rng(5).uniform(-0.05, 0.05, size=base.shape)
    return np.stack([np.concatenate(tw.jittered(tw.octahedron38(), 30 + k)) for k in range(batch)])


def _grms_of(points_dev, n):
    g = dzo.DeviceArray((points_dev.size // (3 * n), 3 * n), points_dev.dtype)
    dzo.pairwise_batch_energy_gradient(points_dev, n, g)
    g = g.to_host().astype(np.float64)
    return np.sqrt((g * g).sum(axis=1) / (3 * n))


@pytest.mark.parametrize("n,batch", [(13, 16), (38, 8)])
def test_polish_brings_quenched_clusters_to_a_rounding_level_gradient(n, batch):
    """Energies against the twin's polish of the same quenched points.  Both sum N (N - 1) / 2 pair terms, each carrying a few
    roundings (at most 6 eps relative), in partial sums of at most N terms: either value is within (N + 6) eps sum|pair terms|
    of the exact energy of its point, and the two points, both with grms <= 1e-10, differ in energy by g.H^-1.g / 2 ~ 1e-19.
    The bound is therefore 2 (N + 6) eps sum|pair terms|: about 3.7e-13 at N = 13 and 3.4e-12 at N = 38."""
    dev = _quenched(_polish_starts(n, batch), n)
    quenched = dev.to_host().reshape(batch, 3 * n)
    before = _grms_of(dev, n)
    mf = dzo.ModeFollowing(dev, n, 0, max_step=0.2, zero_tol=ZERO_TOL, grad_tol=1e-10)
    assert mf.status.tolist() == [mt.ACTIVE] * batch
    done = mf.step(20)
    print("grms before", before.max(), "after", mf.grms.max(), "steps", mf.iteration_counts.tolist())
    assert done and mf.count_active() == 0
    assert mf.status.tolist() == [mt.CONVERGED] * batch and mf.index.tolist() == [0] * batch and mf.zeros.tolist() == [6] * batch
    assert mf.iteration_counts.max() <= 19 and np.all(mf.sweeps >= 0)
    assert np.all(_grms_of(dev, n) <= 1e-10) and np.all(mf.grms <= 1e-10)
    energies, points = mf.energies, mf.current_points
    for b in range(batch):
        ref = mt.run(quenched[b], 0, 0, 0.2, ZERO_TOL, 1e-10, 20)
        bound = 2 * (n + 6) * np.finfo(np.float64).eps * mt.pair_term_magnitude(ref["point"])
        assert ref["status"] == mt.CONVERGED and abs(energies[b] - float(ref["E"])) <= bound, (b, energies[b], float(ref["E"]), bound)
        assert np.abs(points[b] - ref["point"]).max() <= 1e-8
    mf.close()


SADDLE_SEEDS = [1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 14, 16, 17, 18, 19, 20]


@functools.lru_cache(maxsize=None)
def _asymmetric_minima():
    """16 different asymmetric minima of LJ13: the twin's polish of random starts (none is the icosahedron: every gap between
    non-zero eigenvalues is above 1e-3 relative)."""
    out = []
    for seed in SADDLE_SEEDS:
        r = mt.run(mt.random_start(13, seed), max_steps=400)
        lam = mt.modes(r["point"])[0][6:]
        assert r["status"] == mt.CONVERGED and r["index"] == 0 and r["zeros"] == 6 and np.min(np.diff(lam) / lam[1:]) > 1e-3
        out.append(r["point"].copy())
    return np.stack(out)


@pytest.mark.parametrize("start_mode", [0, 1])
def test_saddle_search_finds_transition_states_of_lj13(start_mode):
    minima = _asymmetric_minima()
    e_min = np.array([tw.energy_f64(p) for p in minima])
    twin_ok = 0
    for b, p in enumerate(minima):
        x, v = mt.kicked(p, start_mode, 0.05, ZERO_TOL)
        r = mt.run(x, 1, start_mode, 0.1, ZERO_TOL, 1e-10, 200, w=v)
        twin_ok += r["status"] == mt.CONVERGED and r["index"] == 1 and r["zeros"] == 6 and r["steps"] <= 200
    assert twin_ok >= 14, twin_ok
    dev = dzo.DeviceArray.from_host(minima)
    saddles, polished = dzo.find_saddles(dev, 13, start_mode=start_mode, kick=0.05, grad_tol=1e-10, max_steps=200, max_step=0.1,
                                         zero_tol=ZERO_TOL)
    assert polished.status.tolist() == [mt.CONVERGED] * 16 and np.abs(polished.energies - e_min).max() <= 1e-9
    status, index, zeros, energies, points = saddles.status, saddles.index, saddles.zeros, saddles.energies, saddles.current_points
    good = (status == mt.CONVERGED) & (index == 1) & (zeros == 6)
    print("twin", twin_ok, "device", int(good.sum()), "steps", saddles.iteration_counts.tolist(), "barriers", (energies - e_min).round(4).tolist())
    assert good.sum() >= 12, (status, index, zeros)
    assert saddles.iteration_counts.max() <= 200
    for b in np.flatnonzero(status == mt.CONVERGED):
        lam = ht.spectrum_of(points[b])
        assert ((lam < -ZERO_TOL).sum(), (np.abs(lam) <= ZERO_TOL).sum()) == (index[b], zeros[b]), (b, lam[:8])
        g = tw.gradient_f64(points[b])
        assert np.sqrt((g * g).sum() / 39) <= 2e-10
        assert energies[b] > polished.energies[b], (b, energies[b], polished.energies[b])


def test_three_steps_in_one_call_or_in_three_give_the_same_bits():
    starts = np.stack([np.concatenate(tw.lattice(13, seed=60 + k)) for k in range(4)])
    results = []
    for calls in ((3,), (1, 1, 1)):
        dev = dzo.DeviceArray.from_host(starts)
        mf = dzo.ModeFollowing(dev, 13, 1, max_step=0.1, zero_tol=ZERO_TOL, grad_tol=1e-10)
        mf.set_start_mode(1)
        for k in calls:
            mf.step(k)
        results.append([mf.read(w) for w in range(14)])
        mf.close()
    assert results[0][dzo.MODEFOLLOW_ITERATION_COUNTS].tolist() == [3] * 4
    assert not _same_bits(results[0][dzo.MODEFOLLOW_POINTS], starts)
    for what, (a, b) in enumerate(zip(*results)):
        assert _same_bits(a, b), what


@pytest.mark.parametrize("n", [47, 48])
def test_both_storages_of_the_eigensolver_run(n):
    """N = 47 (n = 141) is the last size the eigensolver keeps in LDS in fp64, N = 48 the first in device memory."""
    assert dzo.symeig_plan(3 * n, np.float64)[0] == (dzo.SYMEIG_STORAGE_LDS if n == 47 else dzo.SYMEIG_STORAGE_MEMORY)
    starts = np.stack([np.concatenate(tw.lattice(n, seed=70 + k)) for k in range(2)])
    dev = dzo.DeviceArray.from_host(starts)
    mf = dzo.ModeFollowing(dev, n, 0, max_step=0.2, zero_tol=ZERO_TOL, grad_tol=1e-10)
    e0 = mf.energies
    assert np.allclose(e0, [tw.energy_f64(p) for p in starts], rtol=1e-12)
    mf.step(4)
    points = mf.current_points
    for b in range(2):                                       # the twin's fourth point: the same walk to rounding
        x = starts[b]
        for _ in range(4):
            lam, V = mt.modes(x)
            x = mt.step(x, lam, V, max_step=0.2, zero_tol=ZERO_TOL)["point"]
        assert np.abs(points[b] - x).max() <= 1e-7, np.abs(points[b] - x).max()
    assert mf.iteration_counts.tolist() == [4, 4] and np.all(mf.sweeps > 0) and np.all(mf.step_lengths <= 0.2)
    assert np.all(mf.energies < e0)
    mf.close()


def test_fp32_polish_reaches_the_floor_of_its_element_type():
    """grad_tol is 4 x the grms the fp32 twin bottoms out at on the same quenched points (the smallest grms of 12 of its steps
    with grad_tol = 0).  Measured: the twin's floors are 2.9e-06 to 5.3e-06 over the eight instances (grad_tol 2.1e-05); the device ends at 3.9e-06 to
    7.1e-06 after two moves each.  zero_tol is 1e-3: in fp32 the rigid-body eigenvalues are zeros to some 1e-4 only."""
    n, batch = 13, 8
    quenched = _quenched(_polish_starts(n, batch), n).to_host().reshape(batch, 3 * n)
    quenched = quenched + np.random.default_rng(6).uniform(-1e-3, 1e-3, size=quenched.shape)   # rounded to fp32 the quench's points are at the floor already
    floors = []
    for b in range(batch):
        x, floor = quenched[b].astype(np.float32), np.inf
        for _ in range(12):
            lam, V = mt.modes(x.astype(np.float64))
            r = mt.step(x, lam.astype(np.float32), V.astype(np.float32), max_step=0.2, zero_tol=1e-3, dtype=np.float32)
            x, floor = r["point"], min(floor, r["grms"])
        floors.append(floor)
    grad_tol = 4.0 * max(floors)
    print("fp32 twin floors", min(floors), max(floors), "grad_tol", grad_tol)
    dev = dzo.DeviceArray.from_host(quenched.astype(np.float32))
    mf = dzo.polish_minima(dev, n, grad_tol=grad_tol, max_steps=20, zero_tol=1e-3)
    print("fp32 device grms", mf.grms.tolist(), "steps", mf.iteration_counts.tolist())
    assert mf.status.tolist() == [mt.CONVERGED] * batch and mf.index.tolist() == [0] * batch and mf.zeros.tolist() == [6] * batch
    assert np.all(_grms_of(dev, n) <= grad_tol) and mf.energies.dtype == np.float32 and mf.iteration_counts.min() >= 1
    mf.close()


def test_error_codes_and_every_what():
    L = dzo.lib()
    n, batch = 5, 2
    pts = dzo.DeviceArray.from_host(np.stack([np.concatenate(tw.lattice(n, seed=k)) for k in range(batch)]))
    h = ctypes.c_void_p()

    def create(radial=0, n_=n, batch_=batch, dtype=dzo.F64, p=pts.ptr, target=0, max_step=0.2, zero_tol=1e-4, grad_tol=1e-10, out=None):
        return L.dzo_modefollow_batch_create(radial, n_, batch_, dtype, p, target, max_step, zero_tol, grad_tol, ctypes.byref(h) if out is None else out)

    assert create(radial=7) == 1 and create(dtype=9) == 1 and create(n_=0) == 1 and create(batch_=0) == 1 and create(p=None) == 1
    assert create(target=2) == 1 and create(target=-1) == 1 and create(max_step=0.0) == 1 and create(max_step=-1.0) == 1
    assert create(zero_tol=-1e-9) == 1 and create(grad_tol=-1e-9) == 1
    assert L.dzo_modefollow_batch_create(0, n, batch, dzo.F64, pts.ptr, 0, 0.2, 1e-4, 1e-10, None) == 1
    assert create(n_=129) == 5 and b"128" in L.dzo_last_error()
    host = np.zeros(3 * n * batch)
    assert create(p=host.ctypes.data) == 3
    assert create() == 0 and h.value
    assert L.dzo_modefollow_batch_step(h, -1, None) == 1 and L.dzo_modefollow_batch_step(None, 1, None) == 1
    assert L.dzo_modefollow_batch_set_start_mode(h, -1) == 1 and L.dzo_modefollow_batch_set_start_mode(None, 0) == 1
    assert L.dzo_modefollow_batch_set_directions(h, None) == 1 and L.dzo_modefollow_batch_set_directions(h, host.ctypes.data) == 3
    assert L.dzo_modefollow_batch_count_active(h, None) == 1 and L.dzo_modefollow_batch_read(h, 0, None) == 1
    out = np.zeros(3 * n * 3 * n * batch)
    assert L.dzo_modefollow_batch_read(h, 14, out.ctypes.data) == 1 and L.dzo_modefollow_batch_read(h, -1, out.ctypes.data) == 1
    p = ctypes.c_void_p()
    assert L.dzo_modefollow_batch_get_ptr(h, 14, ctypes.byref(p)) == 1 and L.dzo_modefollow_batch_get_ptr(h, 0, None) == 1
    assert L.dzo_modefollow_batch_step(h, 0, None) == 0 and L.dzo_modefollow_batch_step(h, 2, None) == 0
    for what in range(14):
        assert L.dzo_modefollow_batch_read(h, what, out.ctypes.data) == 0, what
        assert L.dzo_modefollow_batch_get_ptr(h, what, ctypes.byref(p)) == 0 and p.value, what
    assert L.dzo_modefollow_batch_get_ptr(h, dzo.MODEFOLLOW_POINTS, ctypes.byref(p)) == 0 and p.value == pts.ptr      # aliased
    assert L.dzo_modefollow_batch_destroy(h) == 0 and L.dzo_modefollow_batch_destroy(None) == 0

    # apply
    lam, vec = dzo.DeviceArray.zeros((batch, 3 * n)), dzo.DeviceArray.zeros((batch, 3 * n, 3 * n))
    st, fs = (dzo.DeviceArray.from_host(np.zeros(batch, dtype=np.int32)) for _ in range(2))

    def apply(radial=0, n_=n, batch_=batch, dtype=dzo.F64, p=pts.ptr, l=lam.ptr, v=vec.ptr, w=None, ws=None, target=0, start=0, max_step=0.2,
              zero_tol=1e-4, grad_tol=0.0, status=st.ptr):
        return L.dzo_modefollow_batch_apply(radial, n_, batch_, dtype, p, l, v, w, ws, target, start, max_step, zero_tol, grad_tol, None, None,
                                            None, None, status, None, None, None, None)

    assert apply(radial=7) == 1 and apply(dtype=9) == 1 and apply(n_=0) == 1 and apply(batch_=0) == 1
    assert apply(p=None) == 1 and apply(l=None) == 1 and apply(v=None) == 1 and apply(status=None) == 1
    assert apply(target=2) == 1 and apply(start=-1) == 1 and apply(max_step=0.0) == 1 and apply(zero_tol=-1.0) == 1 and apply(grad_tol=-1.0) == 1
    assert apply(target=1) == 1                              # no followed vectors
    assert apply(n_=129) == 5
    assert apply(p=host.ctypes.data) == 3 and apply(l=host.ctypes.data) == 3 and apply(status=host.ctypes.data) == 3
    assert apply(target=1, w=host.ctypes.data, ws=fs.ptr) == 3
    before = pts.to_host()
    assert apply(grad_tol=1e9) == 0 and st.to_host().tolist() == [mt.CONVERGED] * batch and _same_bits(pts.to_host(), before)


def test_lj_saddle_example_prints_transition_states(tmp_path):
    exe, _, _ = link_example(tmp_path, "lj_saddle")
    r = subprocess.run([exe, "200", "2"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout and "transition state" in r.stdout, r.stderr
