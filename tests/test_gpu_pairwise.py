"""The pairwise radial (Lennard-Jones) N-body objective on the device (csrc/dzo_pairwise.hip: the GPU kernels of the
reference's src/ExampleFunctions.jl) against its CPU twin (tests/pairwise_twin.py).

1. per-term arithmetic bit for bit (N = 2: no summation order exists);
2. sums against a DERIVED bound: |gpu_i - exact_i| <= (N + 32) u S_i, S_i = the sum of the absolute values of the
   terms of row i, u = 2^-53 / 2^-24.  Any order of summing N terms costs at most (N - 1) u sum|t| to first order, a
   term carries at most ~32 u of its own (three squares and two adds into r2, one division, a seventh power of the
   result, two or three more products).  Not a measured tolerance;
3. semantics: determinism, unaligned views, coincident particles, energy_delta, error codes;
4. the problem kind DZO_PROBLEM_PAIRWISE_LJ;
5. the optimizers on it: the invariants of the reference's run_and_test! (legacy/DZOptimization.jl:998-1045, compared
   with ==) and the two literature minima;
6. the plain-C example.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import pairwise_twin as tw
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
LD = np.longdouble
U = {np.dtype(np.float64): LD(2.0) ** -53, np.dtype(np.float32): LD(2.0) ** -24}
NS = [1, 3, 38, 63, 64, 65, 257, 1000, 4099]
N_SPLIT = 20011                                  # the split-j regime
DTYPES = [np.float64, np.float32]


# ------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _config(n, dtype):
    """x, y, z, u, v, w as fp64 arrays holding values of `dtype` (so that the twin sees exactly what the device sees)."""
    xyz = tw.cluster(n, seed=n)
    uvw = np.random.default_rng(1000 + n).normal(size=(3, n))
    return tuple(np.asarray(a, dtype=dtype).astype(np.float64) for a in (*xyz, *uvw))


@functools.lru_cache(maxsize=None)
def _twin(n, dtype):
    x, y, z, u, v, w = _config(n, dtype)
    return {"energy": tw.energy(x, y, z), "gradient": tw.gradient(x, y, z), "hvp": tw.hvp(x, y, z, u, v, w)}


def _dev(arrays, dtype):
    """One device buffer [a0 | a1 | ...] and the views of its parts."""
    n = len(arrays[0])
    buf = dzo.DeviceArray.from_host(np.concatenate(arrays), dtype=dtype)
    return buf, [buf.view(k * n, n) for k in range(len(arrays))]


def _out3(n, dtype):
    buf = dzo.DeviceArray.zeros(3 * n, dtype)
    return buf, [buf.view(k * n, n) for k in range(3)]


def _gpu_all(n, dtype, cfg=None):
    cfg = _config(n, dtype) if cfg is None else cfg
    keep, (x, y, z, u, v, w) = _dev(cfg, dtype)
    e = dzo.pairwise_radial_energy(x, y, z)
    gb, g = _out3(n, dtype)
    dzo.pairwise_radial_gradient_(*g, x, y, z)
    pb, p = _out3(n, dtype)
    dzo.pairwise_radial_hvp_(*p, x, y, z, u, v, w)
    return e, gb.to_host().reshape(3, n), pb.to_host().reshape(3, n)


def _check_rows(what, n, dtype, got, exact, S, Sc=None):
    """|got - exact| <= (N + 32) u S_i for every component; S_i is one number per row (the sum of the absolute values -- the
    lengths -- of the row's terms).  Sc, the same sum per component, is a stricter scale: its ratio is printed, not asserted."""
    S = np.asarray(S, dtype=LD)
    bound = LD(n + 32) * U[np.dtype(dtype)] * (S[None, :] if got.ndim == 2 else S)
    err = np.abs(got.astype(LD) - exact)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        extra = ""
        if Sc is not None:
            bc = LD(n + 32) * U[np.dtype(dtype)] * Sc
            extra = f" (against the per-component sums: {float(np.max(np.where(bc > 0, err / bc, np.where(err > 0, np.inf, 0.0)))):.4f})"
    print(f"{what} N={n} {np.dtype(dtype).name}: worst error / bound = {float(np.max(ratio)):.4f}{extra}")
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (what, n, np.dtype(dtype).name, bad[:5].tolist(), float(err[tuple(bad[0])]), float(np.broadcast_to(bound, err.shape)[tuple(bad[0])]))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ------------------------------------------------------------------------------ 1. per-term arithmetic, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_pairs_bit_for_bit(dtype):
    rng = np.random.default_rng(20)
    for k in range(200):
        r2 = np.exp(rng.uniform(np.log(0.6), np.log(16.0)))
        d = rng.normal(size=3); d *= np.sqrt(r2) / np.linalg.norm(d)
        p0 = rng.uniform(-1, 1, size=3)
        p0, p1 = np.asarray(p0, dtype), np.asarray(p0 + d, dtype)
        u0, u1 = np.asarray(rng.normal(size=3), dtype), np.asarray(rng.normal(size=3), dtype)
        cfg = [np.array([p0[c], p1[c]], dtype=np.float64) for c in range(3)] + [np.array([u0[c], u1[c]], dtype=np.float64) for c in range(3)]
        e, g, p = _gpu_all(2, dtype, cfg)
        want_e = tw.pair_energy(p0, p1, dtype)
        want_g = np.array(tw.pair_gradient(p0, p1, dtype), dtype=dtype).T          # [component, particle]
        want_p = np.array(tw.pair_hvp(p0, p1, u0, u1, dtype), dtype=dtype).T
        assert np.float64(e).view(np.int64) == np.float64(want_e).view(np.int64), (k, e, want_e)
        assert np.array_equal(_bits(g), _bits(want_g)), (k, g, want_g)
        assert np.array_equal(_bits(p), _bits(want_p)), (k, p, want_p)


# ------------------------------------------------------------------------------ 2. sums against the derived bound
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS)
def test_sums_within_the_derived_bound(n, dtype):
    """S_i is the issue's: ONE scale per row, the sum over j of the lengths of the row's (vector) terms.  Measured on the
    device against the stricter per-component sums (printed next to each ratio): at most 0.47 of the bound for N >= 38, but
    1.0176 (fp64) and 1.0556 (fp32) at N = 3 -- bit for bit what the reference's own sequential loop gives on the CPU, since
    e'(r2) = -12 inv_r8 (2 inv_r6 - 1) cancels at r = 2^(1/6) = 1.1225 next to the 1.12 lattice spacing and a component of a
    two-term row has nothing else to cover the rounding of inv_r6.  A term's own ~32 u are 32 u of its length, not of each
    of its components, which is what the row scale expresses.  The bound is not a theorem at N = 3 even so: over lattice
    seeds 0 ... 39 the REFERENCE's loop reaches 2.1 times the row-scale bound when both neighbours of a particle sit at the
    zero of e' (this file's seed rule, seed = N, fixed before the first run, gives 0.84 in fp64 and 0.38 in fp32)."""
    e, g, p = _gpu_all(n, dtype)
    twin = _twin(n, dtype)
    E, S = twin["energy"]
    _check_rows("energy", n, dtype, np.array([e]), np.array([E], dtype=LD), np.array([S], dtype=LD))
    _check_rows("gradient", n, dtype, g, *twin["gradient"])
    _check_rows("hvp", n, dtype, p, *twin["hvp"])
    if n == 1:
        assert e == 0.0 and not g.any() and not p.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_j_regime(dtype):
    n = N_SPLIT
    x, y, z, u, v, w = _config(n, dtype)
    keep, (xd, yd, zd) = _dev((x, y, z), dtype)
    gb, g = _out3(n, dtype)
    dzo.pairwise_radial_gradient_(*g, xd, yd, zd)
    got = gb.to_host().reshape(3, n)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.random.default_rng(7).choice(n, 512, replace=False)]))
    exact, S, Sc = tw.gradient(x, y, z, rows=rows)
    _check_rows("gradient(rows)", n, dtype, got[:, rows], exact, S, Sc)
    e = dzo.pairwise_radial_energy(xd, yd, zd)
    E, SE = tw.energy_blockwise_f64(x, y, z)      # this twin sums in fp64: twice the bound
    bound = 2 * float(LD(n + 32) * U[np.dtype(dtype)] * LD(SE))
    print(f"energy N={n} {np.dtype(dtype).name}: error / bound = {abs(e - E) / bound:.4f}")
    assert abs(e - E) <= bound, (e, E, bound)


# ------------------------------------------------------------------------------ 3. semantics
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", NS + [N_SPLIT])
def test_same_input_same_bits(n, dtype):
    a = _gpu_all(n, dtype)
    b = _gpu_all(n, dtype)
    assert np.float64(a[0]).view(np.int64) == np.float64(b[0]).view(np.int64)
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    x, y, z = _config(n, dtype)[:3]
    keep, (xd, yd, zd) = _dev((x, y, z), dtype)
    i = n // 2
    d = [dzo.pairwise_radial_energy_delta(xd, yd, zd, i, x[i] + 0.03, y[i] - 0.02, z[i] + 0.01) for _ in range(2)]
    assert np.float64(d[0]).view(np.int64) == np.float64(d[1]).view(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [38, 257, 4099])
def test_views_at_odd_element_offsets(n, dtype):
    cfg = _config(n, dtype)
    stride = n + 2 if n % 2 == 0 else n + 1                         # even: odd + k * even stays odd
    big = np.zeros(6 * stride + 3, dtype=dtype)
    for k, a in enumerate(cfg):
        big[1 + k * stride: 1 + k * stride + n] = a
    buf = dzo.DeviceArray.from_host(big)
    views = [buf.view(1 + k * stride, n) for k in range(6)]
    assert all(((vv.ptr - buf.ptr) // np.dtype(dtype).itemsize) % 2 == 1 for vv in views)
    x, y, z, u, v, w = views
    out = dzo.DeviceArray.zeros(3 * stride + 3, dtype)
    o = [out.view(1 + k * stride, n) for k in range(3)]
    twin = _twin(n, dtype)
    e = dzo.pairwise_radial_energy(x, y, z)
    _check_rows("energy(odd)", n, dtype, np.array([e]), np.array([twin["energy"][0]], dtype=LD), np.array([twin["energy"][1]], dtype=LD))
    dzo.pairwise_radial_gradient_(*o, x, y, z)
    h = out.to_host()
    _check_rows("gradient(odd)", n, dtype, np.stack([h[1 + k * stride: 1 + k * stride + n] for k in range(3)]), *twin["gradient"])
    dzo.pairwise_radial_hvp_(*o, x, y, z, u, v, w)
    h = out.to_host()
    _check_rows("hvp(odd)", n, dtype, np.stack([h[1 + k * stride: 1 + k * stride + n] for k in range(3)]), *twin["hvp"])
    assert h[0] == 0 and not h[1 + n: 1 + stride].any()             # nothing written outside the views


@pytest.mark.parametrize("dtype", DTYPES)
def test_coincident_particles(dtype):
    x, y, z = (a.copy() for a in _config(38, dtype)[:3])
    x[7], y[7], z[7] = x[5], y[5], z[5]
    keep, (xd, yd, zd) = _dev((x, y, z), dtype)
    e = dzo.pairwise_radial_energy(xd, yd, zd)
    E, _ = tw.energy(x, y, z)
    assert not np.isfinite(e) and not np.isfinite(float(E))
    assert np.isnan(e) == np.isnan(float(E))
    gb, g = _out3(38, dtype)
    dzo.pairwise_radial_gradient_(*g, xd, yd, zd)
    got = gb.to_host().reshape(3, 38)
    others = [k for k in range(38) if k not in (5, 7)]
    assert np.all(np.isfinite(got[:, others]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [38, 4099])
def test_energy_delta(n, dtype):
    x, y, z = _config(n, dtype)[:3]
    keep, (xd, yd, zd) = _dev((x, y, z), dtype)
    rng = np.random.default_rng(n)
    worst = 0.0
    for _ in range(50):
        i = int(rng.integers(n))
        new = [float(np.asarray(c[i] + rng.uniform(-0.1, 0.1), dtype)) for c in (x, y, z)]
        got = dzo.pairwise_radial_energy_delta(xd, yd, zd, i, *new)
        want, S = tw.energy_delta(x, y, z, i, *new)
        bound = LD(n + 32) * U[np.dtype(dtype)] * S
        worst = max(worst, float(abs(LD(got) - want) / bound))
        assert abs(LD(got) - want) <= bound, (i, got, float(want), float(bound))
    print(f"energy_delta N={n} {np.dtype(dtype).name}: worst error / bound = {worst:.4f}")


def test_error_codes():
    n = 38
    x, y, z = _config(n, np.float64)[:3]
    keep, (xd, yd, zd) = _dev((x, y, z), np.float64)
    gb, g = _out3(n, np.float64)
    L = dzo.lib()
    import ctypes as C
    r = C.c_double()
    args = (n, dzo.F64, xd.ptr, yd.ptr, zd.ptr)
    assert L.dzo_pairwise_energy(7, *args, C.byref(r)) == 1                                    # unknown radial
    assert L.dzo_pairwise_gradient(7, n, dzo.F64, g[0].ptr, g[1].ptr, g[2].ptr, xd.ptr, yd.ptr, zd.ptr) == 1
    assert L.dzo_pairwise_hvp(7, n, dzo.F64, g[0].ptr, g[1].ptr, g[2].ptr, xd.ptr, yd.ptr, zd.ptr, xd.ptr, yd.ptr, zd.ptr) == 1
    assert L.dzo_pairwise_energy_delta(7, *args, 0, 0.0, 0.0, 0.0, C.byref(r)) == 1
    assert L.dzo_pairwise_energy_delta(0, *args, n, 0.0, 0.0, 0.0, C.byref(r)) == 1            # i = N
    assert L.dzo_pairwise_energy_delta(0, *args, -1, 0.0, 0.0, 0.0, C.byref(r)) == 1
    assert L.dzo_pairwise_energy_delta(0, *args, n - 1, 0.0, 0.0, 0.0, C.byref(r)) == 0
    assert L.dzo_pairwise_energy(0, n, dzo.F64, xd.ptr, None, zd.ptr, C.byref(r)) == 1         # null pointer
    assert L.dzo_pairwise_energy(0, *args, None) == 1
    assert L.dzo_pairwise_gradient(0, n, dzo.F64, None, g[1].ptr, g[2].ptr, xd.ptr, yd.ptr, zd.ptr) == 1
    assert L.dzo_pairwise_energy(0, 0, dzo.F64, xd.ptr, yd.ptr, zd.ptr, C.byref(r)) == 1       # no particles
    host = np.ascontiguousarray(y)                                                             # a host pointer
    assert L.dzo_pairwise_energy(0, n, dzo.F64, xd.ptr, host.ctypes.data, zd.ptr, C.byref(r)) == 3
    assert L.dzo_pairwise_gradient(0, n, dzo.F64, g[0].ptr, g[1].ptr, g[2].ptr, xd.ptr, yd.ptr, host.ctypes.data) == 3
    assert L.dzo_pairwise_hvp(0, n, dzo.F64, g[0].ptr, g[1].ptr, g[2].ptr, xd.ptr, yd.ptr, zd.ptr, host.ctypes.data, yd.ptr, zd.ptr) == 3
    with pytest.raises(dzo.AssertionFailed):
        dzo.pairwise_radial_energy(xd, dzo.DeviceArray(n, np.float64, ptr=host.ctypes.data, owner=False), zd)
    with pytest.raises(dzo.DzoError) as err:
        dzo.Problem(dzo.PAIRWISE_LJ, 7)
    assert err.value.code == 1
    prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
    with pytest.raises(dzo.DzoError) as err:
        dzo.BatchedBFGS(prob, np.zeros((4, 3 * n)), 1.0)
    assert err.value.code == 5
    h = C.c_void_p()
    x0 = dzo.DeviceArray.zeros(4 * 3 * n)
    assert L.dzo_bfgs_batch_create_problem(prob.h, 4, x0.ptr, 1.0, -1, C.byref(h)) == 5
    assert L.dzo_bfgs_batch_create(dzo.PAIRWISE_LJ, 4, 3 * n, dzo.F64, x0.ptr, 1.0, C.byref(h)) == 5


# ------------------------------------------------------------------------------ 4. the problem kind
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [38, 257, 4099])
def test_problem_kind(n, dtype):
    x, y, z = _config(n, dtype)[:3]
    buf, (xd, yd, zd) = _dev((x, y, z), dtype)
    prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n, dtype)
    e = dzo.pairwise_radial_energy(xd, yd, zd)
    f = prob(buf)
    assert np.float64(f).view(np.int64) == np.float64(np.dtype(dtype).type(e)).view(np.int64)
    gb, g = _out3(n, dtype)
    dzo.pairwise_radial_gradient_(*g, xd, yd, zd)
    pg = dzo.DeviceArray.zeros(3 * n, dtype)
    prob.gradient_(pg, buf)
    g_plain = gb.to_host()
    assert np.array_equal(_bits(pg.to_host()), _bits(g_plain))
    # decorators on top: L2 wrappers (legacy :231-232, :247) and the box gradient (:289-294)
    allc = np.concatenate([x, y, z])
    lam, lo, hi = 0.01, float(np.quantile(allc, 0.05)), float(np.quantile(allc, 0.95))   # a tenth of the coordinates on or beyond a bound
    clamped = dzo.DeviceArray.from_host(allc, dtype=dtype)
    xc = clamped.to_host()
    dec = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n, dtype, l2=lam, box_gradient=(lo, hi))
    f_plain, f_dec = prob(clamped), dec(clamped)
    ss = dzo.norm2(clamped)
    t = np.dtype(dtype).type
    want = float(t(f_plain) + t(lam) * t(ss))
    if np.isfinite(f_plain):
        assert abs(f_dec - want) <= 4 * float(U[np.dtype(dtype)]) * (abs(f_plain) + lam * ss) * (1 + 3 * n * float(U[np.dtype(np.float64)])), (f_dec, want)
    prob.gradient_(pg, clamped)
    dzo.axpy_(float(t(lam) + t(lam)), clamped, pg)              # g += 2 lambda x with the L1 entry point
    gw = pg.to_host()
    lo_t, hi_t = t(lo), t(hi)
    gw[((xc <= lo_t) & (gw >= 0)) | ((xc >= hi_t) & (gw <= 0))] = 0
    gd = dzo.DeviceArray.zeros(3 * n, dtype)
    dec.gradient_(gd, clamped)
    assert np.array_equal(gd.to_host(), gw)
    assert (gw == 0).sum() > 0


# ------------------------------------------------------------------------------ 5. the optimizers
def _start(name, seed, dtype=np.float64):
    base = tw.icosahedron13() if name == "ico" else tw.octahedron38()
    return np.asarray(np.concatenate(tw.jittered(base, seed)), dtype=dtype)


def _make(kind, prob, x0, via="problem"):
    obj = prob if via == "problem" else prob.native_callbacks()
    if kind == "lbfgs":
        return dzo.LBFGSOptimizer(None, obj, None, dzo.DeviceArray.from_host(x0), 0.01, 10)
    if kind == "bfgs":
        return dzo.BFGSOptimizer(prob, None, dzo.DeviceArray.from_host(x0), 0.01)
    if kind == "gd":
        return dzo.GradientDescentOptimizer(prob, None, None, dzo.DeviceArray.from_host(x0), 0.01)
    return dzo.AdGDOptimizer(None, prob, None, dzo.DeviceArray.from_host(x0), 0.01)


def _run_with_invariants(kind, opt, prob, max_steps, monotone):
    """step!() up to max_steps or the termination flag; after every one of the first 50 steps and every 25th after them the
    invariants of run_and_test! (the step before each of those is read too, for the deltas).  Returns the last value."""
    n, dtype = opt.n, opt.dtype
    scratch_x, scratch_g = dzo.DeviceArray(n, dtype), dzo.DeviceArray(n, dtype)

    def snapshot():
        return opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value

    def consistent(x, g, f, k):
        scratch_x.upload(x)
        fx = prob(scratch_x)
        assert np.float64(fx).view(np.int64) == np.float64(f).view(np.int64), (kind, k, f, fx)
        prob.gradient_(scratch_g, scratch_x)
        assert np.array_equal(_bits(scratch_g.to_host()), _bits(g)), (kind, k)

    prev = snapshot()
    consistent(*prev, 0)
    prev_k, f_last, k = 0, prev[2], 0
    while k < max_steps and not opt.is_stuck:
        opt.step()
        k += 1
        f = opt.current_objective_value
        if monotone:
            assert f <= f_last, (kind, k, f, f_last)
        f_last = f
        check = k <= 50 or k % 25 == 0
        if check or k % 25 == 24:
            cur = snapshot()
            if check:
                consistent(*cur, k)
                if prev_k == k - 1 and not opt.is_stuck:
                    assert np.array_equal(opt.delta_point.to_host(), cur[0] - prev[0]), (kind, k, "delta_point")
                    assert np.array_equal(opt.delta_gradient.to_host(), cur[1] - prev[1]), (kind, k, "delta_gradient")
                if prev_k == k - 1 and opt.is_stuck:
                    assert np.array_equal(cur[0], prev[0]) and np.array_equal(cur[1], prev[1]), (kind, k, "terminated step moved")
            prev, prev_k = cur, k
    return f_last, k, opt.is_stuck


CASES = [("lbfgs", "problem"), ("lbfgs", "native_callbacks"), ("bfgs", "problem"), ("gd", "problem"), ("adgd", "problem")]


@pytest.mark.parametrize("name,lit", [("ico", tw.LJ13), ("oct", tw.LJ38)])
@pytest.mark.parametrize("kind,via", CASES)
def test_optimizers_relax_the_clusters(kind, via, name, lit):
    for seed in range(5):
        x0 = _start(name, seed)
        prob = dzo.Problem(dzo.PAIRWISE_LJ, x0.size)
        opt = _make(kind, prob, x0, via)
        f, steps, flag = _run_with_invariants(kind, opt, prob, 2000, monotone=(kind == "lbfgs"))
        print(f"{kind}/{via} {name} seed {seed}: f = {f:.9f} after {steps} steps, terminated = {flag}")
        if kind in ("lbfgs", "bfgs"):
            assert abs(f - lit) <= 5e-7, (kind, via, name, seed, f, lit)


@pytest.mark.parametrize("via", ["problem", "native_callbacks"])
def test_lbfgs_large_lattice(via):
    n = 4096
    x0 = np.concatenate(tw.lattice(n, seed=1))
    prob = dzo.Problem(dzo.PAIRWISE_LJ, 3 * n)
    opt = _make("lbfgs", prob, x0, via)
    f, steps, _ = _run_with_invariants("lbfgs", opt, prob, 40, monotone=True)
    assert steps == 40
    p = opt.current_point.to_host()
    E, S = tw.energy(p[:n], p[n:2 * n], p[2 * n:])
    bound = LD(n + 32) * U[np.dtype(np.float64)] * S
    print(f"lbfgs/{via} lattice N={n}: f = {f:.6f} after {steps} steps, error / bound = {float(abs(LD(f) - E) / bound):.4f}")
    assert abs(LD(f) - E) <= bound


@pytest.mark.parametrize("via", ["problem", "native_callbacks"])
def test_lbfgs_fp32_invariants(via):
    x0 = _start("oct", 0, np.float32)
    prob = dzo.Problem(dzo.PAIRWISE_LJ, x0.size, np.float32)
    opt = _make("lbfgs", prob, x0, via)
    f, steps, flag = _run_with_invariants("lbfgs", opt, prob, 20, monotone=True)
    print(f"lbfgs/{via} fp32 oct: f = {f:.6f} after {steps} steps, terminated = {flag}")
    assert np.isfinite(f)


# ------------------------------------------------------------------------------ 6. the plain-C example
def test_lj_cluster_example_runs(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_cluster")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_cluster.c"),
                    "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
