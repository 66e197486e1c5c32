"""The one bit every non-batched optimizer ends on -- "did the trial point differ from the old point anywhere" -- and its
relatives (the host-write check of the point ring, the dense searches' "direction is not zero"), when ONE element differs, at
every seam of the kernel that raises the flag.  All of them go through block_raise_flag (csrc/dzo_common.h).

Probes (tests/test_vec_twin.py asserts what is said here on the CPU oracle, for every (n, p) used):

* window: chained Rosenbrock (or the chained quadratic) at its minimiser x = 1 with x[p] += 1e-3.  The gradient is non-zero
  exactly on {p - 1, p, p + 1}; a step moves exactly those elements, after several halvings on Rosenbrock; every further step
  moves elements of a window one element wider on each side;
* one-hot: log-sum-exp with c = 0, lambda = 0 at x = -800, x[p] = 0: the gradient is exactly e_p, a step moves element p alone
  (one step: the next gradient is e_p again, so y = 0 and the reference's recurrence has no direction);
* stuck: x = 1, zero gradient: stuck from construction, and a step changes no byte of x.

Sizes and positions come from tests/vec_twin.py: flag_sizes() (1 .. 2 * 1024 N + 1 and 100 003; N = 2 fp64 / 4 fp32 elements
per 16-byte vector) with positions(), extended by the seams of the fused passes' rows (row_positions()): csrc/dzo_lbfgs_plan.h
gives a wave kRowOwn = 62 own vectors per wave-row and a block four rows, so 62 N - 1 | 62 N is the first boundary between two
waves and 4 * 62 N - 1 | 4 * 62 N the first between two blocks; a ragged n has its last, partial vector on the point ring
only.  The passes that take whole vectors (pair ring, fused AdGD) run whole_vector_sizes().  The chained Rosenbrock function
needs two elements, the tile rings 4 N.

The L-BFGS device optimizer runs free and the oracle follows it (the protocol of
test_point_ring_steps_match_the_oracle_from_the_same_state): before every step the oracle is given the device's point,
gradient, objective value and history.  After every step: is_stuck and last_trials are the oracle's, the SET of indices at which
current_point changed is the oracle's, and the point has the oracle's bits wherever the two directions have the same bits (the
trial point is elementwise: fma(t, d, x)), and agrees within the same-state tests' tolerance otherwise.

a. trial_kernel<VEC, FIRST> through the split entry points;  b. two-pass L-BFGS (trial_kernel inside step!(), and
rosen_trial_eval_kernel under DZO_TUNE_FUSED_TRIAL=1);  c. lbfgs_single_pass_kernel (pair ring);  d. lbfgs_point_pass_kernel
and lse_trial_kernel (point ring);  e. adgd_fused_rosen_kernel;  f. phi_point_kernel (dense BFGS, gradient descent; both
flags);  g. ring_compare_kernel (one element written by the host);  h. the stuck probe, inside each of them.
"""
import functools

import numpy as np
import pytest

import vec_twin as vt
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
CANARY = 12345.0
GUARD = 64
M = 3
STEPS = 3


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _moved(after, before):
    return np.flatnonzero(vt.bits(after) != vt.bits(before)).tolist()


def _problems(kind, n, dt):
    if kind == "lse":
        c = np.zeros(n, dt)
        return orc.Problem(orc.LSE, n, dt, c=c, lam=0.0), dzo.Problem(dzo.LSE, n, dt, c=c, lam=0.0)
    if kind == "qchain":
        return orc.Problem(orc.QUADRATIC_CHAIN, n, dt, lam=0.05), dzo.Problem(dzo.QUADRATIC_CHAIN, n, dt, lam=0.05)
    return orc.Problem(orc.ROSENBROCK_CHAIN, n, dt), dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt)


def _wide_sums(fn):
    """fp32 runs of the oracle sum in fp64, as the device does."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        orc.set_dot_mode(orc.DOT_WIDE)
        try:
            return fn(*args, **kwargs)
        finally:
            orc.set_dot_mode(orc.DOT_SEQUENTIAL)
    return wrapped


# ------------------------------------------------------------------------------ L-BFGS: paths b, c, d (and h)
def _expected_layout(path, n, dt):
    N = vt.vec_n(dt)
    if path in ("two_pass", "two_pass_fused") or n < 4 * N:
        return 0
    if path == "pairs":
        return 1 if n % N == 0 else 0
    return 2


def _lbfgs_follow(kind, path, n, dt, x0, steps, what):
    """The device optimizer from x0, the oracle following it; the assertions of the module docstring after every step."""
    ref_p, dev_p = _problems(kind, n, dt)
    ref = orc.LBFGS(ref_p, x0.copy(), 1.0, M)
    opt = dzo.LBFGSOptimizer(None, dev_p, None, dzo.DeviceArray.from_host(x0), 1.0, M)
    layout = _expected_layout(path, n, dt)
    assert opt.ring_layout == layout, what
    assert opt.is_stuck == ref.is_stuck, what
    tol_x = 1e-12 if dt == np.float64 else 1e-6
    widened = []
    for it in range(steps):
        k = opt.history_count
        S = np.stack([h.to_host() for h in opt.delta_point_history]) if k else np.zeros((0, n), dt)
        Y = np.stack([h.to_host() for h in opt.delta_gradient_history]) if k else np.zeros((0, n), dt)
        x, g = opt.current_point.to_host(), opt.current_gradient.to_host()
        ref.install_state(x, g, opt.current_objective_value, S, Y, opt.rho_history[:k], opt.iteration_count)
        opt.step(); ref.step()
        tag = (what, "step", it)
        assert opt.ring_layout == layout, tag
        assert opt.is_stuck == ref.is_stuck, tag
        assert opt.last_trials == ref.last_trials, (tag, opt.last_trials, ref.last_trials)
        x_new = opt.current_point.to_host()
        assert _moved(x_new, x) == _moved(ref.current_point, x), tag
        d_dev, d_ref = opt.step_direction.to_host(), np.array(ref.step_direction)
        if np.array_equal(vt.bits(d_dev), vt.bits(d_ref)):
            assert np.array_equal(vt.bits(x_new), vt.bits(ref.current_point)), tag
        else:
            assert rel(d_dev, d_ref) <= (1e-10 if dt == np.float64 else 2e-4), tag
            assert rel(x_new, ref.current_point) <= tol_x, tag
        widened.append(_moved(x_new, x))
        if ref.is_stuck:
            break
    return opt, ref, widened


def _set_path(path, monkeypatch):
    if path in ("two_pass", "two_pass_fused"):
        monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", "0")
    monkeypatch.setenv("DZO_TUNE_FUSED_TRIAL", "1" if path == "two_pass_fused" else "0")
    if path == "pairs":
        monkeypatch.setenv("DZO_TUNE_POINT_RING", "0")


def _lbfgs_cases():
    out = []
    for d in DTYPES:
        for path, kinds in (("two_pass", ("rosen", "qchain")), ("two_pass_fused", ("rosen",)), ("pairs", ("rosen",)),
                            ("points", ("rosen", "qchain"))):
            sizes = vt.whole_vector_sizes(d) if path == "pairs" else vt.flag_sizes(d)
            out += [pytest.param(path, kind, d, n, id="%s-%s-%s-n%d" % (path, kind, d, n)) for kind in kinds for n in sizes if n >= 2]
    return out


@pytest.mark.parametrize("path,kind,dtype,n", _lbfgs_cases())
@_wide_sums
def test_lbfgs_steps_that_move_a_window_of_elements(path, kind, dtype, n, monkeypatch):
    """Paths b, c, d with the window probe, three steps: {p - 1, p, p + 1}, then a window one element wider per step; and the
    stuck probe (h)."""
    dt = np.dtype(dtype)
    _set_path(path, monkeypatch)
    for p in vt.row_positions(n, dt):
        opt, ref, widened = _lbfgs_follow(kind, path, n, dt, vt.window_start(n, p, dt), STEPS, (path, kind, dtype, n, p))
        assert not opt.is_stuck and len(widened) == STEPS
        assert widened[0] == vt.window(n, p), (p, widened[0])
        for it, moved in enumerate(widened):                     # (equal to the oracle's sets already)
            assert moved and set(moved) <= set(vt.window(n, p, it + 1)), (p, it, moved)
        assert opt.iteration_count == STEPS
        if path == "points" and opt.ring_layout == 2 or path == "pairs":
            # every step was one pass (the pair ring's first step has no pair to pass over: the two-pass kernels take it)
            assert opt.single_pass_steps == (STEPS if path == "points" else STEPS - 1), (p, opt.single_pass_steps)
    # stuck: zero gradient at x = 1
    ones = np.ones(n, dt)
    opt, ref, widened = _lbfgs_follow(kind, path, n, dt, ones, 1, (path, kind, dtype, n, "stuck"))
    assert opt.is_stuck and ref.is_stuck and widened == [[]]
    assert np.array_equal(vt.bits(opt.current_point.to_host()), vt.bits(ones)) and opt.iteration_count == 0


@pytest.mark.parametrize("path,kernel,other", [("two_pass", "lbfgs_trial", "lbfgs_trial_objective"), ("two_pass_fused", "lbfgs_trial_objective", "lbfgs_trial")])
@_wide_sums
def test_the_two_pass_paths_launch_the_trial_kernel_they_are_selected_for(path, kernel, other, monkeypatch):
    """The other paths count their steps (single_pass_steps, fused_steps, host_write_checks); these two are told apart by the
    library's own launch table: trial_kernel is timed as lbfgs_trial, rosen_trial_eval_kernel as lbfgs_trial_objective."""
    dt = np.dtype("float64")
    n, p = 1024 * 2 + 3, 1024 * 2 + 2
    _set_path(path, monkeypatch)
    dzo.profile_enable(2)
    try:
        dzo.profile_reset()
        opt, ref, widened = _lbfgs_follow("rosen", path, n, dt, vt.window_start(n, p, dt), 1, (path, n, p))
        dzo.synchronize()
        table = dzo.profile_table()
    finally:
        dzo.profile_enable(0)
        dzo.profile_reset()
    assert ref.last_trials >= 2 and widened == [vt.window(n, p)]
    assert table.get(kernel, (0, 0.0))[0] == ref.last_trials and other not in table, sorted(table)


def _lse_cases():
    return [pytest.param(path, d, n, id="%s-%s-n%d" % (path, d, n)) for d in DTYPES for path in ("two_pass", "points") for n in vt.flag_sizes(d)]


@pytest.mark.parametrize("path,dtype,n", _lse_cases())
@_wide_sums
def test_lbfgs_step_that_moves_one_element(path, dtype, n, monkeypatch):
    """The one-hot probe on the log-sum-exp paths: lse_trial_kernel on the point ring (d), trial_kernel on the slabs (b)."""
    dt = np.dtype(dtype)
    _set_path(path, monkeypatch)
    for p in vt.row_positions(n, dt):
        x0 = vt.one_hot_start(n, p, dt)
        opt, ref, widened = _lbfgs_follow("lse", path, n, dt, x0, 1, (path, "lse", dtype, n, p))
        assert not opt.is_stuck and widened == [[p]], (p, widened)
        e_p = np.zeros(n, dt); e_p[p] = 1.0
        assert np.array_equal(opt.current_gradient.to_host(), e_p), p
        assert np.array_equal(vt.bits(opt.current_point.to_host()), vt.bits(ref.current_point)), p    # d = -e_p on both sides
        if opt.ring_layout == 2:
            assert opt.single_pass_steps == 1


# ------------------------------------------------------------------------------ a. trial_kernel, all four instantiations
class _GuardedPoint:
    """The optimizer's aliased point inside a canary-filled allocation, `off` elements off the 16-byte grid."""

    def __init__(self, n, dt, off):
        self.n, self.lo = n, GUARD + off
        self.buf = dzo.DeviceArray.from_host(np.full(self.lo + n + GUARD, CANARY, dt))
        assert self.buf.ptr % 16 == 0
        self.dev = self.buf.view(self.lo, n)

    def read(self):
        h = self.buf.to_host()
        c = h.dtype.type(CANARY)
        assert np.all(h[:self.lo] == c) and np.all(h[self.lo + self.n:] == c), "the trial wrote outside the point"
        return h[self.lo:self.lo + self.n]


@pytest.mark.parametrize("off", [0, 1], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype,n", [pytest.param(d, n, id="%s-n%d" % (d, n)) for d in DTYPES for n in vt.flag_sizes(d)])
def test_trial_kernel_sees_one_moved_element(dtype, n, off):
    """A callback handle (no built-in problem: every trial is trial_kernel), the direction uploaded as test_stuck_semantics
    does, begin_search(), trial(t) (FIRST: reads x, saves it), trial(t / 2) (reads the saved point).  x aligned: the VEC
    instantiations, where the elements past the last whole vector are the tail; x one element off: the scalar ones.
    d = v e_p: True, x = fma(t, d, x_old) bit for bit; d = 0, or |t v| below half an ulp of x[p]: False, x keeps its bytes."""
    dt = np.dtype(dtype)
    T = dt.type
    rng = np.random.default_rng(n + off)
    x0 = rng.standard_normal(n).astype(dt)
    X = _GuardedPoint(n, dt, off)
    X.dev.upload(x0)
    g = dzo.DeviceArray.zeros(n, dt)
    opt = dzo.LBFGSOptimizer(None, lambda x_: 0.0, lambda g_, x_: None, X.dev, 0.0, g, 1.0, M)
    assert opt.current_point.ptr == X.dev.ptr and (X.dev.ptr % 16 == 0) == (off == 0)
    t, v = 0.75, T(1.25)
    d = np.zeros(n, dt)
    for p in vt.positions(n, dt):
        # the direction is zero: nothing changes, in either instantiation
        opt.step_direction.upload(d)
        opt.begin_search()
        assert not opt.trial(t), ("zero, first", p)
        assert np.array_equal(vt.bits(X.read()), vt.bits(x0))
        assert not opt.trial(t / 2), ("zero, later", p)
        assert np.array_equal(vt.bits(X.read()), vt.bits(x0))
        # one element of the direction is not
        d[p] = v
        opt.step_direction.upload(d)
        opt.begin_search()
        assert opt.trial(t), ("one element, first", p)
        assert np.array_equal(vt.bits(X.read()), vt.bits(vt.trial_point(t, d, x0))), p
        assert _moved(X.read(), x0) == [p]
        assert np.array_equal(vt.bits(opt.delta_point.to_host()), vt.bits(x0))               # :118, the saved point
        assert opt.trial(t / 2), ("one element, later", p)
        assert np.array_equal(vt.bits(X.read()), vt.bits(vt.trial_point(t / 2, d, x0))), p
        opt.reject()
        dzo.synchronize()
        assert np.array_equal(vt.bits(X.read()), vt.bits(x0)), p
        # ... but too small to move x[p] = 1: |t v| = 2^-60 (2^-30 in fp32) is below half an ulp on either side of 1
        x1 = x0.copy(); x1[p] = 1.0
        X.dev.upload(x1)
        d[p] = T(2.0 ** (-60 if dt == np.float64 else -30))
        for sign in (1.0, -1.0):
            opt.step_direction.upload(T(sign) * d)
            opt.begin_search()
            assert not opt.trial(1.0), ("below half an ulp, first", p, sign)
            assert np.array_equal(vt.bits(X.read()), vt.bits(x1))
            assert not opt.trial(0.5), ("below half an ulp, later", p, sign)
            assert np.array_equal(vt.bits(X.read()), vt.bits(x1))
        X.dev.upload(x0)
        d[p] = 0


# ------------------------------------------------------------------------------ e. AdGD
def _adgd_cases():
    return [pytest.param(d, n, id="%s-n%d" % (d, n)) for d in DTYPES for n in sorted(set(vt.whole_vector_sizes(d) + vt.flag_sizes(d))) if n >= 2]


@pytest.mark.parametrize("dtype,n", _adgd_cases())
@_wide_sums
def test_adgd_steps_that_move_a_window_of_elements(dtype, n):
    """adgd_fused_rosen_kernel (whole vectors, from 4 N elements on) and the generic kernels (every other n) against orc.AdGD,
    both free from the same start, as test_adgd_matches_oracle runs them."""
    dt = np.dtype(dtype)
    N = vt.vec_n(dt)
    fused = n % N == 0 and n >= 4 * N
    tol = 1e-10 if dt == np.float64 else 1e-5
    for p in vt.row_positions(n, dt):
        x0 = vt.window_start(n, p, dt)
        ref = orc.AdGD(orc.Problem(orc.ROSENBROCK_CHAIN, n, dt), x0.copy(), 0.1)
        opt = dzo.AdGDOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt), None, dzo.DeviceArray.from_host(x0), 0.1)
        assert opt.is_stuck == ref.is_stuck
        x = x0
        for it in range(STEPS):
            x_ref = np.array(ref.current_point)
            opt.step(); ref.step()
            assert opt.is_stuck == ref.is_stuck and opt.iteration_count == ref.iteration_count, (p, it)
            x_new = opt.current_point.to_host()
            moved = _moved(x_new, x)
            assert moved == _moved(ref.current_point, x_ref) and moved and set(moved) <= set(vt.window(n, p, it + 1)), (p, it, moved)
            assert it > 0 or moved == vt.window(n, p), (p, moved)
            assert rel(x_new, ref.current_point) <= tol, (p, it)
            x = x_new
        assert opt.fused_steps == (STEPS if fused else 0), (p, opt.fused_steps)
    ones = np.ones(n, dt)
    ref = orc.AdGD(orc.Problem(orc.ROSENBROCK_CHAIN, n, dt), ones.copy(), 0.1)
    opt = dzo.AdGDOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt), None, dzo.DeviceArray.from_host(ones), 0.1)
    assert opt.is_stuck == ref.is_stuck
    opt.step(); ref.step()
    assert opt.is_stuck and ref.is_stuck and opt.iteration_count == ref.iteration_count
    assert np.array_equal(vt.bits(opt.current_point.to_host()), vt.bits(ones))


# ------------------------------------------------------------------------------ f. dense BFGS and gradient descent
def _dense_cases():
    return [pytest.param(cls, d, n, id="%s-%s-n%d" % (cls, d, n)) for cls in ("bfgs", "gd") for d in DTYPES for n in vt.flag_sizes(d) if n <= 1025]


def _dense_pair(cls, kind, n, dt, x0):
    ref_p, dev_p = _problems(kind, n, dt)
    if cls == "bfgs":
        return orc.BFGS(ref_p, x0.copy(), 1.0), dzo.BFGSOptimizer(dev_p, None, dzo.DeviceArray.from_host(x0), 1.0)
    return orc.GradientDescent(ref_p, x0.copy(), 1.0), dzo.GradientDescentOptimizer(dev_p, None, None, dzo.DeviceArray.from_host(x0), 1.0)


@pytest.mark.parametrize("cls,dtype,n", _dense_cases())
@_wide_sums
def test_dense_searches_see_one_element(cls, dtype, n):
    """phi_point_kernel raises two flags: the point changed, and the direction is not zero.  One-hot probe: the direction is
    non-zero at p alone and must not be called zero; window probe: three steps; stuck probe: the zero direction reports what
    the oracle reports."""
    dt = np.dtype(dtype)
    tol = 1e-9 if dt == np.float64 else 1e-4
    for p in vt.positions(n, dt):
        x0 = vt.one_hot_start(n, p, dt)
        ref, opt = _dense_pair(cls, "lse", n, dt, x0)
        # (f falls without bound along -e_p: uncapped, the bracket doubles until the arithmetic overflows, and there the
        # oracle's extended-precision sum of squares and the device's fp64 one differ; QuadraticLineSearch.max_increases
        # (legacy :181-188) ends it at 2^8)
        opt.set_max_increases(8); ref.set_max_increases(8)
        opt.step(); ref.step()
        assert opt.has_terminated == ref.has_terminated and not ref.has_terminated, p
        assert opt.iteration_count == ref.iteration_count == 1, p
        x_new = opt.current_point.to_host()
        assert _moved(x_new, x0) == _moved(ref.current_point, x0) == [p], p
        assert rel(x_new, ref.current_point) <= tol, p
        if n < 2:
            continue
        x0 = vt.window_start(n, p, dt)
        ref, opt = _dense_pair(cls, "rosen", n, dt, x0)
        x = x0
        for it in range(STEPS):
            x_ref = np.array(ref.current_point)
            opt.step(); ref.step()
            assert opt.has_terminated == ref.has_terminated and opt.iteration_count == ref.iteration_count, (p, it)
            x_new = opt.current_point.to_host()
            assert _moved(x_new, x) == _moved(ref.current_point, x_ref), (p, it)
            assert it > 0 or _moved(x_new, x0) == vt.window(n, p), p     # the first step walks along the gradient
            assert rel(x_new, ref.current_point) <= tol, (p, it)
            x = x_new
        assert not opt.has_terminated
    if n >= 2:
        ones = np.ones(n, dt)
        ref, opt = _dense_pair(cls, "rosen", n, dt, ones)
        assert opt.has_terminated == ref.has_terminated
        opt.step(); ref.step()
        assert opt.has_terminated == ref.has_terminated and ref.has_terminated and opt.iteration_count == ref.iteration_count
        assert np.array_equal(vt.bits(opt.current_point.to_host()), vt.bits(ones))


# ------------------------------------------------------------------------------ g. the host wrote one element
def _ring_sizes(dtype):
    N = vt.vec_n(dtype)
    return [1024 * N, 1024 * N + N + 1, vt.FLAG_LARGE]            # whole vectors; a full vector and a one-element tail; large and ragged


@pytest.mark.parametrize("written", ["point", "gradient"])
@pytest.mark.parametrize("dtype,n", [pytest.param(d, n, id="%s-n%d" % (d, n)) for d in DTYPES for n in _ring_sizes(d)])
@_wide_sums
def test_point_ring_notices_one_element_the_host_wrote(dtype, n, written):
    """test_point_ring_adopts_what_the_host_wrote_into_the_aliased_arrays with ONE element written (ring_compare_kernel: a
    vector per thread, 256 per block): x[p] moved by 1e-3 with g and f recomputed, or one element of current_gradient alone.
    The next step has left the point ring -- for the pair ring, or the slabs where n is ragged -- and matches the oracle from
    the written state; p runs over the point ring's seams, the last element of a ragged n included."""
    dt = np.dtype(dtype)
    T = dt.type
    x0 = orc.rosenbrock_chain_x0(n, dt)
    pr = orc.Problem(orc.ROSENBROCK_CHAIN, n, dt)
    xd = dzo.DeviceArray.from_host(x0)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt), None, xd, 1.0, M)
    for _ in range(M + 2):
        opt.step()
    assert opt.ring_layout == 2
    state = None
    for p in vt.row_positions(n, dt):
        if state is not None:
            # back to the same ring state: a fresh optimizer stepped to it (the written one has left the point ring)
            xd = dzo.DeviceArray.from_host(x0)
            opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dt), None, xd, 1.0, M)
            for _ in range(M + 2):
                opt.step()
        S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
        x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
        rho, its = opt.rho_history.copy(), opt.iteration_count
        if state is None:
            state = (x, g, f)
        assert np.array_equal(x, state[0]) and np.array_equal(g, state[1]) and opt.ring_layout == 2      # deterministic
        checks = opt.host_write_checks
        if written == "point":
            x_new = x.copy(); x_new[p] += T(1e-3)
            g_new, f_new = pr.grad(x_new), pr.eval(x_new)
            xd.view(p, 1).upload(x_new[p:p + 1])                 # one element, through the caller's own handle of the aliased array
            opt.current_gradient.upload(g_new)
            opt.set_objective_value(f_new)
        else:
            x_new, f_new = x, f
            g_new = g.copy(); g_new[p] += T(1000.0)             # (large: the direction changes by far more than the tolerance)
            gp = opt.current_gradient                            # the pointer hand-out after which the host may have written
            gp.view(p, 1).upload(g_new[p:p + 1])
        ref = orc.LBFGS(pr, x0.copy(), 1.0, M)
        ref.install_state(x_new, g_new, f_new, S, Y, rho, its)
        opt.step(); ref.step()
        assert opt.host_write_checks == checks + 1, p
        assert opt.ring_layout == (1 if n % vt.vec_n(dt) == 0 else 0), (p, opt.ring_layout)
        assert opt.is_stuck == ref.is_stuck and opt.last_trials == ref.last_trials and opt.iteration_count == ref.iteration_count, p
        assert rel(opt.step_direction.to_host(), ref.step_direction) <= (1e-10 if dt == np.float64 else 2e-4), p
        assert rel(opt.current_point.to_host(), ref.current_point) <= (1e-12 if dt == np.float64 else 1e-6), p
        assert np.array_equal(xd.to_host(), opt.current_point.to_host())
