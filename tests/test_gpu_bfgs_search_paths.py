"""The rare paths of the quadratic line search where they run on the device: wave 0 of the batched step kernel (csrc/dzo_batch.hip,
which keeps its own statement of the search) and the dense optimizer over callbacks with a constraint (csrc/dzo_bfgs.hip: the
sequential driver of csrc/dzo_phi_search.h over its evaluator; tests/test_phi_search.py decides every exit of that driver on the CPU
against the oracle).  Conventions of tests/test_gpu_bfgs_steps.py: the oracle's state installed, one step on both sides, _check_step.

Batched cases: three instances, the middle one in the special state, its neighbours in an ordinary one -- all three must step as
their oracles do.  n = 2 is one lane of the search wave, n = 66 one element past a full pass of its lane-strided loops.  In fp32
the oracle forms its dot products as the device does (a double sum rounded once), so decisions, point, value and step length are
compared bit for bit there; in fp64 _check_step's bounds apply."""
import ctypes as C

import numpy as np
import pytest

from dzo_loader import dzo
from oracle import oracle as orc
from test_gpu_bfgs_steps import _batch_read, _check_step, _oracle_state

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SHAPES = [(n, dt) for n in (2, 66) for dt in (F64, F32)]


def _matrix(n, dtype):
    """SPD, symmetric bit for bit, every row sum positive (so that A x < 0 elementwise for x = -c 1), exact in fp32."""
    A = np.full((n, n), 2.0 ** -6) + np.diag(1.0 + np.arange(n) % 5 / 4.0)
    return np.asfortranarray(A.astype(dtype))


def _step_and_compare(batch, refs, dtype, where):
    """install the oracles' states, one step on both sides, compare every instance; returns what the device holds"""
    st = [_oracle_state(r) for r in refs]
    batch.install_state(**{k: np.stack([s[k] for s in st]) if isinstance(st[0][k], np.ndarray) else [s[k] for s in st] for k in st[0]},
                        has_terminated=[0] * len(refs))
    f_before = [r.current_objective_value for r in refs]
    batch.step(1, poll=False)
    for r in refs:
        r.step()
    got = _batch_read(batch)
    for b, ref in enumerate(refs):
        one = {k: v[b] for k, v in got.items()}
        one["has_terminated"] = bool(one["has_terminated"])
        if dtype == F64:
            _check_step(one, ref, f_before[b], where + (b,))
        else:
            assert one["has_terminated"] == ref.has_terminated and int(one["last_step_type"]) == ref.last_step_type, where + (b,)
            assert one["iteration_count"] == ref.iteration_count, where + (b,)
            assert one["x"].tobytes() == ref.current_point.tobytes(), where + (b,)
            assert float(one["f"]) == float(ref.current_objective_value), where + (b,)
            if not ref.has_terminated:
                assert float(one["last_step_length"]) == float(ref.last_step_length), where + (b,)
    return got


def _oracles(n, dtype, problem_kw, X0, lengths, max_increases=0):
    """one oracle per instance of a shared dense quadratic, instance b started at X0[b] with last_step_length lengths[b]"""
    refs = [orc.BFGS(orc.Problem(orc.QUADRATIC, n, dtype, A=_matrix(n, dtype), **problem_kw), X0[b].copy(), float(lengths[b]))
            for b in range(len(X0))]
    for r in refs:
        r.set_max_increases(max_increases)
    return refs


def _case(n, dtype, problem_kw, X0, lengths, max_increases=0):
    """(batch, oracles)"""
    batch = dzo.BatchedBFGS(dzo.Problem(dzo.QUADRATIC, n, dtype=dtype, A=_matrix(n, dtype), **problem_kw), X0, 1.0)
    assert batch.dtype == np.dtype(dtype)
    batch.set_max_increases(max_increases)
    return batch, _oracles(n, dtype, problem_kw, X0, lengths, max_increases)


@pytest.fixture(autouse=True)
def _wide_dots():
    orc.set_dot_mode(orc.DOT_WIDE)                 # (fp32: the oracle's norms as the device forms them; fp64 is not affected by the bound)
    yield
    orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def _starts(n, dtype, seed):
    return np.stack([(orc.pcg_fill(n, seed + b) - 0.5).astype(dtype) for b in range(3)])


@pytest.mark.parametrize("n,dtype", SHAPES)
def test_batched_tiny_first_step_is_doubled_until_the_point_moves(n, dtype):
    """:91-101.  x scaled by 2^40, last_step_length 2^-30: the first trial point of both searches is x itself."""
    X0 = _starts(n, dtype, 300)
    X0[1] *= dtype(2.0 ** 40)
    batch, refs = _case(n, dtype, {}, X0, [1.0, 2.0 ** -30, 1.0])
    g = refs[1].current_gradient
    t0 = dtype(2.0 ** -30) / dtype(np.sqrt(np.sum(g.astype(F64) ** 2)))
    assert t0 > 0 and np.array_equal(X0[1] - t0 * g, X0[1])                 # the step is below half an ulp of every coordinate
    _step_and_compare(batch, refs, dtype, ("tiny", n, np.dtype(dtype).name))
    assert not refs[1].has_terminated and refs[1].iteration_count == 1      # ... and the search went on from a doubled step


@pytest.mark.parametrize("n,dtype", SHAPES)
def test_batched_tiny_step_clamped_back_to_x_terminates_the_instance(n, dtype):
    """:107-123.  Every coordinate on the upper bound and the gradient pointing outward: the first point that moves is clamped
    back to x, both searches return step 0, the instance terminates; its neighbours inside the box go on."""
    hi = 2.0 ** 40
    X0 = np.stack([(-hi * (1.5 + orc.pcg_fill(n, 310 + b))).astype(dtype) for b in range(3)])
    X0[1] = -hi
    batch, refs = _case(n, dtype, dict(box_constraint=(-4 * hi, -hi)), X0, [hi, 2.0 ** -30, hi])
    g = refs[1].current_gradient
    assert (g < 0).all()                                                    # x - t g leaves the box through the bound x lies on
    t0 = dtype(2.0 ** -30) / dtype(np.sqrt(np.sum(g.astype(F64) ** 2)))
    assert np.array_equal(X0[1] - t0 * g, X0[1])
    got = _step_and_compare(batch, refs, dtype, ("tiny clamped", n, np.dtype(dtype).name))
    assert refs[1].has_terminated and got["has_terminated"][1] and not refs[0].has_terminated and not refs[2].has_terminated
    assert got["x"][1].tobytes() == X0[1].tobytes()


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("n,dtype", SHAPES)
def test_batched_max_increases_stops_the_doubling(n, dtype, cap):
    """:147.  From a last_step_length 2^-12 of the natural one the gradient search doubles many times; the cap ends it after
    `cap` doublings (the oracle's evaluation count says so)."""
    X0 = _starts(n, dtype, 320)
    lengths = [1.0, 2.0 ** -12, 1.0]
    evals = {}
    for c in (0, 1, 2):
        probe = _oracles(n, dtype, {}, X0, lengths, max_increases=c)
        g = probe[1].current_gradient
        before = probe[1].objective_evaluations
        probe[1].line_search(True, float(dtype(lengths[1]) / dtype(np.sqrt(np.sum(g.astype(F64) ** 2)))))
        evals[c] = probe[1].objective_evaluations - before
    assert evals[0] >= 1 + 3 + 1 and evals[1] < evals[2] < evals[0], evals   # first point, at least three doublings, the parabola's point
    batch, refs = _case(n, dtype, {}, X0, lengths, max_increases=cap)
    _step_and_compare(batch, refs, dtype, ("max_increases", cap, n, np.dtype(dtype).name))
    assert not refs[1].has_terminated


@pytest.mark.parametrize("n,dtype", SHAPES)
def test_batched_halving_ten_times_and_more(n, dtype):
    """:157-171.  last_step_length 2^14 times too long: the oracle halves at least ten times before a point is below f0."""
    X0 = _starts(n, dtype, 330)
    lengths = [1.0, 2.0 ** 14, 1.0]
    probe = _oracles(n, dtype, {}, X0, lengths)
    g = probe[1].current_gradient
    t0 = float(dtype(lengths[1]) / dtype(np.sqrt(np.sum(g.astype(F64) ** 2))))
    before = probe[1].objective_evaluations
    t, _ = probe[1].line_search(True, t0)
    assert probe[1].objective_evaluations - before >= 11 and 0 < t <= t0 * 2.0 ** -9
    batch, refs = _case(n, dtype, {}, X0, lengths)
    _step_and_compare(batch, refs, dtype, ("halving", n, np.dtype(dtype).name))
    assert not refs[1].has_terminated


# ------------------------------------------------------------------------------ dense, over callbacks with a constraint
def _rosen(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))


def _rosen_grad(x):
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return g


def _feasible(x):
    return bool(np.all(np.abs(x) <= 1.25))


class _CallbackOracle(orc.BFGS):
    """orc.BFGS over the Python objective, gradient and constraint above; records the points the objective is given and the
    constraint's refusals."""

    def __init__(self, x0, step):
        self.dtype, self.n, self.suf = np.dtype(F64), x0.size, "_f64"
        self.points, self.refused = [], 0

        def of(_ctx, xp, nn):
            p = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
            self.points.append(p)
            return _rosen(p)

        def gf(_ctx, gp, xp, nn):
            np.ctypeslib.as_array(gp, shape=(nn,))[:] = _rosen_grad(np.ctypeslib.as_array(xp, shape=(nn,)))

        def cf(_ctx, xp, nn):
            ok = _feasible(np.ctypeslib.as_array(xp, shape=(nn,)))
            self.refused += not ok
            return int(ok)

        dp = C.POINTER(C.c_double)
        self._cbs = (C.CFUNCTYPE(C.c_double, C.c_void_p, dp, C.c_int64)(of), C.CFUNCTYPE(None, C.c_void_p, dp, dp, C.c_int64)(gf),
                     C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_int64)(cf))
        create = orc.lib().orc_bfgs_create_f64
        create.restype = C.c_void_p
        create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64]
        self.h = create(*(C.cast(cb, C.c_void_p) for cb in self._cbs), None, x0.ctypes.data_as(C.c_void_p), step, x0.size)
        assert self.h


def test_dense_search_over_callbacks_with_a_constraint_that_refuses_trial_points():
    """Ten steps, each from the oracle's state.  An infeasible trial point counts as typemax(T) and is no evaluation: the objective
    callback sees exactly the oracle's points, in order, and objective_evaluations is the oracle's.  Points, value and step length
    within _check_step's bound (the two sides form the norms that scale the first trial step in their own order), everything
    counted exactly."""
    x0 = np.array([-1.2, 1.0, -0.5])
    ref = _CallbackOracle(x0, 4.0)                                          # (a first step long enough to leave the feasible cube)
    seen = []

    def objective(x):
        seen.append(x.to_host().copy())
        return _rosen(seen[-1])

    opt = dzo.BFGSOptimizer(objective, lambda g, x: g.upload(_rosen_grad(x.to_host())), lambda x: _feasible(x.to_host()),
                            dzo.DeviceArray.from_host(x0), 4.0)
    for it in range(10):
        opt.install_state(**_oracle_state(ref))
        f_before = ref.current_objective_value
        counts = (opt.objective_evaluations, ref.objective_evaluations, len(seen), len(ref.points))
        opt.step(); ref.step()
        n = opt.n
        state = dict(x=opt.current_point.to_host(), g=opt.current_gradient.to_host(), dx=opt.delta_point.to_host(),
                     dg=opt.delta_gradient.to_host(), d=opt.next_step_direction.to_host(),
                     H=opt.approximate_inverse_hessian.to_host().reshape(n, n), f=opt.current_objective_value,
                     last_step_length=opt.last_step_length, iteration_count=opt.iteration_count,
                     last_step_type=opt.last_step_type, has_terminated=opt.has_terminated)
        _check_step(state, ref, f_before, ("callbacks", it))
        assert opt.objective_evaluations - counts[0] == ref.objective_evaluations - counts[1] == len(seen) - counts[2] == len(ref.points) - counts[3], it
        for p, q in zip(seen[counts[2]:], ref.points[counts[3]:]):
            assert np.abs(p - q).max() <= 1e-10 * np.abs(q).max(), it
        if ref.has_terminated:
            break
    assert ref.refused >= 4 and it >= 5                                     # the constraint did refuse trial points of these searches
