"""tests/lbfgs_options_twin.py pinned to the oracle, on the CPU: the replay of the Wolfe search against orc.LBFGS.step() bit for
bit on the whole case list of tests/test_gpu_lbfgs_options.py, the numpy twin against the replay, the branches the case list
reaches, the fields the constructed exits leave on the oracle, and the measured decision margin."""
import functools

import numpy as np
import pytest

import lbfgs_options_twin as tw
from oracle import oracle as orc

DTYPES = tw.DTYPES
IDS = [f"{kind}-n{n}-m{m}" for kind, n, m in tw.KIND_CASES]


@functools.lru_cache(maxsize=None)
def _run(kind, n, m, dtype_name):
    """The oracle's free Wolfe run of one case, every step replayed beforehand: computed once, read by several tests."""
    dtype = np.dtype(dtype_name).type
    steps, branches, touched = [], [], False
    with tw.dot_mode_for(dtype):
        ref, p = tw.oracle_optimizer(kind, n, m, dtype)
        ref.set_line_search(1)
        for _ in range(tw.STEPS):
            x, g, f = ref.current_point.copy(), ref.current_gradient.copy(), ref.current_objective_value
            rp = tw.replay_search(p, x, f, g, tw.direction_of(ref))
            ref.step()
            steps.append((rp, ref.is_stuck, ref.last_trials, ref.current_point.copy(), ref.current_objective_value, ref.current_gradient.copy()))
            branches += rp["branches"]
            if kind == "box" and not ref.is_stuck:
                lo, hi = (dtype(v) for v in tw.BOX["box_constraint"])
                touched |= bool(np.any(ref.current_point == lo) or np.any(ref.current_point == hi))
            if ref.is_stuck:
                break
    return steps, branches, touched


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("kind,n,m", tw.KIND_CASES, ids=IDS)
def test_replay_is_the_oracles_search_bit_for_bit(kind, n, m, dtype):
    steps, _, touched = _run(kind, n, m, np.dtype(dtype).name)
    assert len(steps) >= 3                                 # (log-sum-exp converges within a handful of steps)
    for it, (rp, stuck, trials, x, f, g) in enumerate(steps):
        assert rp["trials"] == trials and rp["accepted"] == (not stuck), it
        assert rp["branches"].count("accept") == (0 if stuck else 1) and len(rp["margins"]) == trials, it
        if not stuck:
            assert np.array_equal(rp["x_new"], x) and rp["f_new"] == f and np.array_equal(rp["g_new"], g), it
    if kind == "box":
        assert touched                                     # an accepted point sits on a bound: the search's projection acted


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_case_list_takes_every_branch_of_the_search(dtype):
    seen = set()
    for kind, n, m in tw.KIND_CASES:
        seen |= set(_run(kind, n, m, np.dtype(dtype).name)[1])
    assert seen >= {"armijo_fail", "too_steep", "overshoot", "accept"}, seen


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("kind,n,m", [("rosen", 3, 2), ("box", 65, 4), ("box", 257, 4), ("qchain", 65, 4), ("rosen", 1000, 5)])
def test_numpy_twin_is_the_replay_over_callbacks(kind, n, m, dtype):
    """wolfe_search over Python callbacks that wrap the oracle's problem (the box as a projecting constraint callback) takes the
    replay's branches and accepts its point, at every step of the oracle's run."""
    with tw.dot_mode_for(dtype):
        ref, p = tw.oracle_optimizer(kind, n, m, dtype)
        ref.set_line_search(1)
        box = tw.BOX["box_constraint"] if kind == "box" else None

        def constraint(xt):
            orc.box_clamp(xt, *box)
            return True
        for it in range(15):
            x, g, f = ref.current_point.copy(), ref.current_gradient.copy(), ref.current_objective_value
            d = tw.direction_of(ref)
            a = tw.replay_search(p, x, f, g, d)
            b = tw.wolfe_search(x, f, g, d, constraint if box else None, p.eval, p.grad, dtype)
            assert a["branches"] == b["branches"] and a["trials"] == b["trials"] and a["accepted"] == b["accepted"], it
            if a["accepted"]:
                assert a["t"] == b["t"] and np.array_equal(a["x_new"], b["x_new"]) and a["f_new"] == b["f_new"], it
                assert np.array_equal(a["g_new"], b["g_new"]), it
            ref.step()
            if ref.is_stuck:
                break


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_numpy_twin_bisects_down_from_infeasible_trials(dtype):
    """By hand at n = 1: x = 0.5, d = -8, |x| <= 1, f = (x - 0.2)^2 (w_0 = 1).  t = 1, 1/2, 1/4 are infeasible (x = -7.5, -3.5,
    -1.5); t = 1/8 gives x = -0.5, f = 0.49 > 0.09: Armijo fails; t = 1/16 gives x = 0, f = 0.04, ir = 1/6, sr = -2/3: accepted."""
    cons, obj, grad = tw.bounded_quadratic(1, dtype)
    x = np.array([tw.BOUND_X0], dtype)
    g = grad(x)
    d = np.array([-tw.BOUND_STEP0], dtype)
    r = tw.wolfe_search(x, obj(x), g, d, cons, obj, grad, dtype)
    assert r["branches"] == ["infeasible"] * 3 + ["armijo_fail", "accept"] and r["trials"] == 5
    assert r["t"] == 0.0625 and r["x_new"][0] == 0.0
    # a search that stays infeasible ends when the evaluations run out, with nothing accepted
    r = tw.wolfe_search(x, obj(x), g, d, lambda xt: False, obj, grad, dtype, max_evals=7)
    assert not r["accepted"] and r["branches"] == ["infeasible"] * 7


@pytest.mark.parametrize("explicit", [False, True], ids=["defaults", "explicit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_numpy_twin_at_the_c1_and_c2_edges(dtype, explicit):
    """ir == (T)1e-4 passes Armijo (>=) and one ulp below fails; |sr| == (T)0.9 passes the curvature test and one ulp outside
    fails, on either side -- with the defaults and with the same constants passed explicitly."""
    T = np.dtype(dtype).type
    for name, f_trial, g_trial, first in tw.edge_cases(dtype):
        obj, grad = tw.edge_functions(dtype, f_trial, g_trial)
        x = np.array([tw.EDGE_X0], dtype)
        r = tw.wolfe_search(x, obj(x), grad(x), -grad(x), None, obj, grad, dtype, *((1e-4, 0.9) if explicit else ()))
        assert r["branches"][0] == first, name
        assert r["accepted"] == (first == "accept") and (r["trials"] == 1) == (first == "accept"), name
        if first == "accept":
            assert r["t"] == T(1) and r["x_new"][0] == T(tw.EDGE_X0 - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("n,m", tw.EXIT_CASES)
@pytest.mark.parametrize("name", list(tw.EXITS))
def test_constructed_exits_on_the_oracle(name, n, m, dtype):
    with tw.dot_mode_for(dtype):
        ref, _ = tw.oracle_optimizer("rosen", n, m, dtype)
        tw.exit_warmup(name, ref)
        tw.apply_exit(name, ref, [ref])
        x, g, f = ref.current_point.copy(), ref.current_gradient.copy(), ref.current_objective_value
        dx, dg = ref.delta_point.copy(), ref.delta_gradient.copy()
        S, Y = ref.history_arrays()
        trials = ref.last_trials
        ref.step()
        tw.assert_exit(name, ref)
        if tw.EXITS[name]["stuck"]:
            assert np.array_equal(ref.current_point, x) and np.array_equal(ref.current_gradient, g) and ref.current_objective_value == f
            assert np.array_equal(ref.delta_point, dx) and np.array_equal(ref.delta_gradient, dg)       # the last accepted step's
            S1, Y1 = ref.history_arrays()
            assert np.array_equal(S1, S) and np.array_equal(Y1, Y, equal_nan=True)
            if tw.EXITS[name]["trials"] is None:
                assert ref.last_trials == trials                                                     # no search ran
        elif name == "zero_fallback":
            for it in range(5):                            # the ring restarts at one pair
                ref.step()
                assert ref.history_count == min(m, it + 2) and not ref.is_stuck


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("n,m", tw.EXIT_CASES)
def test_max_evals_exit_on_the_oracle(n, m, dtype):
    """wolfe_max_evals = 1 at the first step past the sixth (and past the twelfth) whose search needs two evaluations: stuck after
    one trial, x / dx / dg / history unchanged."""
    with tw.dot_mode_for(dtype):
        for warm in (tw.EXIT_WARMUP, 2 * tw.EXIT_WARMUP):
            ref, p = tw.oracle_optimizer("rosen", n, m, dtype)
            ref.set_line_search(1)
            for _ in range(warm):
                ref.step()
            for _ in range(60):
                x, g, f = ref.current_point.copy(), ref.current_gradient.copy(), ref.current_objective_value
                if tw.replay_search(p, x, f, g, tw.direction_of(ref))["trials"] >= 2:
                    break
                ref.step()
                assert not ref.is_stuck
            else:
                raise AssertionError("no search of two evaluations")
            dx, dg = ref.delta_point.copy(), ref.delta_gradient.copy()
            S, Y = ref.history_arrays()
            count = ref.iteration_count
            ref.set_line_search(1, max_evals=1)
            ref.step()
            assert ref.is_stuck and ref.last_trials == 1 and ref.iteration_count == count
            assert np.array_equal(ref.current_point, x) and np.array_equal(ref.current_gradient, g) and ref.current_objective_value == f
            assert np.array_equal(ref.delta_point, dx) and np.array_equal(ref.delta_gradient, dg)
            S1, Y1 = ref.history_arrays()
            assert np.array_equal(S1, S) and np.array_equal(Y1, Y)


@pytest.mark.parametrize("dtype,last", [(np.float64, 90), (np.float32, 49)], ids=["float64", "float32"])
def test_free_wolfe_run_of_the_smallest_case_ends_without_a_trial(dtype, last):
    """(n, m) = (3, 2) run free in the oracle's default dot mode: the run reaches x = 1 exactly, the search of step `last` finds
    g.d = 0 and ends with no trial.  (How such a run ends depends on the last roundings: with the wide dot the fp32 run ends at
    step 43 on wolfe_max_evals instead, the fp64 one at step 89 without a trial.  The GPU test therefore lets the oracle follow
    the device and compares the exit both sides take.)"""
    ref, _ = tw.oracle_optimizer("rosen", 3, 2, dtype)
    ref.set_line_search(1)
    for _ in range(200):
        dx, dg = ref.delta_point.copy(), ref.delta_gradient.copy()
        ref.step()
        if ref.is_stuck:
            break
    assert ref.is_stuck and ref.last_trials == 0 and ref.iteration_count == last
    assert np.all(ref.current_point == 1) and np.all(ref.current_gradient == 0)
    assert np.array_equal(ref.delta_point, dx) and np.array_equal(ref.delta_gradient, dg)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_decision_margin_is_the_measured_one(dtype):
    """A fresh measurement stays inside the figures of the helper's docstring, is not far below them (they are measurements, not
    allowances), and the two dot modes never disagree on a trial count over the case list."""
    m_ir, m_sr, m_f, disagreements, steps = tw.measure_decision_margin(dtype)
    want = tw.DECISION_MARGIN[np.dtype(dtype)]
    assert disagreements == 0 and steps >= 900
    for got, limit in zip((m_ir, m_sr, m_f), want):
        assert 0.95 * limit <= got <= limit, (got, limit)


def test_rho_bound_holds_for_other_summation_orders():
    """The bound on rho covers a sum carried in fp64 in another order (here: reversed, and pairwise), in both types."""
    rng = np.random.default_rng(3)
    for dtype in DTYPES:
        for n in (1, 3, 65, 4100):
            dx, dg = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
            value, bound = tw.rho_bound(dx, dg, dtype)
            p = dx.astype(np.float64) * dg.astype(np.float64)
            for s in (np.sum(p), sum(p[::-1].tolist())):
                assert abs(float(dtype(s)) - value) <= bound
            assert bound <= (n + 2) * 2.0 ** -52 * np.abs(p).sum() + 2.0 ** -22 * abs(value)      # ... and is no allowance beyond that
