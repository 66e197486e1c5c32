"""The optional L-BFGS behaviours on the device (include/dzo.h: dzo_lbfgs_set_line_search, dzo_lbfgs_set_safeguards) in both
element types, at every exit and at the shapes where the history changes layout: the strong-Wolfe search, the descent check and
the steepest-descent fallback against the oracle, per step from identical state (the protocol of tests/test_gpu_safeguards.py),
and the search over host callbacks against the numpy twin.  Helpers, tolerances, the case list and the decision margin:
tests/lbfgs_options_twin.py (pinned to the oracle on the CPU by tests/test_lbfgs_options_twin.py)."""
import numpy as np
import pytest

import lbfgs_options_twin as tw
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = tw.DTYPES
DT_IDS = ["float64", "float32"]
KIND_IDS = [f"{kind}-n{n}-m{m}" for kind, n, m in tw.KIND_CASES]
WOLFE, BACKTRACKING = dzo.LINE_SEARCH_WOLFE, dzo.LINE_SEARCH_BACKTRACKING


def _oracle_state(ref):
    """What a replay of the oracle's next search needs, copied before the step."""
    S, Y = ref.history_arrays()
    return dict(x=ref.current_point.copy(), g=ref.current_gradient.copy(), f=ref.current_objective_value, S=S, Y=Y, rho=ref.rho_history,
                count=ref.iteration_count, d0=ref.step_direction.copy())


def _replay(ref, st):
    d = st["d0"] if st["count"] == 0 else orc.lbfgs_direction(st["g"].copy(), st["S"], st["Y"], st["rho"])[0]
    return tw.replay_search(ref.problem, st["x"], st["f"], st["g"], d)


def _counts_agree(opt, ref):
    return opt.is_stuck == ref.is_stuck and opt.last_trials == ref.last_trials and opt.iteration_count == ref.iteration_count


def _steps_against_the_oracle(kind, n, m, dtype, safeguards, steps=tw.STEPS, leave_at=None):
    """The oracle runs free; before every step but the first the device is given its state; both step; the fields are compared
    (tw.same_step).  The option is set BEFORE the first step: a handle built from a Problem is a point ring then and has to
    leave it with an empty history.  leave_at: the step before which both go back to the backtracking search.  A step whose
    trial counts or stuck flags differ is excused only by tw.near_a_decision, the next step starts from the oracle's state
    again, and the number of such steps is printed and returned with the number of steps taken."""
    with tw.dot_mode_for(dtype):
        opt, ref, _ = tw._pair(n, m, dtype, kind=kind)
        fresh, after = tw.layouts(kind, n, m, dtype)
        assert opt.ring_layout == fresh
        for o in (opt, ref):
            o.set_line_search(WOLFE)
            if safeguards:
                o.set_safeguards(True, True)
        excused, taken = [], 0
        touched = False
        for it in range(steps):
            if it == leave_at:
                opt.set_line_search(BACKTRACKING); ref.set_line_search(BACKTRACKING)
            if it > 0:
                tw._sync(opt, ref)
            x_old, g_old = opt.current_point.to_host(), opt.current_gradient.to_host()
            st = _oracle_state(ref)
            opt.step(); ref.step()
            taken += 1
            assert opt.ring_layout == after, it
            if not _counts_agree(opt, ref):
                rp = _replay(ref, st)
                wolfe = leave_at is None or it < leave_at
                assert wolfe and ref.last_step_kind == 0 and opt.last_step_kind == 0 and tw.near_a_decision(rp, st["f"], dtype), \
                    (it, opt.is_stuck, ref.is_stuck, opt.last_trials, ref.last_trials, rp["branches"], rp["margins"])
                excused.append((it, opt.is_stuck, ref.is_stuck, opt.last_trials, ref.last_trials, rp["margins"][-1]))
                if ref.is_stuck:
                    break
                dzo._check(dzo.lib().dzo_lbfgs_set_stuck(opt.h, 0))      # (the next step starts from the oracle's state)
                continue
            tw.same_step(opt, ref, ref.problem, kind, x_old, g_old, safeguards)
            if ref.is_stuck:
                break
            if kind == "box":
                x_new = opt.current_point.to_host()
                lo, hi = (dtype(v) for v in tw.BOX["box_constraint"])
                assert x_new.min() >= lo and x_new.max() <= hi, it
                touched |= bool(np.any(x_new == lo) or np.any(x_new == hi))
        # at most one excused step in twenty: no two of them within twenty steps of each other
        assert all(b[0] - a[0] >= 20 for a, b in zip(excused, excused[1:])), excused
        if kind == "box":
            assert touched                                 # the projection inside the search acted on an accepted point
        print(f"{kind} n={n} m={m} {np.dtype(dtype).name}: {taken} steps, {len(excused)} excused {excused if excused else ''}")
        return len(excused), taken


# ------------------------------------------------------------------------------ a, b: per step from identical state
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,n,m", tw.KIND_CASES, ids=KIND_IDS)
def test_wolfe_steps_match_the_oracle_in_both_types(kind, n, m, dtype):
    _steps_against_the_oracle(kind, n, m, dtype, safeguards=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind,n,m", tw.KIND_CASES, ids=KIND_IDS)
def test_wolfe_steps_with_both_safeguards_match_the_oracle(kind, n, m, dtype):
    """The accepted Wolfe step notes its length (lbfgs_note_step_length after the search), the descent check runs before every
    search, and neither steps in on a healthy run."""
    _steps_against_the_oracle(kind, n, m, dtype, safeguards=True)


# ------------------------------------------------------------------------------ e: leaving the option
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,m", [(4100, 5), (4099, 12)])
def test_backtracking_again_after_ten_wolfe_steps(n, m, dtype):
    excused, taken = _steps_against_the_oracle("rosen", n, m, dtype, safeguards=False, steps=20, leave_at=10)
    assert taken == 20


# ------------------------------------------------------------------------------ c: constructed exits
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,m", tw.EXIT_CASES)
@pytest.mark.parametrize("name", list(tw.EXITS))
def test_constructed_exits_leave_what_the_oracle_leaves(name, n, m, dtype):
    """Six oracle steps, a history that makes the next step take one particular exit (tw.EXITS), the device given that state --
    delta_point / delta_gradient included -- and one step of both.  A stuck exit leaves every field bit for bit; after the
    fallback the ring restarts at one pair and the next five steps match."""
    with tw.dot_mode_for(dtype):
        opt, ref, _ = tw._pair(n, m, dtype)
        tw.exit_warmup(name, ref)
        tw.apply_exit(name, ref, [ref, opt])
        tw._sync(opt, ref)
        opt.delta_point.upload(ref.delta_point); opt.delta_gradient.upload(ref.delta_gradient)
        before = tw.device_state(opt)
        assert np.array_equal(before["dx"], ref.delta_point) and np.array_equal(before["dg"], ref.delta_gradient)
        opt.step(); ref.step()
        tw.assert_exit(name, ref); tw.assert_exit(name, opt)
        assert opt.ring_layout == tw.layouts("rosen", n, m, dtype)[1]
        if tw.EXITS[name]["stuck"]:
            tw.assert_nothing_moved(opt, ref, before)
            return
        assert _counts_agree(opt, ref)
        tw.same_step(opt, ref, ref.problem, "rosen", before["x"], before["g"], safeguards=True)
        if name == "zero_fallback":
            for it in range(5):
                tw._sync(opt, ref)
                x_old, g_old = opt.current_point.to_host(), opt.current_gradient.to_host()
                opt.step(); ref.step()
                assert _counts_agree(opt, ref) and opt.history_count == min(m, it + 2), it
                tw.same_step(opt, ref, ref.problem, "rosen", x_old, g_old, safeguards=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,m", tw.EXIT_CASES)
def test_wolfe_max_evals_exit_leaves_the_last_accepted_steps_deltas(n, m, dtype):
    """wolfe_max_evals = 1 at the first step past the sixth (and past the twelfth) whose search needs two evaluations.  The device
    takes the steps before it itself, so its delta_point / delta_gradient are where an accepted step leaves them (the pushed pair),
    and the ORACLE is given the device's state before the step that fails: stuck after one trial, everything bit for bit as
    the step found it and as the oracle holds it."""
    with tw.dot_mode_for(dtype):
        for warm in (tw.EXIT_WARMUP, 2 * tw.EXIT_WARMUP):
            opt, ref, _ = tw._pair(n, m, dtype)
            opt.set_line_search(WOLFE); ref.set_line_search(WOLFE)
            for it in range(warm + 60):
                if it > 0:
                    tw._sync(opt, ref)
                opt.step(); ref.step()
                assert _counts_agree(opt, ref) and not ref.is_stuck, it
                if it + 1 < warm:
                    continue
                before = tw.oracle_follows(opt, ref)
                if tw.replay_search(ref.problem, before["x"], before["f"], before["g"], tw.direction_of(ref))["trials"] >= 2:
                    break
            else:
                raise AssertionError("no search of two evaluations")
            assert np.array_equal(before["dx"], before["S"][0]) and np.array_equal(before["dg"], before["Y"][0])
            opt.set_line_search(WOLFE, max_evals=1); ref.set_line_search(WOLFE, max_evals=1)
            opt.step(); ref.step()
            assert opt.last_trials == 1 and ref.last_trials == 1
            tw.assert_nothing_moved(opt, ref, before)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_free_wolfe_run_of_the_smallest_case_ends_like_the_oracle(dtype):
    """(n, m) = (3, 2) to its natural end, the device running free and the oracle given its state before every step (how such a
    run ends depends on its last roundings, see the CPU test): both end on the same step after the same number of trials, and
    the stuck device holds what the step started from, delta_point / delta_gradient of the last accepted step included."""
    with tw.dot_mode_for(dtype):
        opt, ref, _ = tw._pair(3, 2, dtype)
        opt.set_line_search(WOLFE); ref.set_line_search(WOLFE)
        for it in range(200):
            before = tw.oracle_follows(opt, ref)
            opt.step(); ref.step()
            assert _counts_agree(opt, ref), (it, opt.is_stuck, ref.is_stuck, opt.last_trials, ref.last_trials)
            if opt.is_stuck:
                break
        assert opt.is_stuck and it >= 10
        print(f"{np.dtype(dtype).name}: stuck at step {it} after {opt.last_trials} trials")
        assert np.array_equal(before["dx"], before["S"][0]) and np.array_equal(before["dg"], before["Y"][0])
        tw.assert_nothing_moved(opt, ref, before)


# ------------------------------------------------------------------------------ d: host callbacks against the numpy twin
def _callback_optimizer(dtype, constraint, objective, gradient, x0, step0, m):
    """The device optimizer over host functions of a numpy point (the callbacks copy the point down and the gradient up)."""
    def cons(x):
        return constraint(x.to_host())

    def obj(x):
        return float(objective(x.to_host()))

    def grd(g, x):
        g.upload(np.asarray(gradient(x.to_host()), dtype))
    return dzo.LBFGSOptimizer(cons if constraint else None, obj, grd, dzo.DeviceArray.from_host(np.asarray(x0, dtype)), step0, m)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 5])
def test_wolfe_bisects_down_from_infeasible_trials_like_the_twin(n, dtype):
    """A constraint callback that rejects max |x| > 1: the first trials of the first step are infeasible (f_t = tmax) and the
    search bisects down from them.  Every step against tw.wolfe_search from the device's own state along the device's direction:
    trial count, accepted point, objective value and gradient bit for bit."""
    cons, obj, grad = tw.bounded_quadratic(n, dtype)
    x0 = np.full(n, tw.BOUND_X0, dtype)
    with tw.dot_mode_for(dtype):
        opt = _callback_optimizer(dtype, cons, obj, grad, x0, tw.BOUND_STEP0, 3)
        opt.set_line_search(WOLFE)
        branches = []
        for it in range(6):
            x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
            opt.step()
            r = tw.wolfe_search(x, f, g, opt.step_direction.to_host(), cons, obj, grad, dtype)
            if it == 0:
                assert r["branches"][:2] == ["infeasible", "infeasible"] and r["accepted"]
            assert opt.is_stuck == (not r["accepted"]) and opt.last_trials == r["trials"], (it, opt.last_trials, r["branches"])
            if opt.is_stuck:
                break
            assert np.array_equal(opt.current_point.to_host(), r["x_new"]) and opt.current_objective_value == r["f_new"], it
            assert np.array_equal(opt.current_gradient.to_host(), r["g_new"]) and cons(r["x_new"]), it
            assert np.array_equal(opt.delta_point.to_host(), r["x_new"] - x) and np.array_equal(opt.delta_gradient.to_host(), r["g_new"] - g), it
            branches += r["branches"]
        assert it >= 2 and branches.count("infeasible") >= 2


@pytest.mark.parametrize("explicit", [False, True], ids=["defaults", "explicit"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_wolfe_constants_at_their_edges_like_the_twin(dtype, explicit):
    """n = 1, start gradient 1, step length 1: ir = -f_trial and sr = g_trial at the first trial.  ir == (T)1e-4 is accepted at
    one evaluation and one ulp below fails Armijo; |sr| == (T)0.9 is accepted and one ulp outside is not -- with the default
    constants (which the handle holds in its element type) and with the same constants passed explicitly."""
    T = np.dtype(dtype).type
    consts = (1e-4, 0.9) if explicit else ()
    for name, f_trial, g_trial, first in tw.edge_cases(dtype):
        obj, grad = tw.edge_functions(dtype, f_trial, g_trial)
        x0 = np.array([tw.EDGE_X0], dtype)
        opt = _callback_optimizer(dtype, None, obj, grad, x0, 1.0, 2)
        opt.set_line_search(WOLFE, *consts)
        x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
        assert g[0] == 1 and f == 0
        opt.step()
        d = opt.step_direction.to_host()
        assert d[0] == -1, name
        r = tw.wolfe_search(x, f, g, d, None, obj, grad, dtype, *consts)
        assert r["branches"][0] == first, name
        assert opt.is_stuck == (not r["accepted"]) and opt.last_trials == r["trials"], (name, opt.is_stuck, opt.last_trials, r["trials"])
        if r["accepted"]:
            assert r["trials"] == 1 and opt.iteration_count == 1, name
            assert opt.current_point.to_host()[0] == T(tw.EDGE_X0 - 1) and opt.current_objective_value == float(T(f_trial)), name
        else:
            assert opt.iteration_count == 0 and opt.current_point.to_host()[0] == T(tw.EDGE_X0), name
