"""Helpers for the tests of the optional L-BFGS behaviours (include/dzo.h: dzo_lbfgs_set_line_search, dzo_lbfgs_set_safeguards):
the strong-Wolfe search, the descent check and the steepest-descent fallback.  A helper module like tests/sphere_twin.py: no
fixtures, not a conftest, imported by name from tests/test_lbfgs_options_twin.py (CPU: pins everything below to the oracle),
tests/test_gpu_lbfgs_options.py and tests/test_gpu_safeguards.py (GPU: hold the device to the oracle and to the twin).

What is here

  wolfe_search     the loop of oracle/dzo_oracle_impl.h:495-527 in numpy, in the element type, over Python callbacks
                   (constraint, objective, gradient): the oracle's Python wrapper has no callback entry.  Returns the accepted t,
                   the trial count and the branch every evaluation took.
  replay_search    the same loop over a built-in Problem, every evaluation through orc.line_search_eval: the branch list and, per
                   evaluation, the margins of the decisions that were taken (ir - c1, f_t - f, |sr| - c2).
  the device side  _pair / _sync / _same_step (the protocol of test_gpu_safeguards: the oracle runs free, the device is given its
                   state before every step) and same_step, which adds fp32 and the identities on the device's own fields.

Tolerances (nothing here is fitted to what the device returns)

  fp64 against the oracle: the numbers of _same_step, unchanged.
  fp32 against the oracle (orc.DOT_WIDE, the device sums in fp64): the rules of test_gpu_lbfgs._point_ring_steps_against_the_oracle
      -- direction 2e-4, point max(1e-6, 2 e_d max(1, moved_by)), objective value rel 1e-5.
  both types, exact: delta_point == x_new - x_old, delta_gradient == g_new - g_old, current_gradient == grad(x_new) for the
      chained objectives (term-relative for log-sum-exp, as in the point-ring tests).
  rho_history[0]: rho_bound below, from operation counts.

The decision margin.  Trial counts and stuck flags are compared exactly; a step whose counts differ is excused only when the
replay shows a decision that was actually taken within DECISION_MARGIN_FACTOR x the measured margin of zero.  The measured
margin is the largest difference of ir, sr (absolute: both are ratios of order one) and f_t (relative to |f|) between the
oracle's DOT_SEQUENTIAL and DOT_WIDE on the same trial -- same point, same direction, same t -- over the whole case list
(measure_decision_margin below, run on the CPU; test_lbfgs_options_twin.py asserts that a new measurement stays inside):

                 ir          sr          f_t        steps   trial counts that differed
    float64      6.37e-03    3.52e-12    2.15e-16   955     0
    float32      1.86e-03    4.83e-03    1.15e-07   956     0

(measured values rounded up in the third digit.  f_t differs only under the L2 decorator, whose term is a dot product.  The
large ir figures come from the last steps of the decorated runs: there f_t - f is a few roundings of f, and ir is the quotient
of two such numbers; on the plain chained Rosenbrock alone the figures are 8.9e-15 / 1.2e-13 and 2.8e-05 / 3.4e-04.)
The factor is 4: the device's fp64 block sums are a third summation order, and its direction a fourth.  At most one step in
twenty may be excused per case (no two excused steps of a run within twenty steps of each other); none in the constructed exits
and the callback cases, whose margins are large by construction.  On the MI355X the chained cases excuse nothing (about 3000
steps); the two fp64 log-sum-exp runs, which converge in 12 and 7 steps, excuse one step each, next to their end, where
f_t - f is one or two ulps of f (-4.4e-16 at f = 3.44, -1.8e-15 at f = 8.35) and the device takes 3 trials for the oracle's 1,
or 1 for its 2.
"""
import contextlib
import math

import numpy as np

import lbfgs_plan_twin as plan
from oracle import oracle as orc

DTYPES = [np.float64, np.float32]
# (n, m): below four 16-byte vectors in both types (2, 3), in fp32 only (7); the wave edge 63 / 64 / 65; ragged 257; whole
# wave-rows 372 = 6 x 62; aligned 1000; 4099 becomes slabs, 4100 the tile pair ring
CASES = [(2, 3), (3, 2), (7, 3), (63, 4), (64, 4), (65, 4), (257, 4), (372, 5), (1000, 5), (4099, 12), (4100, 5)]
EXIT_CASES = [(3, 2), (65, 4), (257, 4), (4099, 12), (4100, 5)]
BOX = dict(l2=0.01, box_gradient=(-1.1, 0.9), box_constraint=(-1.1, 0.9))
KIND_CASES = [(kind, n, m) for kind in ("rosen", "box") for n, m in CASES] + [(kind, n, m) for kind in ("qchain", "lse") for n, m in [(65, 4), (4100, 5)]]
STEPS = 40

# measured (see the docstring): dtype -> (ir, sr, f_t relative)
DECISION_MARGIN = {np.dtype(np.float64): (6.37e-03, 3.52e-12, 2.15e-16), np.dtype(np.float32): (1.86e-03, 4.83e-03, 1.15e-07)}
DECISION_MARGIN_FACTOR = 4.0
BRANCHES = ("armijo_fail", "too_steep", "overshoot", "accept", "infeasible")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@contextlib.contextmanager
def dot_mode_for(dtype):
    """fp32: the oracle's dots carried wide, as the device's are (fp64 sums, one rounding to fp32)."""
    if np.dtype(dtype) == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        yield
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


# ------------------------------------------------------------------------------ the problems of the case list
def lse_centre(n, dtype):
    return (orc.pcg_fill(n, 6) - 0.5).astype(dtype)


def start_point(kind, n, dtype):
    if kind == "lse":
        return (0.5 * (orc.pcg_fill(n, 8) - 0.5)).astype(dtype)
    return orc.rosenbrock_chain_x0(n, dtype)


def oracle_problem(kind, n, dtype):
    if kind == "lse":
        return orc.Problem(orc.LSE, n, dtype, c=lse_centre(n, dtype), lam=1e-2)
    if kind == "qchain":
        return orc.Problem(orc.QUADRATIC_CHAIN, n, dtype, lam=0.05)
    return orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, **(BOX if kind == "box" else {}))


def device_problem(kind, n, dtype):
    from dzo_loader import dzo
    if kind == "lse":
        return dzo.Problem(dzo.LSE, n, dtype, c=lse_centre(n, dtype), lam=1e-2)
    if kind == "qchain":
        return dzo.Problem(dzo.QUADRATIC_CHAIN, n, dtype, lam=0.05)
    return dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype, **(BOX if kind == "box" else {}))


def oracle_optimizer(kind, n, m, dtype, step0=1.0):
    p = oracle_problem(kind, n, dtype)
    return orc.LBFGS(p, start_point(kind, n, dtype).copy(), step0, m), p


def layouts(kind, n, m, dtype):
    """(ring_layout a fresh handle has, ring_layout after the first step with an option), from the plan's twin."""
    dt = plan.F64 if np.dtype(dtype) == np.float64 else plan.F32
    pk = {"lse": plan.LSE, "qchain": plan.QUADRATIC_CHAIN}.get(kind, plan.ROSENBROCK_CHAIN)
    L = plan.layout(n, dt, m, kind=pk, decorated=kind == "box")
    return plan.ring_layout(L["blocked"], L["points"]), plan.layout_after_leaving_points(L, n, dt, False)


# ------------------------------------------------------------------------------ the search, twice
def _branch(T, f, f_t, ir, sr, c1, c2):
    """The decision of :507-510 on values of type T."""
    if not (ir >= c1) or not (f_t < f):
        return "armijo_fail"
    if sr > c2:
        return "too_steep"
    if sr < -c2:
        return "overshoot"
    return "accept"


def _constants(dtype, c1, c2):
    T = np.dtype(dtype).type
    return T, (T(1e-4) if not c1 else T(c1)), (T(0.9) if not c2 else T(c2))       # :410, :1070-1071


def wolfe_search(x, f, g, d, constraint, objective, gradient, dtype, c1=0.0, c2=0.0, max_evals=40):
    """oracle/dzo_oracle_impl.h:495-527 (and the evaluator call :477-489) over Python callbacks: constraint(xt) -> bool (may
    project xt in place; None: no constraint), objective(xt) -> value, gradient(xt) -> array.  Every scalar operation is one
    rounding in T; the two dot products and the axpy are the oracle's own primitives (orc.dot honours the dot mode).  Returns a
    dict: accepted, t, trials, branches, and x_new / f_new / g_new when accepted."""
    T, c1, c2 = _constants(dtype, c1, c2)
    tmax = T(np.finfo(np.dtype(dtype)).max)
    x, g, d, f = np.asarray(x, dtype), np.asarray(g, dtype), np.asarray(d, dtype), T(f)
    out = dict(accepted=False, t=None, trials=0, branches=[])
    overlap = T(orc.dot(g, d))                                      # :499
    if not (overlap < T(0)):                                        # :500
        return out
    half = T(1) / (T(1) + T(1))
    t, lo, hi = T(1), T(0), T(-1)
    with np.errstate(all="ignore"):
        for _ in range(max_evals):
            xt = x.copy()                                           # :479-480
            orc.axpy(t, d, xt)
            if constraint is not None and not constraint(xt):       # :481-484
                f_t, ir, sr, gt = tmax, -tmax, tmax, None
                branch = "infeasible"
            else:
                f_t = T(objective(xt))                              # :485
                ir = T(T(f_t - f) / T(t * overlap))                 # :486
                gt = np.asarray(gradient(xt), dtype)                # :487
                sr = T(T(orc.dot(gt, d)) / overlap)                 # :488
                branch = _branch(T, f, f_t, ir, sr, c1, c2)
            out["trials"] += 1
            out["branches"].append(branch)
            if branch in ("armijo_fail", "infeasible", "overshoot"):
                hi = t
            elif branch == "too_steep":
                lo = t
            else:
                out.update(accepted=True, t=t, x_new=xt, f_new=f_t, g_new=gt)
                return out
            t_next = T(t + t) if hi < T(0) else T(T(lo + hi) * half)    # :521
            if t_next == lo or t_next == hi or not (t_next > T(0)):     # :522
                break
            t = t_next
    return out


def direction_of(ref):
    """The direction the oracle's next step!() searches along without a safeguard stepping in: the constructor's (:386-387)
    before the first step, the two-loop recursion (:430-451, the oracle's own function) afterwards."""
    if ref.iteration_count == 0:
        return ref.step_direction.copy()
    S, Y = ref.history_arrays()
    return orc.lbfgs_direction(ref.current_gradient.copy(), S, Y, ref.rho_history)[0]


def replay_search(problem, x, f, g, d, c1=0.0, c2=0.0, max_evals=40):
    """The oracle's search replayed evaluation by evaluation through orc.line_search_eval (the evaluator the search is written
    on, constraint callback included).  As wolfe_search, plus `margins`: per evaluation a dict of the decisions that were taken
    there -- ir (ir - c1) and f (f_t - f) always, sr (|sr| - c2) when Armijo held -- and `evals`: (t, f_t, ir, sr)."""
    dtype = problem.dtype
    T, c1, c2 = _constants(dtype, c1, c2)
    x, g, d, f = np.ascontiguousarray(x, dtype), np.ascontiguousarray(g, dtype), np.ascontiguousarray(d, dtype), T(f)
    out = dict(accepted=False, t=None, trials=0, branches=[], margins=[], evals=[])
    overlap = T(orc.dot(g, d))
    if not (overlap < T(0)):
        return out
    half = T(1) / (T(1) + T(1))
    tmax = T(np.finfo(np.dtype(dtype)).max)
    t, lo, hi = T(1), T(0), T(-1)
    with np.errstate(all="ignore"):
        for _ in range(max_evals):
            f_t, ir, sr, xt, gt = orc.line_search_eval(problem, x, f, d, overlap, t, True)
            f_t, ir, sr = T(f_t), T(ir), T(sr)
            if f_t == tmax and ir == -tmax:
                branch, margin = "infeasible", {}
            else:
                branch = _branch(T, f, f_t, ir, sr, c1, c2)
                margin = dict(ir=float(ir) - float(c1), f=float(f_t) - float(f))
                if branch != "armijo_fail":
                    margin["sr"] = abs(float(sr)) - float(c2)
            out["trials"] += 1
            out["branches"].append(branch)
            out["margins"].append(margin)
            out["evals"].append((t, f_t, ir, sr))
            if branch in ("armijo_fail", "infeasible", "overshoot"):
                hi = t
            elif branch == "too_steep":
                lo = t
            else:
                out.update(accepted=True, t=t, x_new=xt, f_new=f_t, g_new=gt)
                return out
            t_next = T(t + t) if hi < T(0) else T(T(lo + hi) * half)
            if t_next == lo or t_next == hi or not (t_next > T(0)):
                break
            t = t_next
    return out


def near_a_decision(replay, f, dtype):
    """True when one decision the replay took lies within DECISION_MARGIN_FACTOR x the measured margin of zero."""
    m_ir, m_sr, m_f = (DECISION_MARGIN_FACTOR * v for v in DECISION_MARGIN[np.dtype(dtype)])
    for mg in replay["margins"]:
        if "ir" in mg and (abs(mg["ir"]) <= m_ir or abs(mg["f"]) <= m_f * abs(float(f))):
            return True
        if "sr" in mg and abs(mg["sr"]) <= m_sr:
            return True
    return False


def measure_decision_margin(dtype, kind_cases=None, steps=STEPS):
    """The measurement behind DECISION_MARGIN: the oracle runs free with the Wolfe search (DOT_SEQUENTIAL); before every step
    its search is replayed from the same point along the same direction under DOT_SEQUENTIAL and under DOT_WIDE, and the
    differences of ir, sr and f_t (relative to |f|) are taken evaluation by evaluation for as long as both replays evaluate the
    same t.  Returns (max |d ir|, max |d sr|, max |d f_t| / |f|, number of steps whose trial counts differed, steps)."""
    worst, disagreements, total = [0.0, 0.0, 0.0], 0, 0
    for kind, n, m in (KIND_CASES if kind_cases is None else kind_cases):
        ref, p = oracle_optimizer(kind, n, m, dtype)
        ref.set_line_search(1)
        for _ in range(steps):
            x, g, f = ref.current_point.copy(), ref.current_gradient.copy(), ref.current_objective_value
            d = direction_of(ref)
            a = replay_search(p, x, f, g, d)
            orc.set_dot_mode(orc.DOT_WIDE)
            try:
                b = replay_search(p, x, f, g, d)
            finally:
                orc.set_dot_mode(orc.DOT_SEQUENTIAL)
            total += 1
            disagreements += a["trials"] != b["trials"] or a["accepted"] != b["accepted"]
            for (ta, fa, ia, sa), (tb, fb, ib, sb) in zip(a["evals"], b["evals"]):
                if ta != tb:
                    break
                if fa == np.finfo(np.dtype(dtype)).max:
                    continue
                worst[0] = max(worst[0], abs(float(ia) - float(ib)))
                worst[1] = max(worst[1], abs(float(sa) - float(sb)))
                worst[2] = max(worst[2], abs(float(fa) - float(fb)) / max(abs(float(f)), 1e-300))
            ref.step()
            if ref.is_stuck:
                break
    return worst[0], worst[1], worst[2], disagreements, total


# ------------------------------------------------------------------------------ constructed exits
# name -> what the oracle leaves after the one step that follows (measured on the CPU in both types at every EXIT_CASES size;
# test_lbfgs_options_twin.py asserts it).  trials None: no search ran (the exit is before it).
EXITS = {
    "reversed_plain": dict(stuck=True, trials=0),                                        # history (S, -Y), Wolfe: g.d >= 0, :500
    "reversed_descent": dict(stuck=False, kind=1, descent_resets=1, history_resets=0),   # ... the descent check replaces d
    "zero_fallback": dict(stuck=False, kind=2, history_count=1, descent_resets=0, history_resets=1),   # history (S, 0 Y): d is NaN
    "zero_plain": dict(stuck=True, trials=0),
    "nan_descent": dict(stuck=True, trials=None),                                        # history (S, NaN Y): g.d not finite, :555
}
EXIT_WARMUP = 6


def apply_exit(name, ref, both):
    """Turn the oracle's history into the construction's and set the options on every optimizer of `both` (the oracle, and the
    device's when there is one).  The device still has to be given the oracle's state (_sync)."""
    S, Y = ref.history_arrays()
    factor = {"reversed": -1.0, "zero": 0.0, "nan": np.nan}[name.split("_")[0]]
    with np.errstate(all="ignore"):
        ref.set_history(S, (factor * Y).astype(ref.dtype), iteration_count=ref.iteration_count)
    for o in both:
        if name != "nan_descent":
            o.set_line_search(1)
        if name.startswith("zero"):
            o.set_max_halvings(64)
        o.set_safeguards(name.endswith("descent"), name.endswith("fallback"))


def exit_warmup(name, ref):
    """The six free oracle steps before a construction (Wolfe from the first step on, except where the construction has none)."""
    if name != "nan_descent":
        ref.set_line_search(1)
    for _ in range(EXIT_WARMUP):
        ref.step()
    assert not ref.is_stuck and ref.iteration_count == EXIT_WARMUP


def assert_exit(name, o):
    """The table row of `name` on one optimizer (either side)."""
    want = EXITS[name]
    assert o.is_stuck == want["stuck"], name
    if want.get("trials") is not None:
        assert o.last_trials == want["trials"], name
    if not want["stuck"]:
        assert o.iteration_count == EXIT_WARMUP + 1 and o.last_step_kind == want["kind"], name
        assert o.descent_resets == want["descent_resets"] and o.history_resets == want["history_resets"], name
        if "history_count" in want:
            assert o.history_count == want["history_count"], name
    else:
        assert o.iteration_count == EXIT_WARMUP, name


# ------------------------------------------------------------------------------ callback problems (host functions of a numpy point)
EDGE_X0 = 2.0


def edge_cases(dtype):
    """The c1 / c2 edges at n = 1: start gradient 1 and step length 1 give d = -1 and overlap = -1, so at the first trial
    (t = 1, x = EDGE_X0 - 1) ir = -f_trial and sr = g_trial exactly.  (name, f_trial, g_trial, branch of the first evaluation):
    ir at (T)1e-4 and one ulp below it, sr at +-(T)0.9 and one ulp outside."""
    T = np.dtype(dtype).type
    c1, c2 = T(1e-4), T(0.9)
    below, above = np.nextafter(c1, T(0)), np.nextafter(c2, T(np.inf))
    return [("c1_at", -c1, T(0.5), "accept"), ("c1_below", -below, T(0.5), "armijo_fail"),
            ("c2_at_pos", T(-0.5), c2, "accept"), ("c2_at_neg", T(-0.5), -c2, "accept"),
            ("c2_above_pos", T(-0.5), above, "too_steep"), ("c2_above_neg", T(-0.5), -above, "overshoot")]


def edge_functions(dtype, f_trial, g_trial):
    """(objective, gradient) of a host point for one edge case: 0 / 1 at the start, f_trial / g_trial at the first trial, and
    1 / 0 anywhere else (no other point passes Armijo: a search that does not accept at once ends stuck)."""
    T = np.dtype(dtype).type
    start, trial = T(EDGE_X0), T(EDGE_X0 - 1)

    def objective(x):
        return T(0) if x[0] == start else (T(f_trial) if x[0] == trial else T(1))

    def gradient(x):
        return np.array([T(1) if x[0] == start else (T(g_trial) if x[0] == trial else T(0))], dtype)
    return objective, gradient


BOUND_X0, BOUND, BOUND_STEP0, BOUND_CENTRE = 0.5, 1.0, 8.0, 0.2


def bounded_quadratic(n, dtype):
    """(constraint, objective, gradient) of a host point: f = sum w_i (x_i - 0.2)^2 with w_i = 1 + i, in T, and a constraint
    that REJECTS max |x| > 1 (it projects nothing).  From x = 0.5 with initial step length 8 the first trials are infeasible."""
    T = np.dtype(dtype).type
    w = (1 + np.arange(n)).astype(dtype)

    def constraint(x):
        return bool(np.max(np.abs(x)) <= T(BOUND))

    def objective(x):
        r = x - T(BOUND_CENTRE)
        return T(np.sum(w * r * r, dtype=dtype))

    def gradient(x):
        return (T(2) * w * (x - T(BOUND_CENTRE))).astype(dtype)
    return constraint, objective, gradient


# ------------------------------------------------------------------------------ rho = s.y, from operation counts
def rho_bound(dx, dg, dtype):
    """(value, bound) for rho_history[0] of a device that holds dx and dg: the value is math.fsum of the n products -- exact in
    fp64 for fp32 inputs (24 + 24 bits), one rounding each (none under FMA) for fp64 inputs -- rounded once to the element type.
    The device carries the sum in fp64 in an order of its own and rounds once to the element type: n - 1 additions in any order
    and at most one rounding per product are gamma_n sum |dx_i dg_i| with gamma_n = n u / (1 - n u), u = 2^-53 (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5); fsum's own error is below that of one more addition
    (gamma_n+1 covers both sides), and the rounding to the element type, made on both sides, adds 2 u_T |rho|."""
    T = np.dtype(dtype).type
    p = dx.astype(np.float64) * dg.astype(np.float64)
    exact = math.fsum(p)
    u, n = 2.0 ** -53, len(p) + 1
    u_t = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    gamma = n * u / (1 - n * u)
    return float(T(exact)), gamma * math.fsum(np.abs(p)) + 2 * u_t * abs(exact)


# ------------------------------------------------------------------------------ the device side
def _pair(n, m, dtype=np.float64, mode=None, kind="rosen", step0=1.0):
    """(device optimizer, oracle optimizer, device problem) on the same start."""
    from dzo_loader import dzo
    x0 = start_point(kind, n, dtype)
    ref = orc.LBFGS(oracle_problem(kind, n, dtype), x0.copy(), step0, m)
    prob = device_problem(kind, n, dtype)
    opt = dzo.LBFGSOptimizer(None, prob, None, dzo.DeviceArray.from_host(x0), step0, m)
    opt.set_two_loop_mode(dzo.TWOLOOP_GRAM if mode is None else mode)
    return opt, ref, prob


def _sync(opt, ref):
    """The oracle's state into the device: point, gradient, objective value, history, rho, iteration count, last step length."""
    opt.current_point.upload(ref.current_point)
    opt.current_gradient.upload(ref.current_gradient)
    opt.set_objective_value(ref.current_objective_value)
    S, Y = ref.history_arrays()
    opt.set_history(S, Y, ref.rho_history, iteration_count=ref.iteration_count)
    opt.set_last_step_length(ref.last_step_length)


def _same_step(opt, ref, tol=1e-10):
    assert opt.is_stuck == ref.is_stuck and opt.iteration_count == ref.iteration_count
    assert opt.last_trials == ref.last_trials
    assert opt.history_count == ref.history_count
    assert opt.last_step_kind == ref.last_step_kind
    assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-12
    assert abs(opt.current_objective_value - ref.current_objective_value) <= 1e-12 * max(abs(ref.current_objective_value), 1e-300)
    if not ref.is_stuck:
        assert rel(opt.delta_point.to_host(), ref.delta_point) <= tol
        assert rel(opt.delta_gradient.to_host(), ref.delta_gradient) <= 1e-9
        assert np.allclose(opt.rho_history, ref.rho_history, rtol=1e-9)


def oracle_follows(opt, ref):
    """The other direction: the device's state, read through the getters, installed into the oracle -- delta_point and
    delta_gradient included (fields a failed search must not touch).  Returns what was read (device_state)."""
    st = device_state(opt)
    k = st["k"]
    S = np.stack(st["S"]) if k else np.zeros((0, opt.n), opt.dtype)
    Y = np.stack(st["Y"]) if k else np.zeros((0, opt.n), opt.dtype)
    ref.install_state(st["x"], st["g"], st["f"], S, Y, st["rho"], st["count"])
    ref.delta_point[:] = st["dx"]
    ref.delta_gradient[:] = st["dg"]
    return st


def device_state(opt):
    """The fields a failed step must leave alone, read from the device."""
    k = opt.history_count
    return dict(x=opt.current_point.to_host(), g=opt.current_gradient.to_host(), f=opt.current_objective_value, k=k,
                S=[h.to_host() for h in opt.delta_point_history], Y=[h.to_host() for h in opt.delta_gradient_history],
                dx=opt.delta_point.to_host(), dg=opt.delta_gradient.to_host(), count=opt.iteration_count, rho=opt.rho_history[:k].copy())


def assert_nothing_moved(opt, ref, before):
    """After a stuck exit: point, gradient, objective value, history, delta_point and delta_gradient are bit for bit what the
    step started from and what the oracle holds; one more step!() changes nothing (:456-458)."""
    for _ in range(2):
        now = device_state(opt)
        assert opt.is_stuck and ref.is_stuck
        assert now["count"] == before["count"] == ref.iteration_count and now["k"] == before["k"] == ref.history_count
        assert now["f"] == before["f"] == ref.current_objective_value
        for key, ours in (("x", ref.current_point), ("g", ref.current_gradient), ("dx", ref.delta_point), ("dg", ref.delta_gradient)):
            assert np.array_equal(now[key], before[key], equal_nan=True), key
            assert np.array_equal(now[key], ours, equal_nan=True), key
        for i in range(before["k"]):
            assert np.array_equal(now["S"][i], before["S"][i], equal_nan=True) and np.array_equal(now["S"][i], ref.S(i), equal_nan=True), i
            assert np.array_equal(now["Y"][i], before["Y"][i], equal_nan=True) and np.array_equal(now["Y"][i], ref.Y(i), equal_nan=True), i
        assert np.array_equal(now["rho"], before["rho"], equal_nan=True)
        opt.step(); ref.step()


def same_step(opt, ref, ref_p, kind, x_old, g_old, safeguards=False):
    """One accepted (or stuck) step of both sides from identical state: the comparisons of the module docstring.  The counters
    are compared by the caller (it may excuse a step)."""
    dtype = np.dtype(opt.dtype)
    assert opt.history_count == ref.history_count
    assert opt.last_step_kind == ref.last_step_kind
    if safeguards:
        assert opt.history_resets == ref.history_resets and opt.descent_resets == ref.descent_resets
    x_new, g_new = opt.current_point.to_host(), opt.current_gradient.to_host()
    if ref.is_stuck:
        assert np.array_equal(x_new, x_old) and np.array_equal(g_new, g_old)
        return
    if dtype == np.float64:
        _same_step(opt, ref)
        if safeguards:
            assert abs(opt.last_step_length - ref.last_step_length) <= 1e-12 * ref.last_step_length
    else:
        e_d = rel(opt.step_direction.to_host(), ref.step_direction)
        assert e_d <= 2e-4, e_d
        moved_by = np.linalg.norm(ref.delta_point.astype(np.float64)) / max(np.linalg.norm(ref.current_point.astype(np.float64)), 1e-300)
        assert rel(x_new, ref.current_point) <= max(1e-6, 2 * e_d * max(1.0, moved_by))
        assert abs(opt.current_objective_value - ref.current_objective_value) <= 1e-5 * abs(ref.current_objective_value)
        if safeguards:
            # the fp64 sum of the device's own dx^2 rounded to fp32 (u / 2 after the root), then sqrtf (u): within 2 u, u = 2^-24
            own = math.sqrt(math.fsum(opt.delta_point.to_host().astype(np.float64) ** 2))
            assert abs(opt.last_step_length - own) <= 2 * 2.0 ** -24 * own
    dx, dg = opt.delta_point.to_host(), opt.delta_gradient.to_host()
    assert np.array_equal(dx, x_new - x_old)
    assert np.array_equal(dg, g_new - g_old)
    if kind == "lse":
        g_ref = ref_p.grad(x_new).astype(np.float64)
        terms = np.linalg.norm(1e-2 * (x_new.astype(np.float64) - lse_centre(len(x_new), dtype).astype(np.float64))) + np.linalg.norm(g_ref)
        assert np.linalg.norm(g_new.astype(np.float64) - g_ref) <= (1e-13 if dtype == np.float64 else 1e-5) * terms
    else:
        assert np.array_equal(g_new, ref_p.grad(x_new))
    value, bound = rho_bound(dx, dg, dtype)
    assert abs(opt.rho_history[0] - value) <= bound, (opt.rho_history[0], value, bound)
