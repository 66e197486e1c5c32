"""GPU parity tests for the L-BFGS hot path, through the C ABI (include/dzo.h).

Bars: elementwise work (trial point, delta_point, delta_gradient, gradient kernel) is
BIT-EXACT against the oracle; reductions (dot products, objective sums) are fp64 and checked
to a stated relative tolerance, because the reference's own reduction order (BLAS) is not
defined; the two-loop direction is within 1e-10 relative L2 of the CPU oracle on identical
inputs (BASELINE.json north_star), for both device implementations (CHAIN and GRAM).
"""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from dzo_loader import dzo
from oracle import mp_twoloop, oracle as orc

pytestmark = pytest.mark.gpu

TOL_DIRECTION = 1e-10      # north_star: per-step output within 1e-10 relative of the CPU reference
TOL_DOT = 1e-13            # fp64 two-stage tree vs sequential sum, relative to sum |a_i b_i|


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _frozen(n, k, m, dtype=np.float64, mode=dzo.TWOLOOP_GRAM):
    """Optimizer whose state is the SURVEY 8(d) frozen two-loop inputs."""
    g, S, Y = orc.frozen_two_loop_state(n, k, dtype)
    x = dzo.DeviceArray.from_host(np.zeros(n, dtype))
    gd = dzo.DeviceArray.from_host(g if n else g)
    opt = dzo.LBFGSOptimizer(None, lambda x: 0.0, lambda g_, x_: None, x, 0.0, gd, 1.0, m)
    opt.set_two_loop_mode(mode)
    if k:
        rho = np.array([orc.dot(S[i].copy(), Y[i].copy()) for i in range(k)])
        opt.set_history(S, Y, rho)
    else:
        rho = np.zeros(0)
    return opt, g, S, Y, rho, (x, gd)


# ------------------------------------------------------------------------------ primitives
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1_000_001])
def test_primitives_match_oracle(n, dtype):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    dx, dy = dzo.DeviceArray.from_host(x), dzo.DeviceArray.from_host(y)
    a = dtype(0.37)
    # axpy / axpby / rmul / trial point: elementwise, bit-exact
    want = y.copy(); orc.axpy(float(a), x, want)
    assert np.array_equal(dzo.axpy_(float(a), dx, dy).to_host(), want)
    want2 = want.copy(); orc.axpby(1.0, x, -1.0, want2)
    assert np.array_equal(dzo.axpby_(1.0, dx, -1.0, dy).to_host(), want2)
    want3 = want2.copy(); orc.scal(want3, float(a))
    assert np.array_equal(dzo.rmul_(dy, float(a)).to_host(), want3)
    dst = dzo.DeviceArray(n, dtype)
    assert np.array_equal(dzo.trial_point_(dst, float(a), dx, dy).to_host(), _fma(a, x, want3, dtype))
    # reductions: fp64 accumulation on the device
    exact = float(np.dot(x.astype(np.longdouble), want3.astype(np.longdouble)))
    scale = float(np.abs(x.astype(np.float64) * want3.astype(np.float64)).sum())
    assert abs(dzo.dot(dx, dy) - exact) <= TOL_DOT * scale
    assert abs(dzo.norm(dx) - np.sqrt(float(np.dot(x.astype(np.longdouble), x.astype(np.longdouble))))) <= \
        (1e-6 if dtype == np.float32 else 1e-14) * np.linalg.norm(x.astype(np.float64))
    assert dzo.isequal(dx, dx.copy())
    assert np.array_equal(dzo.fill_(dst, 2.5).to_host(), np.full(n, 2.5, dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 3, 64, 65, 1001, 100_003])
def test_legacy_kernel_primitives_a14(n, dtype):
    """legacy/Kernels.jl:49-55 norm2 (sum of squares, NOT the root), :141 inv_norm = rsqrt(norm2),
    :76-83 negate!, :96-104 out-of-place scale!: elementwise ones bit-exact, reductions to the fp64 sum."""
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal(n).astype(dtype)
    if n > 1:
        x[0] = dtype(0.0)
    dx = dzo.DeviceArray.from_host(x)
    exact = float(np.dot(x.astype(np.longdouble), x.astype(np.longdouble)))
    tol = 1e-6 if dtype == np.float32 else 1e-14
    assert abs(dzo.norm2(dx) - exact) <= tol * exact
    assert abs(dzo.inv_norm(dx) - 1.0 / np.sqrt(exact)) <= tol / np.sqrt(exact)
    assert dzo.norm2(dx) == pytest.approx(dzo.norm(dx) ** 2, rel=4 * tol)           # norm2 is the SQUARE
    dst = dzo.DeviceArray(n, dtype)
    a = dtype(-1.7)
    assert np.array_equal(dzo.scale_(dst, float(a), dx).to_host(), a * x)           # dst = alpha * x
    assert np.array_equal(dx.to_host(), x)                                           # x untouched
    assert np.array_equal(dzo.scale_(dx, float(a), dx).to_host(), a * x)             # dst may alias x
    dx.upload(x)
    neg = dzo.negate_(dx).to_host()
    assert np.array_equal(neg, -x) and np.array_equal(np.signbit(neg), ~np.signbit(x))   # incl. -(+0.0) = -0.0
    assert dzo.inv_norm(dzo.DeviceArray.zeros(4, dtype)) == np.inf                   # rsqrt(0)


def _fma(a, x, y, dtype):
    out = y.copy()
    orc.axpy(float(a), x, out)     # oracle axpy IS fma(a, x, y)
    return out


def test_isequal_semantics_and_unaligned_views():
    a = np.array([1.0, np.nan, 0.0, 5.0, 7.0])
    da = dzo.DeviceArray.from_host(a)
    assert dzo.isequal(da, da.copy())                        # NaN equals NaN
    b = a.copy(); b[2] = -0.0
    assert not dzo.isequal(da, dzo.DeviceArray.from_host(b))  # -0.0 differs from +0.0
    # views that start 8 bytes into an allocation exercise the scalar (non 16-B) paths
    n = 1001
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(n + 1), rng.standard_normal(n + 1)
    dx, dy = dzo.DeviceArray.from_host(x), dzo.DeviceArray.from_host(y)
    vx, vy = dx.view(1, n), dy.view(1, n)
    want = y[1:].copy(); orc.axpy(0.5, x[1:].copy(), want)
    assert np.array_equal(dzo.axpy_(0.5, vx, vy).to_host(), want)
    assert abs(dzo.dot(vx, vy) - float(np.dot(x[1:], want))) <= 1e-12 * np.abs(x[1:] * want).sum()


# ------------------------------------------------------------------------------ problems (K12)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 64, 65, 1000, 100_003])
def test_rosenbrock_chain_kernels(n, dtype):
    x = orc.rosenbrock_chain_x0(n, dtype)
    ref = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype)
    p = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype)
    dx = dzo.DeviceArray.from_host(x)
    g = p.gradient_(dzo.DeviceArray(n, dtype), dx).to_host()
    assert np.array_equal(g, ref.grad(x))                     # elementwise: bit-exact
    f_ref = ref.eval(x)
    assert abs(p(dx) - f_ref) <= (1e-6 if dtype == np.float32 else 1e-13) * abs(f_ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 100_003])
def test_chained_quadratic_kernels(n, dtype):
    x = (orc.pcg_fill(n, 7) * 2).astype(dtype)
    ref = orc.Problem(orc.QUADRATIC_CHAIN, n, dtype, lam=0.25)
    p = dzo.Problem(dzo.QUADRATIC_CHAIN, n, dtype, lam=0.25)
    dx = dzo.DeviceArray.from_host(x)
    assert np.array_equal(p.gradient_(dzo.DeviceArray(n, dtype), dx).to_host(), ref.grad(x))     # elementwise: bit-exact
    f_ref = ref.eval(x)
    assert abs(p(dx) - f_ref) <= (1e-6 if dtype == np.float32 else 1e-13) * abs(f_ref)
    with pytest.raises(Exception):
        dzo.Problem(dzo.QUADRATIC_CHAIN, n, dtype, lam=0.0)


def test_rosenbrock2d_quadratic_lse_kernels():
    x = orc.pcg_fill(2, 1)
    p2, r2 = dzo.Problem(dzo.ROSENBROCK2D, 2), orc.Problem(orc.ROSENBROCK2D, 2)
    dx = dzo.DeviceArray.from_host(x)
    assert p2(dx) == r2.eval(x)
    assert np.array_equal(p2.gradient_(dzo.DeviceArray(2), dx).to_host(), r2.grad(x))
    for n in (8, 63, 256):
        A = orc.quadratic_matrix(n)
        x = orc.pcg_fill(n, 4) - 0.5
        pq, rq = dzo.Problem(dzo.QUADRATIC, n, A=A), orc.Problem(orc.QUADRATIC, n, A=A)
        dx = dzo.DeviceArray.from_host(x)
        assert abs(pq(dx) - rq.eval(x)) <= 1e-13 * abs(rq.eval(x))
        assert rel(pq.gradient_(dzo.DeviceArray(n), dx).to_host(), rq.grad(x)) <= 1e-14
    n = 5000
    c = orc.pcg_fill(n, 6) - 0.5
    x = (orc.pcg_fill(n, 8) - 0.5) * 3
    for dtype, tol in ((np.float64, 1e-13), (np.float32, 2e-6)):
        pl = dzo.Problem(dzo.LSE, n, dtype, c=c.astype(dtype), lam=1e-2)
        rl = orc.Problem(orc.LSE, n, dtype, c=c.astype(dtype), lam=1e-2)
        dx = dzo.DeviceArray.from_host(x.astype(dtype))
        assert abs(pl(dx) - rl.eval(x.astype(dtype))) <= tol * abs(rl.eval(x.astype(dtype)))
        assert rel(pl.gradient_(dzo.DeviceArray(n, dtype), dx).to_host().astype(np.float64),
                   rl.grad(x.astype(dtype)).astype(np.float64)) <= tol * 10


# ------------------------------------------------------------------------------ two-loop (K1)
@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 100_003])
@pytest.mark.parametrize("k,m", [(0, 4), (1, 4), (3, 4), (4, 4), (20, 20)])
def test_two_loop_direction_matches_oracle(n, k, m, mode):
    opt, g, S, Y, rho, _keep = _frozen(n, k, m, mode=mode)
    d_gpu = opt.compute_step_direction().to_host()
    d_ref, alpha_ref = orc.lbfgs_direction(g, S, Y, rho)
    if k == 0:
        assert np.array_equal(d_gpu, g)                       # :438 plain copy, no scaling (:443)
        return
    assert rel(d_gpu, d_ref) <= TOL_DIRECTION
    assert np.allclose(opt.alpha_history[:k], alpha_ref, rtol=1e-9, atol=1e-13 * np.abs(alpha_ref).max())
    # and against the wide-accumulator oracle (closest to the exact value)
    orc.set_dot_mode(orc.DOT_WIDE)
    try:
        d_wide, _ = orc.lbfgs_direction(g, S, Y, rho)
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)
    assert rel(d_gpu, d_wide) <= TOL_DIRECTION


@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
def test_two_loop_against_mpmath_arbiter(mode):
    n, k = 257, 6
    opt, g, S, Y, rho, _keep = _frozen(n, k, 8, mode=mode)
    d_gpu = opt.compute_step_direction().to_host()
    d_mp, _ = mp_twoloop.two_loop(g, S, Y, rho)
    d_ref, _ = orc.lbfgs_direction(g, S, Y, rho)
    assert rel(d_gpu, d_mp) <= 1e-12
    assert rel(d_ref, d_mp) <= 1e-12


@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
def test_two_loop_fp32_against_fp64_oracle(mode):
    n, k = 10_001, 10
    opt, g, S, Y, rho, _keep = _frozen(n, k, 10, dtype=np.float32, mode=mode)
    d_gpu = opt.compute_step_direction().to_host().astype(np.float64)
    d64, _ = orc.lbfgs_direction(g.astype(np.float64), S.astype(np.float64), Y.astype(np.float64),
                                 rho.astype(np.float64))
    # mixed-precision tolerance (config 4): elementwise fp32 fma chain of 2k+1 terms
    assert rel(d_gpu, d64) <= 2e-6 * np.sqrt(2 * k + 1)


def test_two_loop_is_deterministic_and_modes_agree():
    n, k = 50_001, 7
    outs = []
    for mode in (dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM):
        opt, *_ , _keep = _frozen(n, k, 8, mode=mode)
        a = opt.compute_step_direction().to_host()
        b = opt.compute_step_direction().to_host()
        assert np.array_equal(a, b)                           # run-twice bitwise equality
        outs.append(a)
    assert rel(outs[0], outs[1]) <= 1e-12


# ------------------------------------------------------------------------------ step! (K2-K7)
def _gpu_and_oracle(n, m, dtype=np.float64, mode=dzo.TWOLOOP_GRAM):
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype), x0.copy(), 1.0, m)
    prob = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype)
    opt = dzo.LBFGSOptimizer(None, prob, None, dzo.DeviceArray.from_host(x0), 1.0, m)
    opt.set_two_loop_mode(mode)
    return opt, ref, prob


def test_constructor_state_matches_reference_init():
    n, m = 1000, 5
    opt, ref, _ = _gpu_and_oracle(n, m)
    assert np.array_equal(opt.current_gradient.to_host(), ref.current_gradient)
    assert abs(opt.current_objective_value - ref.current_objective_value) <= 1e-13 * ref.current_objective_value
    assert rel(opt.step_direction.to_host(), ref.step_direction) <= 1e-15     # -step*g/|g| (:386-387)
    assert not opt.delta_point.to_host().any() and not opt.delta_gradient.to_host().any()
    assert opt.history_count == 0 and opt.iteration_count == 0 and not opt.is_stuck
    assert opt.current_point.ptr == opt.current_point_array.ptr               # aliasing (:393)
    with pytest.raises(AssertionError):                                       # :380 @assert
        dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, 8), None,
                           dzo.DeviceArray.from_host(orc.rosenbrock_chain_x0(8)), -1.0, 3)


def _sync_from_oracle(opt, ref):
    """Upload the oracle's complete state into the GPU optimizer ("state
    uploaded from the CPU restatement each checked step, so trajectories cannot diverge")."""
    opt.current_point.upload(ref.current_point)
    opt.current_gradient.upload(ref.current_gradient)
    opt.set_objective_value(ref.current_objective_value)
    S, Y = ref.history_arrays()
    opt.set_history(S, Y, ref.rho_history, iteration_count=ref.iteration_count)


@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
@pytest.mark.parametrize("n,m,steps", [(2, 3, 60), (1000, 5, 80), (4099, 20, 80)])
def test_each_step_matches_oracle_on_identical_state(n, m, steps, mode):
    """Per-step parity: every step!() starts from the oracle's state and must reproduce the
    oracle's next state.  L-BFGS on a non-convex objective amplifies last-bit differences
    of the dot products from step to step, so free-running trajectories of ANY two
    implementations with different reduction orders drift apart (see the free-running test)."""
    opt, ref, _ = _gpu_and_oracle(n, m, mode=mode)
    worst = 0.0
    for it in range(steps):
        _sync_from_oracle(opt, ref)
        opt.step(); ref.step()
        assert opt.is_stuck == ref.is_stuck and opt.iteration_count == ref.iteration_count
        if ref.is_stuck:
            break
        e = rel(opt.step_direction.to_host(), ref.step_direction)
        worst = max(worst, e)
        assert e <= TOL_DIRECTION, (it, e)
        assert opt.last_trials == ref.last_trials, it
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-12, it
        assert abs(opt.current_objective_value - ref.current_objective_value) <= 1e-12 * abs(ref.current_objective_value)
        assert rel(opt.delta_point.to_host(), ref.delta_point) <= TOL_DIRECTION
        assert rel(opt.delta_gradient.to_host(), ref.delta_gradient) <= 1e-9
        assert opt.history_count == ref.history_count
        assert np.allclose(opt.rho_history, ref.rho_history, rtol=1e-9)
    print(f"worst per-step direction error n={n} m={m}: {worst:.3e}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("edge", ["full", "plus1", "minus1"])
@pytest.mark.parametrize("U", [1, 2, 4])
def test_gram_and_combine_match_the_oracle_at_their_tile_edges(U, edge, dtype, monkeypatch):
    """The same per-step parity on the two-pass kernels (DZO_TUNE_SINGLE_PASS=0: Gram pass + combine pass over the slabs) at the
    sizes where their tiling changes.  A tile is 256 U vectors of 16 bytes; the host starts from U = 4 and halves it while
    ceil(n / tile) < 4 CUs, so t = 4 CUs tiles is the smallest count at which a U is kept.  n = t tile: full tiles only, all on
    the predicate-free path; + 1: a ragged tile of one element (fp64: one scalar-tail element); + tile - 1: a ragged tile one
    element short of full.  The oracle takes one step of its own first, so the three checked steps start from 1, 2 and 3 pairs:
    the pair loop's "one pair left", "two pairs left" and steady-state bodies.  Tolerances: those of the test above; fp32 those
    of the point ring's per-step test (the device sums in fp64, so the oracle does too)."""
    monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", "0")
    tile = 256 * U * (16 // np.dtype(dtype).itemsize)
    t = 4 * dzo.device_info()["compute_units"]
    n = t * tile + {"full": 0, "plus1": 1, "minus1": tile - 1}[edge]
    for u in (4, 2):                                      # the halving loop ends at this U
        assert (-(-n // (256 * u * (16 // np.dtype(dtype).itemsize))) >= t) == (u <= U), (n, u)
    m = 3
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        opt, ref, _ = _gpu_and_oracle(n, m, dtype)
        assert opt.ring_layout == 0
        ref.step()
        tol_d, tol_x, tol_f = (TOL_DIRECTION, 1e-12, 1e-12) if dtype == np.float64 else (2e-4, 1e-6, 1e-5)
        for it in range(3):
            _sync_from_oracle(opt, ref)
            assert opt.history_count == it + 1
            opt.step(); ref.step()
            assert opt.is_stuck == ref.is_stuck and not ref.is_stuck and opt.iteration_count == ref.iteration_count
            e_d = rel(opt.step_direction.to_host().astype(np.float64), ref.step_direction.astype(np.float64))
            x_new = opt.current_point.to_host()
            e_x = rel(x_new.astype(np.float64), ref.current_point.astype(np.float64))
            e_f = abs(opt.current_objective_value - ref.current_objective_value) / abs(ref.current_objective_value)
            print(f"{np.dtype(dtype).name} U={U} n={n} step {it}: d {e_d:.3e} x {e_x:.3e} f {e_f:.3e} trials {opt.last_trials}/{ref.last_trials}")
            assert e_d <= tol_d, it
            assert opt.last_trials == ref.last_trials, it
            moved_by = np.linalg.norm(ref.delta_point.astype(np.float64)) / np.linalg.norm(ref.current_point.astype(np.float64))
            assert e_x <= (tol_x if dtype == np.float64 else max(tol_x, 2 * e_d * max(1.0, moved_by))), it
            assert e_f <= tol_f, it
            assert np.array_equal(opt.current_gradient.to_host(), ref.problem.grad(x_new)), it     # elementwise: bit-exact
        assert opt.ring_layout == 0 and opt.single_pass_steps == 0
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
def test_free_running_trajectory_stays_close_then_converges(mode):
    n, m = 1000, 5
    opt, ref, _ = _gpu_and_oracle(n, m, mode=mode)
    for it in range(10):                                   # early steps: still within 1e-10
        opt.step(); ref.step()
        assert rel(opt.step_direction.to_host(), ref.step_direction) <= TOL_DIRECTION, it
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-11, it
        assert opt.last_trials == ref.last_trials and opt.history_count == ref.history_count
    steps = 10
    while not opt.is_stuck and steps < 20000:
        opt.step(); steps += 1
    assert opt.is_stuck and opt.current_objective_value < 1e-20
    assert np.allclose(opt.current_point.to_host(), 1.0, atol=1e-9)


def test_run_and_test_invariants_on_device():
    """legacy/DZOptimization.jl:998-1049 -- exact equalities hold on the GPU path too."""
    n, m = 130, 6
    opt, _, prob = _gpu_and_oracle(n, m)
    ref_p = orc.Problem(orc.ROSENBROCK_CHAIN, n)
    prev_x, prev_g = opt.current_point.to_host(), opt.current_gradient.to_host()
    for it in range(5000):
        opt.step()
        x, g = opt.current_point.to_host(), opt.current_gradient.to_host()
        if opt.is_stuck:
            assert np.array_equal(x, prev_x) and np.array_equal(g, prev_g)      # :1039,:1046
            break
        assert opt.iteration_count == it + 1                                     # :1013-1015
        assert np.array_equal(x - prev_x, opt.delta_point.to_host())            # :1035-1039 exact
        assert np.array_equal(g - prev_g, opt.delta_gradient.to_host())         # :1042-1046 exact
        assert np.array_equal(ref_p.grad(x), g)                                  # :1025-1032 exact
        assert abs(ref_p.eval(x) - opt.current_objective_value) <= 1e-13 * abs(opt.current_objective_value)
        # newest history pair IS the last deltas (:483,:491), rho[1] = s.y (:505)
        assert np.array_equal(opt.delta_point_history[0].to_host(), x - prev_x)
        assert np.array_equal(opt.delta_gradient_history[0].to_host(), g - prev_g)
        s, y = x - prev_x, g - prev_g
        assert abs(opt.rho_history[0] - float(np.dot(s, y))) <= 1e-12 * np.abs(s * y).sum()
        prev_x, prev_g = x, g
    assert opt.is_stuck and opt.current_objective_value < 1e-10
    assert opt.history_count == m


def test_callback_path_equals_builtin_path():
    """objective / gradient supplied as host callbacks (the reference's plugin boundary)."""
    n, m = 300, 4
    x0 = orc.rosenbrock_chain_x0(n)
    ref_p = orc.Problem(orc.ROSENBROCK_CHAIN, n)
    calls = {"f": 0, "g": 0, "c": 0}

    def objective(x):
        calls["f"] += 1
        return ref_p.eval(x.to_host())

    def gradient(g, x):
        calls["g"] += 1
        g.upload(ref_p.grad(x.to_host()))

    def constraint(x):
        calls["c"] += 1
        return True

    a = dzo.LBFGSOptimizer(constraint, objective, gradient, dzo.DeviceArray.from_host(x0), 1.0, m)
    ref = orc.LBFGS(ref_p, x0.copy(), 1.0, m)
    for it in range(25):
        _sync_from_oracle(a, ref)
        a.step(); ref.step()
        assert rel(a.current_point.to_host(), ref.current_point) <= 1e-12
        assert a.current_objective_value == pytest.approx(ref.current_objective_value, rel=1e-12)
        assert np.array_equal(a.current_gradient.to_host(), ref_p.grad(a.current_point.to_host()))
        assert a.last_trials == ref.last_trials
    assert calls["f"] >= 26 and calls["g"] == 26 and calls["c"] >= 26


@pytest.mark.parametrize("n", [4100, 4099, 100_003])
def test_deferred_tail_in_the_gram_pass_gives_the_same_run(n, monkeypatch):
    """DZO_TUNE_GENERIC_POST=2 (off by default: measured slower, DESIGN round-4 table row 2): on the general path the accepted
    step's delta_point / delta_gradient / rho are formed by the NEXT step's Gram pass on its way (gram_pass_lanes_kernel<POST>)
    -- or, when somebody looks first, by lbfgs_flush_post.  Same elementwise values; rho is summed in another order, so two
    free runs agree to rounding.  Run A never looks between steps (every tail rides in a Gram pass), run B looks after every
    step (every tail is flushed), run C is the default."""
    m = 4
    x0 = orc.rosenbrock_chain_x0(n)

    def run(knob, look):
        monkeypatch.setenv("DZO_TUNE_GENERIC_POST", str(knob))
        prob = dzo.Problem(dzo.ROSENBROCK_CHAIN, n)
        opt = dzo.LBFGSOptimizer(None, prob.native_callbacks(), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        trials = []
        for _ in range(m + 6):
            opt.step()
            trials.append(opt.last_trials)
            if look:
                s0 = opt.delta_point.to_host(); y0 = opt.delta_gradient.to_host()
                assert np.array_equal(s0, opt.delta_point_history[0].to_host()) and np.array_equal(y0, opt.delta_gradient_history[0].to_host())
                assert opt.rho_history[0] == pytest.approx(float(s0 @ y0), rel=1e-12)
        x, g = opt.current_point.to_host(), opt.current_gradient.to_host()
        S = np.stack([h.to_host() for h in opt.delta_point_history]); rho = opt.rho_history.copy()
        assert np.array_equal(g, orc.Problem(orc.ROSENBROCK_CHAIN, n).grad(x))
        assert np.allclose(rho, [float(a @ b) for a, b in zip(S, np.stack([h.to_host() for h in opt.delta_gradient_history]))], rtol=1e-12, atol=0)
        return trials, x, opt.current_objective_value
    ta, xa, fa = run(2, False)
    tb, xb, fb = run(2, True)
    tc, xc, fc = run(1, False)
    assert ta == tb == tc
    assert rel(xa, xc) <= 1e-9 and rel(xb, xc) <= 1e-9
    assert fa == pytest.approx(fc, rel=1e-10) and fb == pytest.approx(fc, rel=1e-10)


def test_split_entry_points_reproduce_step(monkeypatch):
    n, m = 257, 3
    # (bit for bit: both on the two-pass kernels -- the split entry points are those kernels driven from the host, and
    # step!() would otherwise take the point pass, whose dot products are summed in another order)
    monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", "0")
    opt_a, _, prob = _gpu_and_oracle(n, m)
    opt_b, _, prob_b = _gpu_and_oracle(n, m)
    for _ in range(8):
        opt_a.step()
        # the same step driven from the host (what the Julia module does around its callbacks)
        if opt_b.iteration_count > 0:
            opt_b.compute_step_direction()
        opt_b.begin_search()
        t = 1.0
        while True:
            assert opt_b.trial(t)
            f_new = prob_b(opt_b.current_point)
            if f_new < opt_b.current_objective_value:
                opt_b.accept(f_new)
                break
            t *= 0.5
        opt_b.pre_gradient()
        prob_b.gradient_(opt_b.current_gradient, opt_b.current_point)
        opt_b.post_gradient()
        assert np.array_equal(opt_a.current_point.to_host(), opt_b.current_point.to_host())
        assert np.array_equal(opt_a.delta_gradient.to_host(), opt_b.delta_gradient.to_host())
        # step!() sums the objective inside the fused trial kernel, the host-driven loop calls the
        # stand-alone objective kernel: same terms, different summation order
        assert opt_a.current_objective_value == pytest.approx(opt_b.current_objective_value, rel=1e-14)
        opt_b.set_objective_value(opt_a.current_objective_value)
    assert np.array_equal(opt_a.rho_history, opt_b.rho_history)


def test_host_driven_trial_followed_by_a_speculative_step_on_the_same_optimizer():
    """The split entry points copy five result words into the pinned outcome buffer (no seal); the step!() after them waits
    on a SEALED outcome over words 0..5 of the same buffer (core_wait_decision): the decision kernel writes all six
    (ADVICE r3), so the mixture works whatever the copy left behind."""
    n, m = 4100, 4
    opt, ref, prob = _gpu_and_oracle(n, m)
    for _ in range(3):
        opt.step(); ref.step()
    # a host-driven step (what the Julia module does around its callbacks) ...
    opt.compute_step_direction(); opt.begin_search()
    t = 1.0
    while True:
        assert opt.trial(t)
        f_new = prob(opt.current_point)
        if f_new < opt.current_objective_value:
            opt.accept(f_new)
            break
        t *= 0.5
    opt.pre_gradient(); prob.gradient_(opt.current_gradient, opt.current_point); opt.post_gradient()
    ref.step()
    assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-11
    # ... then library-driven ones, whose decisions are read through the seal
    for _ in range(4):
        opt.step(); ref.step()
        assert opt.last_trials == ref.last_trials
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-9
    assert dzo.unsealed_first_reads() >= 0


def test_fused_and_speculative_step_equal_the_plain_kernel_sequence(monkeypatch):
    """The fused accept+gradient+delta kernel and the speculative (device-decided) tail are
    pure re-schedulings: from the same state one step gives bit-identical x, delta_point, g,
    delta_gradient; only rho's reduction order (grid) may differ in the last bits."""
    n, m = 4099, 5
    x0 = orc.rosenbrock_chain_x0(n)
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 1.0, m)
    for _ in range(7):
        ref.step()
    outs = []
    for fused, spec in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("DZO_TUNE_FUSED_POST", fused)
        monkeypatch.setenv("DZO_TUNE_SPECULATE", spec)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        _sync_from_oracle(opt, ref)
        opt.step()
        opt.step()          # a second step exercises the rotated ring after the fused push
        outs.append((opt.current_point.to_host(), opt.delta_point.to_host(), opt.current_gradient.to_host(),
                     opt.delta_gradient.to_host(), opt.current_objective_value, opt.rho_history, opt.last_trials))
    for o in outs[1:]:
        for a, b in zip(o[:4], outs[0][:4]):
            assert rel(a, b) <= 1e-13
        assert o[4] == pytest.approx(outs[0][4], rel=1e-13) and o[6] == outs[0][6]
        assert np.allclose(o[5], outs[0][5], rtol=1e-12)
    # first of the two steps is bit-identical across the three schedules
    firsts = []
    for fused, spec in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("DZO_TUNE_FUSED_POST", fused)
        monkeypatch.setenv("DZO_TUNE_SPECULATE", spec)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        _sync_from_oracle(opt, ref)
        opt.step()
        firsts.append((opt.current_point.to_host(), opt.delta_point.to_host(), opt.current_gradient.to_host(),
                       opt.delta_gradient.to_host()))
    for o in firsts[1:]:
        for a, b in zip(o, firsts[0]):
            assert np.array_equal(a, b)


def test_rejected_trials_with_speculation_leave_state_consistent():
    """Force halvings (huge initial step): every rejected trial's gated tail must be a no-op."""
    n, m = 1000, 3
    x0 = orc.rosenbrock_chain_x0(n)
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 1e4, m)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1e4, m)
    for it in range(6):
        _sync_from_oracle(opt, ref)
        if it == 0:
            opt.step_direction.upload(ref.step_direction)
        opt.step(); ref.step()
        assert opt.last_trials == ref.last_trials
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-12
        assert np.array_equal(opt.current_gradient.to_host(), ref.problem.grad(opt.current_point.to_host()))
        assert rel(opt.delta_gradient.to_host(), ref.delta_gradient) <= 1e-9
    assert ref.last_trials >= 1 and max(1, ref.last_trials) >= 1


@settings(max_examples=int(__import__('os').environ.get('DZO_FUZZ_EXAMPLES', '12')), deadline=None, derandomize=True)
@given(n=st.integers(1, 3000), m=st.integers(1, 7), warm=st.integers(0, 9), seed=st.integers(0, 1000),
       mode=st.sampled_from([0, 1]))
def test_property_single_step_parity_random_shapes(n, m, warm, seed, mode):
    """Ragged n (vector tails), warm-up (k < m) and wrapped rings (k = m after > m steps)."""
    x0 = (orc.pcg_fill(n, seed) - 0.5) * 2.0
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 0.5, m)
    for _ in range(warm):
        ref.step()
    if ref.is_stuck:
        return
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 0.5, m)
    opt.set_two_loop_mode(mode)
    _sync_from_oracle(opt, ref)
    if warm == 0:
        opt.step_direction.upload(ref.step_direction)
    opt.step(); ref.step()
    assert opt.is_stuck == ref.is_stuck
    if not ref.is_stuck:
        assert rel(opt.step_direction.to_host(), ref.step_direction) <= TOL_DIRECTION
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-11
        assert opt.history_count == ref.history_count and opt.last_trials == ref.last_trials


def test_stuck_semantics():
    n = 64
    p = dzo.Problem(dzo.ROSENBROCK_CHAIN, n)
    opt = dzo.LBFGSOptimizer(None, p, None, dzo.DeviceArray.from_host(np.ones(n)), 1.0, 3)
    assert opt.is_stuck and opt.has_terminated and opt.has_converged          # :382, three names
    assert not opt.step_direction.to_host().any()                             # :384
    opt.step()
    assert opt.iteration_count == 0
    # NaN direction: the reference would loop forever; bounded escape restores x
    opt2, _, _ = _gpu_and_oracle(100, 3)
    opt2.step_direction.upload(np.full(100, np.nan))
    opt2.set_max_halvings(6)
    x_before = opt2.current_point.to_host()
    opt2.step()
    assert opt2.is_stuck and np.array_equal(opt2.current_point.to_host(), x_before)


def test_fp32_lse_tolerance_study_config4_small():
    """Config 4 at reduced n: L-BFGS m=10 on log-sum-exp, fp32 on the GPU vs the fp64 oracle
    on the same trajectory start; reports the observed mixed-precision error."""
    n, m = 20_000, 10
    c = orc.pcg_fill(n, 6) - 0.5
    ref = orc.LBFGS(orc.Problem(orc.LSE, n, np.float64, c=c, lam=1e-2), np.zeros(n), 1.0, m)
    p32 = dzo.Problem(dzo.LSE, n, np.float32, c=c.astype(np.float32), lam=1e-2)
    opt = dzo.LBFGSOptimizer(None, p32, None, dzo.DeviceArray.from_host(np.zeros(n, np.float32)), 1.0, m)
    worst = 0.0
    for it in range(12):
        opt.step(); ref.step()
        if ref.is_stuck or opt.is_stuck:
            break
        ef = abs(opt.current_objective_value - ref.current_objective_value) / abs(ref.current_objective_value)
        worst = max(worst, ef)
    assert worst <= 5e-6, worst


@pytest.mark.parametrize("n", [20_000, 1_000_000])
def test_config4_lse_fp32_direction_per_step_against_the_fp64_oracle(n):
    """BASELINE config 4 at full size (n = 10^6, m = 10, fp32 on the GPU, log-sum-exp objective), from
    x0 = 3(u - 1/2) (seed 8).  Every step starts from the fp64 oracle's state rounded to fp32; the
    direction the GPU step used is compared with the fp64 oracle's.  Stated mixed-precision
    tolerance: 2e-6 sqrt(2k+1) (fp32 fma chain of 2k+1 terms on inputs rounded to fp32).

    The objective of SURVEY.md 8(d) is a near-sphere at this size (the softmax part of the Hessian has
    entries <= 1e-6, the quadratic part is lambda = 1e-2 on the diagonal), so the REFERENCE ALGORITHM
    itself terminates after 5-6 steps from any start (checked on the fp64 oracle for start scales 3 to
    1000): k never reaches m = 10 on this workload.  The full-history case at the same size and dtype
    is test_config4_full_history_direction_n1e6_fp32 below."""
    m = 10
    c = orc.pcg_fill(n, 6) - 0.5
    x0 = 3.0 * (orc.pcg_fill(n, 8) - 0.5)
    orc.set_threads(8)
    try:
        ref = orc.LBFGS(orc.Problem(orc.LSE, n, np.float64, c=c, lam=1e-2), x0.copy(), 1.0, m)
        p32 = dzo.Problem(dzo.LSE, n, np.float32, c=c.astype(np.float32), lam=1e-2)
        opt = dzo.LBFGSOptimizer(None, p32, None, dzo.DeviceArray.from_host(x0.astype(np.float32)), 1.0, m)
        worst_d = worst_f = 0.0
        compared = 0
        for it in range(2 * m + 6):
            _sync_from_oracle(opt, ref)
            k = ref.history_count
            opt.step(); ref.step()
            if ref.is_stuck or opt.is_stuck:
                break
            if it > 0:                                             # step 0 uses the constructor's direction
                e = rel(opt.step_direction.to_host().astype(np.float64), ref.step_direction)
                worst_d = max(worst_d, e)
                assert e <= 2e-6 * np.sqrt(2 * k + 1), (it, k, e)
                compared += 1
            if opt.last_trials == ref.last_trials:
                ef = abs(opt.current_objective_value - ref.current_objective_value) / abs(ref.current_objective_value)
                worst_f = max(worst_f, ef)
                assert rel(opt.current_point.to_host().astype(np.float64), ref.current_point) <= 5e-7
        print(f"config 4 (n = {n}): worst direction error {worst_d:.3e}, worst objective error {worst_f:.3e}, "
              f"{compared} directions compared, history length reached {ref.history_count}")
        # (the fp32 run stops earlier than the fp64 one: after two or three steps the objective has
        # converged to fp32 resolution and no trial decreases it any more)
        assert compared >= 2
        assert worst_f <= 5e-6
    finally:
        orc.set_threads(1)


@pytest.mark.parametrize("mode", [dzo.TWOLOOP_CHAIN, dzo.TWOLOOP_GRAM], ids=["chain", "gram"])
def test_config4_full_history_direction_n1e6_fp32(mode):
    """Config 4's two-loop at full size with a FULL history (n = 10^6, k = m = 10, fp32) on the frozen
    synthetic state of SURVEY.md 8(d), against the fp64 oracle on the same (fp32-representable) inputs."""
    n, k = 1_000_000, 10
    opt, g, S, Y, rho, _keep = _frozen(n, k, k, dtype=np.float32, mode=mode)
    d_gpu = opt.compute_step_direction().to_host().astype(np.float64)
    orc.set_threads(8)
    try:
        d64, _ = orc.lbfgs_direction(g.astype(np.float64), S.astype(np.float64), Y.astype(np.float64), rho.astype(np.float64))
    finally:
        orc.set_threads(1)
    e = rel(d_gpu, d64)
    print(f"config 4 two-loop, n = 1e6, k = 10, fp32 vs fp64 oracle: {e:.3e}")
    assert e <= 2e-6 * np.sqrt(2 * k + 1)
    assert np.array_equal(d_gpu, opt.compute_step_direction().to_host().astype(np.float64))   # deterministic


# ------------------------------------------------------------------------------ full size (C3)
def test_full_size_two_loop_n1e7_m20():
    """BASELINE config 3 at full size: frozen synthetic state, n = 10^7, m = k = 20, fp64.
    Size-independent properties plus the oracle itself (a few seconds of CPU)."""
    n, k = 10_000_000, 20
    opt, g, S, Y, rho, _keep = _frozen(n, k, k, mode=dzo.TWOLOOP_GRAM)
    d_gram = opt.compute_step_direction().to_host()
    assert np.array_equal(d_gram, opt.compute_step_direction().to_host())      # deterministic
    opt.set_two_loop_mode(dzo.TWOLOOP_CHAIN)
    d_chain = opt.compute_step_direction().to_host()
    assert rel(d_gram, d_chain) <= TOL_DIRECTION
    orc.set_threads(8)
    try:
        d_ref, _ = orc.lbfgs_direction(g, S, Y, rho)
    finally:
        orc.set_threads(1)
    assert rel(d_gram, d_ref) <= TOL_DIRECTION
    assert rel(d_chain, d_ref) <= TOL_DIRECTION
    # linearity in g: scaling by a power of two is exact in every operation
    opt.set_two_loop_mode(dzo.TWOLOOP_GRAM)
    opt.current_gradient.upload(4.0 * g)
    assert np.array_equal(opt.compute_step_direction().to_host(), 4.0 * d_gram)
    # secant property of the implicit inverse Hessian: H_k y_1 = s_1, so d(g = y_1) = -s_1
    opt.current_gradient.upload(Y[0])
    assert rel(opt.compute_step_direction().to_host(), -S[0]) <= 1e-9


# ------------------------------------------------------------------------------ LineSearchEvaluator (a6)
def test_line_search_evaluator_call_matches_oracle():
    """src/DZOptimization.jl:65-92: trial point, objective, Armijo and curvature quotients."""
    n = 2049
    x = orc.rosenbrock_chain_x0(n)
    ref_p = orc.Problem(orc.ROSENBROCK_CHAIN, n)
    g = ref_p.grad(x)
    d = -g / np.linalg.norm(g)
    overlap = float(g @ d)
    f0 = ref_p.eval(x)
    prob = dzo.Problem(dzo.ROSENBROCK_CHAIN, n)
    lse = dzo.LineSearchEvaluator(None, prob, None, dzo.DeviceArray.from_host(x), f0, dzo.DeviceArray.from_host(g),
                                  dzo.DeviceArray.from_host(d), overlap)
    for t, with_grad in ((1e-3, True), (0.05, False), (0.5, True)):
        f_new = lse(t, with_grad)
        f_ref, ir, sr, tp, tg = orc.line_search_eval(ref_p, x, f0, d, overlap, t, with_grad)
        assert np.array_equal(lse.trial_point.to_host(), tp)                       # fma(t, d, x): bit-exact
        assert f_new == pytest.approx(f_ref, rel=1e-13)
        assert lse.improvement_ratio == pytest.approx(ir, rel=1e-9)
        if with_grad:
            assert np.array_equal(lse.trial_gradient.to_host(), tg)
            assert lse.slope_ratio == pytest.approx(sr, rel=1e-10)
    # infeasible trial point (:71-79): typemax / typemin sentinels, objective not evaluated
    calls = []
    lse2 = dzo.LineSearchEvaluator(lambda x_: False, lambda x_: calls.append(1) or 0.0, None,
                                   dzo.DeviceArray.from_host(x), f0, dzo.DeviceArray.from_host(g),
                                   dzo.DeviceArray.from_host(d), overlap)
    assert lse2(0.1, False) == np.finfo(np.float64).max and not calls
    assert lse2.improvement_ratio == -np.finfo(np.float64).max
    with pytest.raises(AssertionError):                                             # :86 @assert
        lse2(0.1, True)


def test_full_size_step_run_config3_invariants():
    """BASELINE config 3 at full size (n = 10^7, m = 20, fp64): 120 step!() calls on the device;
    strict decrease every step, and the exact run_and_test! equalities at sampled steps."""
    n, m = 10_000_000, 20
    x0 = orc.rosenbrock_chain_x0(n)
    ref_p = orc.Problem(orc.ROSENBROCK_CHAIN, n)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
    f_prev = opt.current_objective_value
    assert f_prev == pytest.approx(ref_p.eval(x0), rel=1e-12)
    trials = 0
    for it in range(120):
        sample = it in (0, 19, 20, 21, 63, 119)                  # warm-up, ring wrap, steady state
        if sample:
            x_old, g_old = opt.current_point.to_host(), opt.current_gradient.to_host()
        opt.step()
        assert not opt.is_stuck
        f = opt.current_objective_value
        assert f < f_prev                                        # :139 strict decrease
        assert opt.delta_objective_value == pytest.approx(f - f_prev, rel=1e-9)
        f_prev = f
        trials += opt.last_trials
        if sample:
            x, g = opt.current_point.to_host(), opt.current_gradient.to_host()
            assert np.array_equal(x - x_old, opt.delta_point.to_host())          # :1035-1039 exact
            assert np.array_equal(g - g_old, opt.delta_gradient.to_host())       # :1042-1046 exact
            orc.set_threads(8)
            try:
                assert np.array_equal(ref_p.grad(x), g)                          # :1025-1032 exact
                assert abs(ref_p.eval(x) - f) <= 1e-12 * f                       # :1019-1022 (reduction order)
            finally:
                orc.set_threads(1)
            assert np.array_equal(opt.delta_point_history[0].to_host(), x - x_old)
            # step_direction (formed on demand by one more pass over the ring) is the direction the step really walked
            # along: x = fma(t, d, x_old) with t = 2^-(trials - 1) (:124; t d is exact, so numpy rounds once as the fma does);
            # its values against the oracle at this size: tests/test_gpu_lbfgs_scale.py
            d = opt.step_direction.to_host()
            assert np.array_equal(x, x_old + 0.5 ** (opt.last_trials - 1) * d)
            assert float(d @ g_old) < 0.0                                        # a descent direction
    assert opt.iteration_count == 120 and opt.history_count == m
    assert trials <= 2 * 120


def test_handles_release_their_device_memory():
    """Constructors allocate (rings, workspaces, streams); destroy must give everything back."""
    import gc
    import torch
    n, m = 1_000_000, 10
    x0 = orc.rosenbrock_chain_x0(n)

    def cycle():
        x = dzo.DeviceArray.from_host(x0)
        p = dzo.Problem(dzo.ROSENBROCK_CHAIN, n)
        o = dzo.LBFGSOptimizer(None, p, None, x, 1.0, m)
        for _ in range(3):
            o.step()
        b = dzo.BFGSOptimizer(dzo.Problem(dzo.ROSENBROCK_CHAIN, 256), None, dzo.DeviceArray.from_host(x0[:256]), 1.0)
        b.step()
        a = dzo.AdGDOptimizer(None, p, None, dzo.DeviceArray.from_host(x0), 0.1)
        a.step()
        bb = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, np.stack([x0[:64]] * 16), 1.0)
        bb.step(2)
        for h in (o, b, a, bb):
            h.close()
        del o, b, a, bb, p, x

    cycle(); gc.collect(); dzo.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    gc.collect(); dzo.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 64 << 20, f"leaked {(free0 - free1) >> 20} MiB over 20 create/destroy cycles"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 5, 127, 128, 129, 257, 4099, 100_003, 1_000_001])
def test_fused_trial_objective_kernel_equals_separate_kernels(n, dtype, monkeypatch):
    """DZO_TUNE_FUSED_TRIAL=1 (trial point + objective in one pass, edge terms in a second tiny
    kernel) is a re-scheduling: same x bit for bit, same objective up to summation order."""
    m = 3
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    outs = []
    for fused in ("0", "1"):
        monkeypatch.setenv("DZO_TUNE_FUSED_TRIAL", fused)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        trials = 0
        for _ in range(6):
            opt.step(); trials += opt.last_trials
        outs.append((opt.current_point.to_host(), opt.current_objective_value, trials, opt.current_gradient.to_host()))
    (xa, fa, ta, ga), (xb, fb, tb, gb) = outs
    assert ta == tb
    assert np.array_equal(xa, xb) and np.array_equal(ga, gb)
    assert fb == pytest.approx(fa, rel=1e-6 if dtype == np.float32 else 1e-13)


# ------------------------------------------------------------------------------ single-pass step
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,m", [(8, 1), (124, 3), (128, 5), (248, 4), (250, 2), (372, 6), (1000, 5), (4098, 20), (100_004, 7), (1_000_000, 10), (1_000_000, 20)])
def test_single_pass_step_hands_the_next_two_loop_its_dots(n, m, dtype):
    """The single-pass step (csrc/dzo_lbfgs.hip lbfgs_single_pass_kernel) also produces every dot
    product of the NEXT two-loop.  From identical state: step both sides, then ask both for the
    next direction -- the GPU one comes from those dots (reduce + finish + combine, no Gram pass)."""
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype), x0.copy(), 1.0, m)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
    # fp32: both sides round every elementwise op to fp32; the device accumulates its sums in fp64,
    # so the fp32 oracle runs in its wide-accumulator mode (fp64 sums) -- its default sequential fp32
    # sums lose ~sqrt(n) ulps and would not be a reference at n >= 1e5
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        _single_pass_handover_body(n, m, dtype, opt, ref)
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def _single_pass_handover_body(n, m, dtype, opt, ref):
    tol = 1e-3 if dtype == np.float32 else 1e-10
    checked = 0
    for it in range(3 * m + 12):
        _sync_from_oracle(opt, ref)
        opt.step(); ref.step()
        assert opt.is_stuck == ref.is_stuck
        if ref.is_stuck:
            break
        assert opt.last_trials == ref.last_trials
        S, Y = ref.history_arrays()
        want = orc.lbfgs_direction(ref.current_gradient.copy(), S, Y, ref.rho_history)[0]
        got = opt.compute_step_direction().to_host()
        assert rel(got.astype(np.float64), want.astype(np.float64)) <= tol, (it, opt.history_count)
        # rho of the pushed pair comes out of the same pass (s_p.y_p); arbiter: the fp64 dot of the
        # device's own deltas (the fp32 oracle sums sequentially in fp32)
        exact = float(np.dot(opt.delta_point.to_host().astype(np.float64), opt.delta_gradient.to_host().astype(np.float64)))
        assert opt.rho_history[0] == pytest.approx(exact, rel=2e-7 if dtype == np.float32 else 1e-11)
        checked += 1
    assert checked >= 3


def test_single_pass_and_two_pass_paths_agree_step_by_step(monkeypatch):
    """DZO_TUNE_SINGLE_PASS=0 restores the Gram pass + combine pass per step: from the same state
    both produce bit-identical x, delta_point, g, delta_gradient (d is the same elementwise
    recurrence given the same scalars; the scalars come from the same Gram pass here)."""
    n, m = 4098, 6
    x0 = orc.rosenbrock_chain_x0(n)
    ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 1.0, m)
    for _ in range(9):
        ref.step()
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", flag)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        _sync_from_oracle(opt, ref)
        opt.step()
        outs.append((opt.current_point.to_host(), opt.delta_point.to_host(), opt.current_gradient.to_host(),
                     opt.delta_gradient.to_host(), opt.step_direction.to_host(), opt.last_trials))
    for a, b in zip(outs[0][:5], outs[1][:5]):
        assert np.array_equal(a, b)
    assert outs[0][5] == outs[1][5]


def test_single_pass_free_run_matches_two_pass_free_run(monkeypatch):
    """Free run of 12 steps (dots handed from pass to pass, rejected trials included): both paths
    stay within rounding of each other, then both converge."""
    n, m = 1000, 5
    x0 = orc.rosenbrock_chain_x0(n)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", flag)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        xs, tr = [], []
        for _ in range(12):
            opt.step(); xs.append(opt.current_point.to_host()); tr.append(opt.last_trials)
        steps = 12
        while not opt.is_stuck and steps < 20000:
            opt.step(); steps += 1
        runs.append((xs, tr, opt.current_objective_value, opt.current_point.to_host()))
    assert runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert rel(a, b) <= 1e-10
    for r in runs:
        assert r[2] < 1e-20 and np.allclose(r[3], 1.0, atol=1e-9)


def test_single_pass_rejected_first_trials_follow_the_reference_loop():
    """When the single pass's t = 1 trial is rejected, x and g are untouched and the halving loop continues:
    with the same pass at t = 1/2 when the objective there (which rode along) is a decrease, on the trial
    kernels otherwise (one or more further trials); every such step must still reproduce the oracle's step
    from the same state."""
    n, m = 250, 3
    opt, ref, _ = _gpu_and_oracle(n, m)
    seen = set()
    for it in range(60):
        _sync_from_oracle(opt, ref)
        opt.step(); ref.step()
        assert opt.last_trials == ref.last_trials, it
        seen.add(opt.last_trials)
        assert rel(opt.current_point.to_host(), ref.current_point) <= 1e-12, it
        assert np.array_equal(opt.current_gradient.to_host(), orc.Problem(orc.ROSENBROCK_CHAIN, n).grad(opt.current_point.to_host()))
        assert rel(opt.delta_gradient.to_host(), ref.delta_gradient) <= 1e-9
        assert np.allclose(opt.rho_history, ref.rho_history, rtol=1e-9)
    assert opt.single_pass_steps >= 55
    assert opt.single_pass_rejections >= 3 and {1, 2}.issubset(seen)
    # a rejected first trial whose t/2 objective (carried by the pass) is a decrease is continued by the same pass
    # at t/2; deeper halvings go to the trial kernels
    assert 1 <= opt.single_pass_retries <= opt.single_pass_rejections


def test_history_longer_than_the_single_pass_limit_switches_paths_cleanly():
    """m = 26 > 24: the tile ring and the single-pass step are chosen at construction and only for m <= 24 (fp64; the point
    pass has a K = 24 instantiation on two register sets) / m <= 20 (fp32), so this optimizer runs the two-pass kernels
    throughout -- same steps as the oracle."""
    n, m = 1000, 26
    opt, ref, _ = _gpu_and_oracle(n, m)
    for it in range(40):
        opt.step(); ref.step()
        if it < 12:
            assert rel(opt.step_direction.to_host(), ref.step_direction) <= TOL_DIRECTION, it
            assert opt.last_trials == ref.last_trials
    assert opt.single_pass_steps == 0 and opt.history_count == m
    # per-step parity from synced state on both sides of the switch
    opt2, ref2, _ = _gpu_and_oracle(n, m)
    for it in range(30):
        _sync_from_oracle(opt2, ref2)
        opt2.step(); ref2.step()
        assert opt2.last_trials == ref2.last_trials, it
        assert rel(opt2.step_direction.to_host(), ref2.step_direction) <= TOL_DIRECTION, it
        assert rel(opt2.current_point.to_host(), ref2.current_point) <= 1e-12, it


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,m", [(4100, 5), (100_004, 20)])
def test_single_pass_twin_buffers_keep_the_callers_array_aliased(n, m, dtype, monkeypatch):
    """The single-pass step writes the trial point and its gradient into twin buffers and swaps roles on
    accept, so x0 -- which the optimizer ALIASES as current_point (src/DZOptimization.jl:393) -- holds
    the current point only after the library settled it.  K steps with no pointer access in between
    (odd and even K: the live copy ends in the twin / in x0), then the caller's own array, read WITHOUT
    going through the optimizer, must be the current point; the two-pass path from the same start gives
    the same trajectory."""
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    ref_p = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype)
    for K in (7, 8):
        runs = []
        for flag in ("1", "0"):
            monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", flag)
            xd = dzo.DeviceArray.from_host(x0)
            opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, xd, 1.0, m)
            trials = 0
            for _ in range(K):
                opt.step(); trials += opt.last_trials           # scalars only
            mine = xd.to_host()                                  # the caller's array, not opt.current_point
            assert np.array_equal(mine, opt.current_point.to_host())
            assert opt.current_point.ptr == xd.ptr               # still the same array (:393)
            assert np.array_equal(ref_p.grad(mine), opt.current_gradient.to_host())
            runs.append((mine, opt.current_objective_value, trials, opt.single_pass_steps))
            xd2 = dzo.DeviceArray.from_host(x0)                  # destroy also settles
            o2 = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, xd2, 1.0, m)
            for _ in range(K):
                o2.step()
            o2.close()
            assert np.array_equal(xd2.to_host(), mine)
        tol = 1e-10 if dtype == np.float64 else 1e-4
        assert runs[0][3] >= K - 2 and runs[1][3] == 0
        assert runs[0][2] == runs[1][2]
        assert rel(runs[0][0].astype(np.float64), runs[1][0].astype(np.float64)) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,m", [(16, 3), (2 * 62 * 3 + 12, 5), (100_004, 20)])
def test_blocked_ring_hands_out_the_pairs_as_plain_vectors(n, m, dtype):
    """Optimizers on the built-in chained Rosenbrock keep their (s, y) pairs tile-major (rows of 62 vectors
    plus a halo vector either side, DESIGN.md "blocked ring").  The reference's fields stay what they are
    (src/DZOptimization.jl:366-374): delta_point_history[i] / delta_gradient_history[i] are the deltas of
    step count-i, delta_point / delta_gradient the newest of them; set_history round-trips bit for bit;
    switching to the chain kernels converts the ring without changing a bit of it."""
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    prob = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype)

    def run():
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        xs, gs = [x0.copy()], [prob.grad(x0)]
        for it in range(m + 4):
            opt.step()
            if opt.is_stuck:
                break
            xs.append(opt.current_point.to_host()); gs.append(opt.current_gradient.to_host())
        return opt, xs, gs

    opt, xs, gs = run()
    steps = len(xs) - 1
    assert steps >= 3 and opt.single_pass_steps >= 1
    k = opt.history_count
    assert k == min(steps, m)

    def check(o):
        S = [h.to_host() for h in o.delta_point_history]
        Y = [h.to_host() for h in o.delta_gradient_history]
        for i in range(k):
            assert np.array_equal(S[i], xs[steps - i] - xs[steps - i - 1]), i
            assert np.array_equal(Y[i], gs[steps - i] - gs[steps - i - 1]), i
        return S, Y

    S, Y = check(opt)
    if not opt.is_stuck:
        assert np.array_equal(opt.delta_point.to_host(), S[0]) and np.array_equal(opt.delta_gradient.to_host(), Y[0])
    # round trip through set_history (row 0 = newest, as get_ptr's idx)
    opt.set_history(np.stack(S), np.stack(Y), opt.rho_history.copy(), iteration_count=opt.iteration_count)
    check(opt)
    opt.compute_step_direction()
    d_gram = opt.step_direction.to_host()
    opt.set_two_loop_mode(dzo.TWOLOOP_CHAIN)                  # leaves the tile-major layout
    check(opt)
    opt.compute_step_direction()
    tol = 1e-11 if dtype == np.float64 else 2e-4
    assert rel(opt.step_direction.to_host(), d_gram) <= tol
    # the same run, converted right after its last step: deltas and pairs survive the conversion
    opt2, xs2, _ = run()
    assert len(xs2) == len(xs) and np.array_equal(xs2[-1], xs[-1])
    opt2.set_two_loop_mode(dzo.TWOLOOP_CHAIN)
    check(opt2)
    if not opt2.is_stuck:
        assert np.array_equal(opt2.delta_point.to_host(), S[0]) and np.array_equal(opt2.delta_gradient.to_host(), Y[0])
    opt2.step()
    assert opt2.iteration_count == steps + 1 or opt2.is_stuck


# (m = 23: the K = 24 instantiation on two register sets, fp64 only -- fp32 keeps points up to m = 20)
# (ragged n -- not a multiple of the 16-byte vector: 2 elements in fp64, 4 in fp32 -- pads the last vector of every ring
# stream with phantom elements that stay +0; 125 = 62 * 2 + 1 puts a one-element vector alone into the third wave-row
# (fp64), 249 = 62 * 4 + 1 into the second (fp32); 4097 .. 4099 are the three fp32 remainders)
_POINT_RING_CASES = [(n, m, s0, dt) for dt in (np.float64, np.float32)
                     for n, m, s0 in [(16, 3, 1.0), (2 * 62 * 3 + 12, 5, 1.0), (4100, 20, 1.0), (100_004, 7, 1.0), (4100, 6, 300.0), (4100, 23, 1.0),
                                      (17, 3, 1.0), (125, 4, 1.0), (249, 4, 1.0), (385, 5, 1.0), (4097, 9, 1.0), (4098, 11, 1.0), (4099, 20, 1.0),
                                      (100_003, 7, 1.0), (4101, 6, 300.0), (4099, 23, 1.0), (4100, 21, 1.0), (4099, 22, 1.0)]
                     if not (dt == np.float32 and m > 20)]


@pytest.mark.parametrize("n,m,step0,dtype", _POINT_RING_CASES,
                         ids=[f"{np.dtype(dt).name}-n{n}-m{m}-{s0}" for n, m, s0, dt in _POINT_RING_CASES])
def test_point_ring_steps_match_the_oracle_from_the_same_state(n, m, step0, dtype):
    _point_ring_steps_against_the_oracle(n, m, step0, dtype, {})


# the decorators of legacy/DZOptimization.jl:219-296 ride on the point pass (its DEC instantiations): L2 term of the
# objective and of every recomputed gradient, the box-gradient mask, the box projection of the trial point
_DECOR_SETS = {
    "l2": dict(l2=0.01),
    "box": dict(box_gradient=(-1.1, 0.9), box_constraint=(-1.1, 0.9)),          # (the start point -1.2 / 1.0 +- 0.005 is projected: many active bounds)
    "all": dict(l2=0.01, box_gradient=(-0.25, 0.9), box_constraint=(-0.25, 0.9)),
    "mask_only": dict(box_gradient=(-1.0, 1.0)),                               # gradient mask without the projection
}
_POINT_RING_DECOR_CASES = [(n, m, s0, dt, dk) for dt in (np.float64, np.float32)
                           for n, m, s0, dk in [(16, 3, 1.0, "all"), (384, 5, 1.0, "l2"), (385, 5, 1.0, "box"), (4100, 20, 1.0, "all"), (4099, 12, 1.0, "all"),
                                                (4100, 7, 300.0, "box"), (100_004, 16, 1.0, "mask_only"), (4100, 23, 1.0, "all"), (4101, 10, 30.0, "l2")]
                           if not (dt == np.float32 and m > 20)]


@pytest.mark.parametrize("n,m,step0,dtype,decor", _POINT_RING_DECOR_CASES,
                         ids=[f"{np.dtype(dt).name}-n{n}-m{m}-{s0}-{dk}" for n, m, s0, dt, dk in _POINT_RING_DECOR_CASES])
def test_decorated_point_ring_steps_match_the_oracle_from_the_same_state(n, m, step0, dtype, decor):
    _point_ring_steps_against_the_oracle(n, m, step0, dtype, _DECOR_SETS[decor])


_QCHAIN_CASES = [(n, m, s0, dt) for dt in (np.float64, np.float32)
                 for n, m, s0 in [(16, 3, 1.0), (385, 5, 1.0), (4100, 20, 1.0), (4099, 8, 1.0), (100_004, 12, 1.0), (4100, 6, 300.0), (4100, 23, 1.0), (4098, 16, 30.0),
                                  (1001, 11, 30.0)]       # (the last: found by the fuzz -- a phantom gradient of -0 made the host-write check see a difference)
                 if not (dt == np.float32 and m > 20)]


@pytest.mark.parametrize("n,m,step0,dtype", _QCHAIN_CASES, ids=[f"{np.dtype(dt).name}-n{n}-m{m}-{s0}" for n, m, s0, dt in _QCHAIN_CASES])
def test_chained_quadratic_point_ring_steps_match_the_oracle_from_the_same_state(n, m, step0, dtype):
    """The second chained objective of the point pass (ChainObj<T, 1>, VERDICT r3 item 1c: the objective sits behind a
    device functor -- radius-1 stencil, per-element coefficients -- and the chained quadratic is its second instance):
    same protocol as the chained Rosenbrock cases, on a convex problem whose run ends at the minimiser."""
    _point_ring_steps_against_the_oracle(n, m, step0, dtype, {}, kind="qchain")


_LSE_CASES = [(n, m, s0, dt) for dt in (np.float64, np.float32)
              for n, m, s0 in [(16, 3, 1.0), (385, 5, 1.0), (4100, 10, 1.0), (4099, 20, 1.0), (100_004, 10, 1.0), (4100, 6, 300.0), (4100, 23, 1.0)]
              if not (dt == np.float32 and m > 20)]


@pytest.mark.parametrize("n,m,step0,dtype", _LSE_CASES, ids=[f"{np.dtype(dt).name}-n{n}-m{m}-{s0}" for n, m, s0, dt in _LSE_CASES])
def test_log_sum_exp_point_ring_steps_match_the_oracle_from_the_same_state(n, m, step0, dtype):
    """BASELINE configs[3]'s objective on the point ring: log sum exp(x) + lambda/2 |x - c|^2 needs two global
    scalars per point, so its step is a trial pass and a dots pass over the ring of points (lse_trial_kernel / lse_decide_kernel /
    lse_dots_kernel) instead of one sweep.  Same protocol as the other point-ring cases; the gradient is compared to rounding,
    not bit for bit (the sum of exponentials of an accepted point is carried relative to the previous point's maximum)."""
    _point_ring_steps_against_the_oracle(n, m, step0, dtype, {}, kind="lse")


def _point_ring_problem(n, dtype, decor, kind):
    """Start point, the oracle's and the device's problem, and the centre of the log-sum-exp cases (None otherwise)."""
    x0, cc = orc.rosenbrock_chain_x0(n, dtype), None
    if kind == "lse":
        cc = (orc.pcg_fill(n, 6) - 0.5).astype(dtype)                              # c = u - 1/2 (seed 6), lambda = 1e-2
        x0 = (0.5 * (orc.pcg_fill(n, 8) - 0.5)).astype(dtype)
        return x0, orc.Problem(orc.LSE, n, dtype, c=cc, lam=1e-2), dzo.Problem(dzo.LSE, n, dtype, c=cc, lam=1e-2), cc
    if kind == "qchain":
        return x0, orc.Problem(orc.QUADRATIC_CHAIN, n, dtype, lam=0.05), dzo.Problem(dzo.QUADRATIC_CHAIN, n, dtype, lam=0.05), cc
    return x0, orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype, **decor), dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype, **decor), cc


def _point_ring_steps_against_the_oracle(n, m, step0, dtype, decor, kind="rosen"):
    """The default optimizer on the built-in chained Rosenbrock keeps the last k + 1 POINTS and GRADIENTS tile-major
    (ring_layout == 2) and forms the pairs in registers; every trial of a step, the first step included, is one pass.
    The GPU optimizer runs free here (nothing is installed into it: that would turn its ring into the pair ring) and
    the ORACLE follows: before every step it is given the GPU's point, gradient, objective value and history -- read
    through the public getters, which gather them without leaving the point layout -- and both take the step.
    step0 = 300 makes first trials fail (several halvings, all on the same pass)."""
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)                    # the device sums in fp64
    try:
        x0, ref_p, dev_p, cc = _point_ring_problem(n, dtype, decor, kind)
        ref = orc.LBFGS(ref_p, x0.copy(), step0, m)
        opt = dzo.LBFGSOptimizer(None, dev_p, None, dzo.DeviceArray.from_host(x0), step0, m)
        assert opt.ring_layout == 2
        tol_d = TOL_DIRECTION if dtype == np.float64 else 2e-4
        tol_x = 1e-12 if dtype == np.float64 else 1e-6
        seen = set()
        box = decor.get("box_constraint")
        f0 = opt.current_objective_value
        for it in range(3 * m + 12):
            if kind == "lse" and it > 0 and abs(opt.delta_objective_value) <= (1e-13 if dtype == np.float64 else 2e-6) * abs(f0):
                break        # converged to rounding level
            if kind == "qchain" and opt.current_objective_value <= 1e-12 * f0:
                break        # converged (a convex quadratic): what is left of the gradient is rounding noise, and so would the comparison be
            k = opt.history_count
            S = np.stack([h.to_host() for h in opt.delta_point_history]) if k else np.zeros((0, n), dtype)
            Y = np.stack([h.to_host() for h in opt.delta_gradient_history]) if k else np.zeros((0, n), dtype)
            x, g = opt.current_point.to_host(), opt.current_gradient.to_host()
            if it > 0:
                assert np.array_equal(S[0], x - x_prev) and np.array_equal(Y[0], g - g_prev)      # pair 0 = point 0 - point 1
                assert np.array_equal(opt.delta_point.to_host(), S[0]) and np.array_equal(opt.delta_gradient.to_host(), Y[0])
            ref.install_state(x, g, opt.current_objective_value, S, Y, opt.rho_history[:k], opt.iteration_count)
            x_prev, g_prev = x, g
            opt.step(); ref.step()
            assert opt.ring_layout == 2
            if (decor or kind != "rosen") and opt.is_stuck != ref.is_stuck and min(opt.last_trials, ref.last_trials) > 30:
                break        # (the same, one side halving on to x + t d == x)
            assert opt.is_stuck == ref.is_stuck, it
            if ref.is_stuck:
                break
            if (decor or kind != "rosen") and ref.last_trials > 30 and opt.last_trials != ref.last_trials:
                break        # dozens of halvings: f_new - f is at rounding level, the two summation orders may accept one trial apart
            assert opt.iteration_count == ref.iteration_count and opt.last_trials == ref.last_trials, it
            seen.add(opt.last_trials)
            e_d = rel(opt.step_direction.to_host(), ref.step_direction)
            assert e_d <= tol_d, it
            x_new = opt.current_point.to_host()
            # (x_new = x + t d: in fp32 the point inherits the direction's relative error where the move is as large as the
            # point itself -- n = 16 near the minimiser; tests/fuzz_points.py has the same rule)
            moved_by = np.linalg.norm(ref.delta_point.astype(np.float64)) / max(np.linalg.norm(ref.current_point.astype(np.float64)), 1e-300)
            assert rel(x_new, ref.current_point) <= (tol_x if dtype == np.float64 else max(tol_x, 2 * e_d * max(1.0, moved_by))), it
            assert opt.current_objective_value == pytest.approx(ref.current_objective_value, rel=1e-12 if dtype == np.float64 else 1e-5)
            if decor or kind == "qchain":                 # the (decorated) gradient of the new point, elementwise: bit-exact
                assert np.array_equal(opt.current_gradient.to_host(), ref_p.grad(x_new)), it
            if kind == "lse":
                # softmax(x) and lambda (x - c) cancel near the minimiser: the error is measured against the terms, not their difference
                g_ref = ref_p.grad(x_new).astype(np.float64)
                terms = np.linalg.norm(1e-2 * (x_new.astype(np.float64) - cc.astype(np.float64))) + np.linalg.norm(g_ref)
                assert np.linalg.norm(opt.current_gradient.to_host().astype(np.float64) - g_ref) <= (1e-13 if dtype == np.float64 else 1e-5) * terms, it
            if box:
                assert x_new.min() >= dtype(box[0]) and x_new.max() <= dtype(box[1]), it
        assert opt.single_pass_steps == opt.iteration_count + (1 if opt.is_stuck else 0) or opt.is_stuck
        if step0 >= 300.0 and kind == "rosen":
            assert max(seen) >= 3                         # deep halvings happened, on passes
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def test_point_ring_turns_into_the_pair_ring_without_changing_a_bit(monkeypatch):
    """Anything the passes do not serve (installed pairs, an option, the split entry points) turns the point ring
    into the pair ring in place; the run then continues on the pair kernels exactly as an optimizer that never was
    a point ring would from the same state."""
    n, m = 4100, 6
    x0 = orc.rosenbrock_chain_x0(n)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
    for _ in range(m + 3):
        opt.step()
    assert opt.ring_layout == 2
    x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
    S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
    rho, its = opt.rho_history.copy(), opt.iteration_count
    opt.set_safeguards(descent_check=True)                # not served by the passes
    opt.step()
    assert opt.ring_layout == 1
    # the same step from the same state on an optimizer that starts as a pair ring
    monkeypatch.setenv("DZO_TUNE_POINT_RING", "0")
    b = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
    assert b.ring_layout == 1
    b.current_point.upload(x); b.current_gradient.upload(g); b.set_objective_value(f)
    b.set_history(S, Y, rho, iteration_count=its)
    b.set_safeguards(descent_check=True)
    b.step()
    assert opt.last_trials == b.last_trials
    assert rel(opt.step_direction.to_host(), b.step_direction.to_host()) <= 1e-11
    assert rel(opt.current_point.to_host(), b.current_point.to_host()) <= 1e-13
    k = opt.history_count
    for i in range(1, k):                                 # the converted pairs are the pairs the point ring handed out
        assert np.array_equal(opt.delta_point_history[i].to_host(), S[i - 1])
        assert np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i - 1])


@pytest.mark.parametrize("option", ["descent_check", "wolfe"])
@pytest.mark.parametrize("kind,n", [("decorated", 4100), ("decorated", 4099), ("qchain", 4100), ("qchain", 4099), ("lse", 4100), ("lse", 4099)])
def test_point_ring_objectives_continue_on_the_pair_kernels_after_an_option(kind, n, option):
    """Every objective the point ring serves (decorated chained Rosenbrock, chained quadratic, log-sum-exp), aligned and ragged:
    an option the passes do not serve turns the ring into pairs (tile ring; slabs for a ragged n) and the run continues on
    the GENERAL kernels -- Gram / combine, trial, the one-pass accepted-step tail with the gradient in the other buffer --
    step by step like the oracle from the same fields."""
    m = 5
    x0 = orc.rosenbrock_chain_x0(n)
    if kind == "decorated":
        kw = dict(l2=0.01, box_gradient=(-1.1, 0.9), box_constraint=(-1.1, 0.9))
        ref_p, dev_p = orc.Problem(orc.ROSENBROCK_CHAIN, n, **kw), dzo.Problem(dzo.ROSENBROCK_CHAIN, n, **kw)
    elif kind == "qchain":
        ref_p, dev_p = orc.Problem(orc.QUADRATIC_CHAIN, n, lam=1e-3), dzo.Problem(dzo.QUADRATIC_CHAIN, n, lam=1e-3)
    else:
        cc = orc.pcg_fill(n, 6) - 0.5
        x0 = 3.0 * (orc.pcg_fill(n, 8) - 0.5)
        ref_p, dev_p = orc.Problem(orc.LSE, n, c=cc, lam=1e-4), dzo.Problem(dzo.LSE, n, c=cc, lam=1e-4)
    opt = dzo.LBFGSOptimizer(None, dev_p, None, dzo.DeviceArray.from_host(x0), 1.0, m)
    ref = orc.LBFGS(ref_p, x0.copy(), 1.0, m)
    assert opt.ring_layout == 2
    for _ in range(3):
        opt.step()
    assert opt.ring_layout == 2 and not opt.is_stuck
    if option == "descent_check":
        opt.set_safeguards(descent_check=True); ref.set_safeguards(descent_check=True)
    else:
        opt.set_line_search(dzo.LINE_SEARCH_WOLFE); ref.set_line_search(1)
    for it in range(4):
        x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
        k = opt.history_count
        S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
        ref.install_state(x, g, f, S, Y, opt.rho_history[:k], opt.iteration_count)
        opt.step(); ref.step()
        assert opt.ring_layout == (0 if n % 2 else 1), it
        assert opt.is_stuck == ref.is_stuck, it
        if ref.is_stuck:
            break
        assert opt.iteration_count == ref.iteration_count, it
        assert rel(opt.step_direction.to_host(), ref.step_direction) <= TOL_DIRECTION, it
        x1 = opt.current_point.to_host()
        assert rel(x1, ref.current_point) <= 1e-11, it
        assert opt.current_objective_value == pytest.approx(ref.current_objective_value, rel=1e-11)
        if kind != "lse":
            assert np.array_equal(opt.current_gradient.to_host(), ref_p.grad(x1)), it
        assert np.array_equal(opt.delta_point.to_host(), x1 - x), it                                  # run_and_test! :1035-1046, exact
        assert np.array_equal(opt.delta_gradient.to_host(), opt.current_gradient.to_host() - g), it


@pytest.mark.parametrize("n", [4100, 4099])
def test_decorators_changed_between_steps_turn_the_point_ring_into_pairs_under_the_old_set(n):
    """The passes recompute every stored point's gradient under the decorators the ring was created with (ring_dec).  This
    build lets a problem handle's decorators be changed between steps (dzo_problem_set_l2 ...): the stored pairs
    y_i = g_i - g_i+1 must stay what they were -- gradients under the OLD set -- so the ring is turned into pairs before
    the new set takes effect, and the step continues exactly as the oracle does from the same fields with the new set."""
    m = 5
    x0 = orc.rosenbrock_chain_x0(n)
    dev_p = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, l2=0.01)
    opt = dzo.LBFGSOptimizer(None, dev_p, None, dzo.DeviceArray.from_host(x0), 1.0, m)
    for _ in range(m + 3):
        opt.step()
    assert opt.ring_layout == 2
    x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
    S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
    rho, its = opt.rho_history.copy(), opt.iteration_count
    assert np.array_equal(g, orc.Problem(orc.ROSENBROCK_CHAIN, n, l2=0.01).grad(x))              # (gradient under the old set)
    dzo._check(dzo.lib().dzo_problem_set_l2(dev_p.h, 0.03))
    dzo._check(dzo.lib().dzo_problem_set_box_gradient(dev_p.h, 1, -1.5, 1.5))
    new_p = orc.Problem(orc.ROSENBROCK_CHAIN, n, l2=0.03, box_gradient=(-1.5, 1.5))
    ref = orc.LBFGS(new_p, x0.copy(), 1.0, m)
    ref.install_state(x, g, f, S, Y, rho, its)
    opt.step(); ref.step()
    assert opt.ring_layout in (0, 1)                      # pairs (slabs when n is ragged)
    assert opt.last_trials == ref.last_trials and opt.iteration_count == ref.iteration_count
    assert rel(opt.step_direction.to_host(), ref.step_direction) <= TOL_DIRECTION
    x1 = opt.current_point.to_host()
    assert rel(x1, ref.current_point) <= 1e-12
    assert np.array_equal(opt.current_gradient.to_host(), new_p.grad(x1))                          # the new set from here on
    for i in range(1, opt.history_count):                 # the stored pairs are the old ones, bit for bit
        assert np.array_equal(opt.delta_point_history[i].to_host(), S[i - 1])
        assert np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i - 1])


@pytest.mark.parametrize("dtype,n", [(np.float64, 4099), (np.float32, 4097), (np.float32, 4098), (np.float32, 100_003)])
def test_ragged_point_ring_continues_on_the_slabs_when_it_leaves_the_points(dtype, n):
    """A ragged n lives on the tile ring as a POINT ring only (phantom padding in the last vector); what the passes do
    not serve sends it to the slab ring (ring_layout 0), whose two-pass kernels have element tails, with the pairs the
    point ring handed out -- and the next steps match the oracle from that state."""
    m = 6
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        assert opt.ring_layout == 2
        for _ in range(m + 3):
            opt.step()
        assert opt.ring_layout == 2 and opt.single_pass_steps == m + 3
        x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
        S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
        dx, dg, d = opt.delta_point.to_host(), opt.delta_gradient.to_host(), opt.step_direction.to_host()
        rho, its = opt.rho_history.copy(), opt.iteration_count
        assert x.shape == (n,) and S.shape == (m, n)
        opt.set_safeguards(descent_check=True)            # not served by the passes
        ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype), x0.copy(), 1.0, m)
        ref.set_safeguards(descent_check=True)
        ref.install_state(x, g, f, S, Y, rho, its)
        opt.step(); ref.step()
        assert opt.ring_layout == 0
        assert opt.last_trials == ref.last_trials and opt.iteration_count == ref.iteration_count
        assert rel(opt.step_direction.to_host(), ref.step_direction) <= (TOL_DIRECTION if dtype == np.float64 else 2e-4)
        assert rel(opt.current_point.to_host(), ref.current_point) <= (1e-12 if dtype == np.float64 else 1e-6)
        for i in range(1, opt.history_count):             # the pairs survived the move, bit for bit
            assert np.array_equal(opt.delta_point_history[i].to_host(), S[i - 1])
            assert np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i - 1])
        # and a conversion that happens BEFORE the next step keeps the last step's fields
        b = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        for _ in range(m + 3):
            b.step()
        b.set_two_loop_mode(dzo.TWOLOOP_CHAIN)
        assert b.ring_layout == 0
        assert np.array_equal(b.current_point.to_host(), x) and np.array_equal(b.current_gradient.to_host(), g)
        assert np.array_equal(b.delta_point.to_host(), dx) and np.array_equal(b.delta_gradient.to_host(), dg)
        assert np.array_equal(b.step_direction.to_host(), d)
        for i in range(m):
            assert np.array_equal(b.delta_point_history[i].to_host(), S[i]) and np.array_equal(b.delta_gradient_history[i].to_host(), Y[i])
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


# ------------------------------------------------------------------------------ stuck state of the passes
@pytest.mark.parametrize("layout", ["points", "pairs", "two_pass"])
@pytest.mark.parametrize("n,m", [(16, 3), (372, 5), (250_000, 8)])
def test_lbfgs_stuck_step_leaves_the_reference_deltas(n, m, layout, monkeypatch):
    """take_backtracking_step! that ends stuck (src/DZOptimization.jl:128-131: the trial point equals the old point
    everywhere) leaves delta_point = x_old (:118 copy!(delta_point, current_point)) and does not touch delta_gradient,
    which still holds the previous step's value; x, g, f, the history and iteration_count are those of the last
    accepted step.  Run until stuck on all three L-BFGS step implementations (point ring, pair ring, two-pass
    kernels), the oracle following the GPU, and compare the fields of the stuck optimizer with the state the step
    started from and with the oracle's.  (n = 250 000, m = 8 with the standard start is a run whose 14th step finds
    no decrease in 60 halvings: a stuck step with a full history and several rows per wave.)"""
    if layout == "pairs":
        monkeypatch.setenv("DZO_TUNE_POINT_RING", "0")
    if layout == "two_pass":
        monkeypatch.setenv("DZO_TUNE_SINGLE_PASS", "0")
    orc.set_threads(8)
    try:
        x0 = orc.rosenbrock_chain_x0(n)
        ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 1.0, m)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        assert opt.ring_layout == {"points": 2, "pairs": 1, "two_pass": 0}[layout]
        for it in range(5000):
            k = opt.history_count
            S = np.stack([h.to_host() for h in opt.delta_point_history]) if k else np.zeros((0, n))
            Y = np.stack([h.to_host() for h in opt.delta_gradient_history]) if k else np.zeros((0, n))
            x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
            dg_before = opt.delta_gradient.to_host()
            ref.install_state(x, g, f, S, Y, opt.rho_history[:k], opt.iteration_count)
            ref.delta_gradient[:] = dg_before                  # (a field the step may or may not touch: installed as well)
            opt.step(); ref.step()
            if opt.is_stuck:
                break
            # (after dozens of halvings f_new - f is at rounding level: the oracle may call stuck what the device's
            # summation order still accepts; the run goes on from the device's state)
            assert not ref.is_stuck or ref.last_trials > 30, (it, ref.last_trials)
        assert opt.is_stuck, it
        assert it > m + 2                                      # a steady-state step, history full
        assert opt.iteration_count == it
        # ---- the device's fields against the state the stuck step started from
        assert np.array_equal(opt.current_point.to_host(), x) and np.array_equal(opt.current_gradient.to_host(), g)   # :151 restored
        assert opt.current_objective_value == f
        assert np.array_equal(opt.delta_point.to_host(), x)                    # :118
        assert np.array_equal(opt.delta_gradient.to_host(), dg_before)         # untouched ...
        assert np.array_equal(dg_before, Y[0])                                 # ... i.e. still the last accepted step's
        assert opt.history_count == k
        for i in range(k):                                     # the history is the one the step started from
            assert np.array_equal(opt.delta_point_history[i].to_host(), S[i]) and np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i])
        # ---- and that this IS what the reference's loop leaves (the oracle, stuck on the same step unless the decision
        # was at rounding level: then it is stepped on until it is)
        for _ in range(4):
            if ref.is_stuck:
                break
            ref.step()
        assert ref.is_stuck
        assert np.array_equal(ref.delta_point, ref.current_point)              # :118, :128-131
        if ref.iteration_count == it:                          # same step: same fields
            assert np.array_equal(ref.current_point, x) and np.array_equal(ref.delta_point, x)
            assert np.array_equal(ref.delta_gradient, Y[0])
            assert rel(opt.step_direction.to_host(), ref.step_direction) <= 1e-9   # the direction the stuck search walked along
        opt.step()                                             # :456-458: a stuck optimizer does nothing
        assert opt.iteration_count == it and np.array_equal(opt.delta_point.to_host(), x)
    finally:
        orc.set_threads(1)


# ---- the halving limit (set_max_halvings) ends a step on the point ring: the other exit of the trial loops, with the same fields
def _oracle_follows(opt, ref, n, dtype):
    """The device's state, read through the getters (which gather it without leaving the point layout), installed into the
    oracle; returned as (x, g, f, S, Y)."""
    k = opt.history_count
    S = np.stack([h.to_host() for h in opt.delta_point_history]) if k else np.zeros((0, n), dtype)
    Y = np.stack([h.to_host() for h in opt.delta_gradient_history]) if k else np.zeros((0, n), dtype)
    x, g, f = opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value
    ref.install_state(x, g, f, S, Y, opt.rho_history[:k], opt.iteration_count)
    return x, g, f, S, Y


def _limit_pair(kind, n, m, dtype, decor):
    x0, ref_p, dev_p, _ = _point_ring_problem(n, dtype, decor, kind)
    ref = orc.LBFGS(ref_p, x0.copy(), 300.0, m)
    opt = dzo.LBFGSOptimizer(None, dev_p, None, dzo.DeviceArray.from_host(x0), 300.0, m)
    assert opt.ring_layout == 2
    return opt, ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("kind,n,m", [("rosen", 16, 3), ("rosen", 385, 5), ("qchain", 385, 5), ("lse", 16, 3), ("lse", 385, 5)])
def test_halving_limit_ends_the_first_step_on_the_point_ring(kind, n, m, dtype):
    """initial_step_length = 300 and a limit of 3 halvings: the first step (k = 0, the FIRST kernels) finds no decrease in its
    three trials and ends stuck through the limit, not through x + t d == x.  Everything is as before the step, bit for bit,
    and delta_point = x_old (:118)."""
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        opt, ref = _limit_pair(kind, n, m, dtype, {})
        opt.set_max_halvings(3); ref.set_max_halvings(3)
        x0, g0, f0, _, _ = _oracle_follows(opt, ref, n, dtype)
        dg0 = opt.delta_gradient.to_host()
        opt.step(); ref.step()
        assert opt.ring_layout == 2
        assert ref.is_stuck and ref.last_trials == 3 and ref.iteration_count == 0
        for again in (False, True):                            # the second round: after one more step(), which changes nothing
            assert opt.is_stuck and opt.last_trials == 3 and opt.iteration_count == 0 and opt.history_count == 0
            assert np.array_equal(opt.current_point.to_host(), x0) and np.array_equal(opt.current_gradient.to_host(), g0)
            assert opt.current_objective_value == f0
            assert np.array_equal(opt.delta_point.to_host(), x0)                   # :118
            assert np.array_equal(opt.delta_gradient.to_host(), dg0)               # untouched
            if not again:
                opt.step()
                assert opt.ring_layout == 2
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


@pytest.mark.parametrize("dtype", [np.float64], ids=["float64"])      # (fp32: see the docstring)
@pytest.mark.parametrize("kind,n,m,decor", [("rosen", 16, 3, None), ("rosen", 385, 5, None), ("rosen", 4099, 6, None), ("lse", 16, 3, None),
                                            ("rosen", 385, 5, "all")])
def test_halving_limit_ends_a_steady_state_step_on_the_point_ring(kind, n, m, decor, dtype):
    """m + 3 steps under the default limit (initial_step_length = 300: rejected trials on the way), then a limit of one halving:
    the first step whose trial at t = 1 is no decrease ends stuck through the limit with last_trials == 1, on the device and in
    the oracle, and leaves the fields of test_lbfgs_stuck_step_leaves_the_reference_deltas.
    The five cases in fp32 are left out: every field below held bit for bit there as well (limit exits after 4, 3, 3, 3 and 1
    further steps, as in fp64), but the direction on demand differs from the oracle's by 2.1e-7, 2.4e-8, 8.1e-8, 8.9e-8 and
    9.5e-8 relative L2 -- fp32 rounding, above the 1e-9 of this test, before the shared host pieces and after them alike."""
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        opt, ref = _limit_pair(kind, n, m, dtype, _DECOR_SETS[decor] if decor else {})
        for it in range(m + 3):
            _oracle_follows(opt, ref, n, dtype)
            opt.step(); ref.step()
            assert opt.ring_layout == 2 and not opt.is_stuck and not ref.is_stuck, it
        opt.set_max_halvings(1); ref.set_max_halvings(1)
        for further in range(1, 11):                           # (within 10 further steps, or the case fails)
            x, g, f, S, Y = _oracle_follows(opt, ref, n, dtype)
            it, k = opt.iteration_count, opt.history_count
            dg_before = opt.delta_gradient.to_host()
            ref.delta_gradient[:] = dg_before                  # (a field the step may or may not touch: installed as well)
            opt.step(); ref.step()
            assert opt.ring_layout == 2
            assert opt.is_stuck == ref.is_stuck, further       # stuck on the same step
            if opt.is_stuck:
                break
        assert opt.is_stuck and ref.is_stuck, "no step ended by the halving limit"
        assert opt.last_trials == 1 and ref.last_trials == 1
        assert it == m + 3 + further - 1
        e_d = rel(opt.step_direction.to_host(), ref.step_direction)                # formed on demand after the exit
        print(f"limit exit after {further} further steps, direction differs from the oracle's by {e_d:.3e}")
        for again in (False, True):                            # the second round: after one more step(), which changes nothing
            assert opt.is_stuck and opt.iteration_count == it and ref.iteration_count == it
            assert np.array_equal(opt.current_point.to_host(), x) and np.array_equal(opt.current_gradient.to_host(), g)   # :151 restored
            assert opt.current_objective_value == f
            assert np.array_equal(opt.delta_point.to_host(), x)                    # :118
            assert np.array_equal(opt.delta_gradient.to_host(), dg_before) and np.array_equal(dg_before, Y[0])
            assert opt.history_count == k
            for i in range(k):
                assert np.array_equal(opt.delta_point_history[i].to_host(), S[i]) and np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i])
            if not again:
                opt.step()
                assert opt.ring_layout == 2
        assert np.array_equal(ref.current_point, x) and np.array_equal(ref.delta_point, x) and np.array_equal(ref.delta_gradient, Y[0])
        assert e_d <= 1e-9
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


# ------------------------------------------------------------------------------ backend asserts (a8)
def test_constructors_assert_that_their_arrays_live_on_the_context_device():
    """src/DZOptimization.jl:363-364, 376-378, 410, 420 (and AdGD :216-226, LineSearchEvaluator :44-54): `@assert backend ==
    get_backend(...)` -- every array a constructor is given must live where it allocates the rest.  The C constructors
    reject host pointers, pointers HIP does not know and (with more than one GPU visible) another device's memory with
    DZO_ERR_ASSERT before touching them."""
    import ctypes as C
    import torch
    n = 4096
    L = dzo.lib()
    x = dzo.DeviceArray.from_host(orc.rosenbrock_chain_x0(n))
    g = dzo.DeviceArray.from_host(np.ones(n))
    host = np.ones(n)
    hostp = C.c_void_p(host.ctypes.data)
    pinned = torch.ones(n, dtype=torch.float64).pin_memory()               # registered host memory is still not device memory
    pinp = C.c_void_p(pinned.data_ptr())
    bogus = C.c_void_p(0x1000)
    prob = dzo.Problem(dzo.ROSENBROCK_CHAIN, n)
    out = C.c_void_p()

    def expect_assert(rc, what):
        assert rc == 3, (what, rc)                                         # DZO_ERR_ASSERT
        msg = L.dzo_last_error().decode()
        assert "@assert backend == get_backend(" in msg and what in msg, msg
        assert not out.value

    for bad, label in ((hostp, "host"), (pinp, "pinned"), (bogus, "bogus")):
        expect_assert(L.dzo_lbfgs_create(n, 5, dzo.F64, bad, C.c_void_p(g.ptr), 1.0, 1.0, C.byref(out)), "initial_point")
        expect_assert(L.dzo_lbfgs_create(n, 5, dzo.F64, C.c_void_p(x.ptr), bad, 1.0, 1.0, C.byref(out)), "initial_gradient")
        expect_assert(L.dzo_lbfgs_create_problem(prob.h, 5, bad, 1.0, C.byref(out)), "initial_point")
        expect_assert(L.dzo_adgd_create(n, dzo.F64, bad, C.c_void_p(g.ptr), 1.0, 1.0, C.byref(out)), "initial_point")
        expect_assert(L.dzo_adgd_create(n, dzo.F64, C.c_void_p(x.ptr), bad, 1.0, 1.0, C.byref(out)), "initial_gradient")
        expect_assert(L.dzo_adgd_create_problem(prob.h, bad, 1.0, C.byref(out)), "initial_point")
        expect_assert(L.dzo_bfgs_create_problem(prob.h, bad, 1.0, C.byref(out)), "initial_point")
        expect_assert(L.dzo_gd_create_problem(prob.h, bad, 1.0, C.byref(out)), "initial_point")
    # callbacks must not be called with an array that fails the assert (:410 comes before :412-416)
    calls = []
    with pytest.raises(AssertionError):
        dzo.LBFGSOptimizer(None, lambda x_: calls.append(1) or 0.0, lambda g_, x_: calls.append(2), dzo.DeviceArray(n, np.float64, ptr=host.ctypes.data, owner=False), 1.0, 5)
    assert not calls
    # the same arrays on the device pass
    assert L.dzo_lbfgs_create(n, 5, dzo.F64, C.c_void_p(x.ptr), C.c_void_p(g.ptr), 1.0, 1.0, C.byref(out)) == 0
    L.dzo_lbfgs_destroy(out); out.value = None
    if torch.cuda.device_count() > 1:                                      # a pointer from another GPU (the mistake the assert catches on a node)
        other = torch.ones(n, dtype=torch.float64, device="cuda:1")
        expect_assert(L.dzo_lbfgs_create(n, 5, dzo.F64, C.c_void_p(other.data_ptr()), C.c_void_p(g.ptr), 1.0, 1.0, C.byref(out)), "initial_point")
        assert "device 1" in L.dzo_last_error().decode()


# ------------------------------------------------------------------------------ the caller's arrays ARE the current point (:393)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_point_ring_adopts_what_the_host_wrote_into_the_aliased_arrays(dtype):
    """The optimizer aliases the caller's x0 (src/DZOptimization.jl:393) and `current_gradient`: what the host writes into
    them between two steps is what the next step starts from, while delta_point_history / delta_gradient_history are
    separate arrays that such a write does not change.  On the point ring the caller's arrays are copies of point 0;
    a write is detected before the next step and the run continues (on the pair ring) exactly as the oracle does
    from the same fields."""
    n, m = 4100 if dtype == np.float64 else 8200, 6
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    if dtype == np.float32:
        orc.set_dot_mode(orc.DOT_WIDE)
    try:
        pr = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype)
        xd = dzo.DeviceArray.from_host(x0)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, xd, 1.0, m)
        for _ in range(m + 2):
            opt.step()
        assert opt.ring_layout == 2
        # looking does not leave the point ring
        S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
        x = opt.current_point.to_host()
        opt.step()
        assert opt.ring_layout == 2
        S = np.stack([h.to_host() for h in opt.delta_point_history]); Y = np.stack([h.to_host() for h in opt.delta_gradient_history])
        rho, its = opt.rho_history.copy(), opt.iteration_count
        # the host moves the point (and keeps f, g consistent with it, as a restart from a perturbed point would)
        x = opt.current_point.to_host()
        x_new = (x + dtype(1e-3) * np.cos(np.arange(n))).astype(dtype)
        g_new, f_new = pr.grad(x_new), pr.eval(x_new)
        xd.upload(x_new)                                  # through the caller's own handle of the aliased array
        opt.current_gradient.upload(g_new)
        opt.set_objective_value(f_new)
        ref = orc.LBFGS(pr, x0.copy(), 1.0, m)
        ref.install_state(x_new, g_new, f_new, S, Y, rho, its)
        opt.step(); ref.step()
        assert opt.ring_layout == 1                       # continued on the pair ring
        assert opt.last_trials == ref.last_trials and opt.iteration_count == ref.iteration_count
        tol_d = TOL_DIRECTION if dtype == np.float64 else 2e-4
        assert rel(opt.step_direction.to_host().astype(np.float64), ref.step_direction.astype(np.float64)) <= tol_d
        assert rel(opt.current_point.to_host().astype(np.float64), ref.current_point.astype(np.float64)) <= (1e-12 if dtype == np.float64 else 1e-6)
        for i in range(1, opt.history_count):             # the stored pairs were not changed by the write
            assert np.array_equal(opt.delta_point_history[i].to_host(), S[i - 1]) and np.array_equal(opt.delta_gradient_history[i].to_host(), Y[i - 1])
        assert np.array_equal(xd.to_host(), opt.current_point.to_host())   # still aliased
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def test_fused_reduce_finish_launch_gives_the_same_scalars_bit_for_bit(monkeypatch):
    """DZO_TUNE_FUSED_FINISH=1: the scalar stage of a Gram pass (sum of the per-block partials + the two-loop on scalars)
    in one 1024-thread launch instead of two launches (measured slower at config 4, off by default).  Its waves emulate
    the 256-thread reduction kernel's summation order, so alpha, rho and the direction must be the SAME BITS."""
    n, k, m = 100_003, 10, 10

    def direction(fused):
        monkeypatch.setenv("DZO_TUNE_FUSED_FINISH", str(fused))
        opt, g, S, Y, rho, keep = _frozen(n, k, m, np.float32)
        d = opt.compute_step_direction().to_host()
        d2 = opt.compute_step_direction().to_host()
        assert np.array_equal(d, d2)
        return d, opt.alpha_history.copy()
    d0, a0 = direction(0)
    d1, a1 = direction(1)
    assert np.array_equal(a0, a1)
    assert np.array_equal(d0, d1)


@pytest.mark.parametrize("n", [4100, 4099])
def test_watching_the_point_ring_through_read_costs_the_next_step_no_check(n):
    """dzo_lbfgs_read (what `opt.current_point.to_host()` goes through): the field is copied to the host without a pointer
    hand-out, so the step behind it does not compare the aliased arrays with the ring (a monitoring read used to
    cost the next step a regrad, two compare passes and a host round trip).  A pointer hand-out (`.ptr`, get_ptr) still does,
    and so does a write through the caller's own handle after a read (dzo_memcpy_* leaves the look on record)."""
    m = 5
    x0 = orc.rosenbrock_chain_x0(n)
    runs = []
    for watch in (False, True):
        xd = dzo.DeviceArray.from_host(x0)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None, xd, 1.0, m)
        opt.step()
        checks0 = opt.host_write_checks
        seen = []
        for _ in range(10):
            opt.step()
            if watch:
                seen.append((opt.current_point.to_host(), opt.current_gradient.to_host(), opt.delta_point.to_host()))
        assert opt.ring_layout == 2 and opt.host_write_checks == checks0
        runs.append((opt.current_point.to_host(), opt.current_gradient.to_host(), opt.current_objective_value, opt.iteration_count))
        if watch:
            ref = orc.LBFGS(orc.Problem(orc.ROSENBROCK_CHAIN, n), x0.copy(), 1.0, m)
            for _ in range(2):
                ref.step()
            assert rel(seen[0][0], ref.current_point) <= 1e-12 and np.array_equal(seen[0][1], orc.Problem(orc.ROSENBROCK_CHAIN, n).grad(seen[0][0]))
            assert np.array_equal(xd.to_host(), runs[-1][0])          # the caller's own array IS current_point (:393)
            _ = opt.current_point.ptr                                  # a hand-out: the host may write through it
            opt.step()
            assert opt.host_write_checks == checks0 + 1 and opt.ring_layout == 2
            x = opt.current_point.to_host()                            # a read, then a write through the caller's handle
            xd.upload((x + 1e-3 * np.cos(np.arange(n))))
            opt.step()
            assert opt.host_write_checks == checks0 + 2 and opt.ring_layout == (1 if n % 2 == 0 else 0)   # seen, adopted: the run continues on the pair ring (a ragged n: on the slabs)
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_the_recurrences_division_free_quotient_is_the_quotient(mode):
    """gram_finish's 2k dependent quotients (src/DZOptimization.jl:440, :447) are formed from a correctly rounded reciprocal
    and four fused multiply-adds (fd_div: Markstein's final step behind one refinement) instead of an IEEE division each.
    The claim is bit equality with `a / b` for operands in the middle of the exponent range (everything else takes the
    division): checked here on the device over 2^27 operand pairs per kind -- random, special divisors (significand all
    ones / all zeros / one bit), quotients that are exact or one rounding from exact, quotients next to a rounding boundary,
    small integers."""
    checked, bad, first = dzo.selftest_fast_div(1234 + mode, 1 << 27, mode)
    assert checked > (1 << 26) and bad == 0, (mode, checked, bad, first)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fast_division_knob_changes_no_bit(dtype, monkeypatch):
    """DZO_TUNE_FAST_DIV=0 puts the IEEE divisions back into the recurrence: same alpha / coef / scale, same run."""
    n, m = 4100 if dtype == np.float64 else 8200, 7
    x0 = orc.rosenbrock_chain_x0(n, dtype)
    runs = []
    for knob in ("1", "0"):
        monkeypatch.setenv("DZO_TUNE_FAST_DIV", knob)
        opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype), None, dzo.DeviceArray.from_host(x0), 1.0, m)
        trace = []
        for _ in range(25):
            opt.step()
            trace.append((opt.current_objective_value, opt.last_trials, tuple(opt.alpha_history), tuple(opt.rho_history)))
        runs.append((trace, opt.current_point.to_host()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
