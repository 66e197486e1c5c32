"""Dense BFGS kernels of csrc/dzo_bfgs.hip at every shape edge, both element types, every instantiation a launcher can pick.

The file's promise is that the rank-2 update of the inverse Hessian (legacy/DZOptimization.jl:878-886) is evaluated exactly as
written, one rounding per operation, on full storage and on the lower triangle.  A Frobenius norm over n^2 elements cannot see
a contraction into fma or one wrong element, so H is REPLAYED here: tests/bfgs_twin.py searches the few values the two scalars
of the update can take and passes iff one pair reproduces every element of the device's H bit for bit.  The sums (t = H*dg, the
fused next direction, dzo_symv) are held to the derived bound of a double-accumulated sum rounded once (bfgs_twin.sum_bound),
against the longdouble product with the matrix the device itself holds.  Nothing here depends on a line search landing where
the oracle's did, so fp32 is held to the same checks as fp64.

Every test prints the worst error / bound ratio per quantity and the widest candidate window it used (run with -s).  In fp32 a
ratio close to 1 (0.99 on the step paths) is expected and is no sign of a thin margin in the kernels: the double-accumulated sum
is exact to n 2^-53, so the error is the final rounding to fp32 alone, up to half an ulp = u_T |sum|, and the bound's u_T sum |terms|
equals that when all terms of a row have one sign.  A correct kernel cannot exceed it for any seed; fp64 sits at 0.1 - 0.3.

Not covered, on purpose: DZO_TUNE_BFGS_COLS = 8 / 16 (read once per process), the n >= 65535 * 4 branch of step! (H would not
fit), the line searches.  The batched kernel of dzo_batch.hip has its own file, tests/test_gpu_bfgs_batch_shapes.py."""
import numpy as np
import pytest

import bfgs_twin as tw
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64, F32 = np.float64, np.float32
PAD = 8                                       # guard elements behind every operand (and `offset` of them in front)


def _fill(size, dtype):
    """guard pattern: no value an update could produce by accident, different at every index."""
    return (-(2.0 ** 20) - np.arange(size)).astype(dtype)


class _Worst:
    """worst error / bound ratio per quantity, widest windows"""

    def __init__(self):
        self.ratio, self.window = {}, {}

    def bound(self, name, got, exact, bound, where):
        err = np.abs(got.astype(LD) - exact)
        assert np.isfinite(got).all(), (name, where)
        zero = bound == 0
        assert (err[zero] == 0).all(), (name, where)
        r = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        self.ratio[name] = max(self.ratio.get(name, 0.0), r)
        assert r <= 1.0, (name, where, r, int(np.argmax(err / np.where(zero, 1, bound))))

    def replay(self, r, where):
        assert r.ok, (where, r)
        self.window["overlap"] = max(self.window.get("overlap", 0), r.window_overlap)
        self.window["delta"] = max(self.window.get("delta", 0), r.window_delta)
        self.window["pairs tried"] = max(self.window.get("pairs tried", 0), r.tried)

    def report(self, what):
        print(f"\n{what}: worst error/bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.ratio.items()))
              + "; widest window " + ", ".join(f"{k} {v}" for k, v in sorted(self.window.items())))


class _Operand:
    """a device buffer [offset guards | data | PAD guards] and the view of its data"""

    def __init__(self, data, offset, dtype):
        data = np.ascontiguousarray(data, dtype)
        self.offset, self.shape = offset, data.shape
        self.host = _fill(offset + data.size + PAD, dtype)
        self.host[offset:offset + data.size] = data.reshape(-1)
        self.dev = dzo.DeviceArray.from_host(self.host)
        self.view = self.dev.view(offset, data.shape)

    def read(self):
        """the data, after checking that the guards on both sides kept their pattern"""
        got = self.dev.to_host()
        size = int(np.prod(self.shape))
        assert np.array_equal(got[:self.offset], self.host[:self.offset]), "guard in front overwritten"
        assert np.array_equal(got[self.offset + size:], self.host[self.offset + size:]), "guard behind overwritten"
        return got[self.offset:self.offset + size].reshape(self.shape)


def _standalone(n, dtype, worst, offsets=None, direction=True, where=None):
    """dzo_bfgs_update (+ dzo_symv on its result) with every operand at the element offset ``offsets`` names (default 0), and
    all checks of (a): H by replay with d_scaled and lam given (so overlap, :874 and delta are checked too), H equal to its
    transpose, t / d_next / symv within sum_bound, guards intact."""
    offsets = offsets or {}
    where = where or (n, np.dtype(dtype).name, offsets)
    H0, d, dg, g, lam = tw.update_inputs(n, dtype)
    ops = {k: _Operand(a, offsets.get(k, 0), dtype) for k, a in
           dict(H=H0, d=d, dg=dg, g=g, scratch=np.zeros(n), d_next=np.zeros(n), symv_out=np.zeros(n)).items()}
    if direction:
        dzo.update_inverse_hessian_(ops["H"].view, float(lam), ops["d"].view, ops["dg"].view, ops["scratch"].view, ops["g"].view,
                                    ops["d_next"].view)
    else:
        dzo.update_inverse_hessian_(ops["H"].view, float(lam), ops["d"].view, ops["dg"].view, ops["scratch"].view)
    dzo.symv_(ops["symv_out"].view, ops["H"].view, ops["g"].view)
    H_new, d_scaled, t = ops["H"].read(), ops["d"].read(), ops["scratch"].read()
    assert np.array_equal(ops["dg"].read(), dg) and np.array_equal(ops["g"].read(), g)
    worst.replay(tw.replay_update(H0, d, dg, t, H_new, d_scaled=d_scaled, lam=lam, acc_bits=53), where)
    assert np.array_equal(H_new, H_new.T), where
    exact_t, _ = tw.exact_matvec(H0, dg)
    worst.bound("t", t, exact_t, tw.sum_bound(H0, dg, n, dtype), where)
    exact_d, _ = tw.exact_matvec(H_new, g)
    bound_d = tw.sum_bound(H_new, g, n, dtype)
    d_next = ops["d_next"].read()
    if direction:
        worst.bound("d_next", d_next, exact_d, bound_d, where)
    else:
        assert np.array_equal(d_next, np.zeros(n, dtype)), where
    worst.bound("symv", ops["symv_out"].read(), exact_d, bound_d, where)
    # which instantiation the launchers are MEANT to take for these alignments (bfgs_twin.takes_vec; the tests print it).  The
    # device does not report what it ran: what protects the al16 fallbacks is the replay, the guards and the absence of a fault
    mis = {k for k, v in offsets.items() if (v * np.dtype(dtype).itemsize) % 16}
    symv_names = {"H": "H", "dg": "v"}                        # the update hands launch_symv (H, dg) as (H, v)
    return dict(symv=tw.takes_vec(n, dtype, "symv", {symv_names[k] for k in mis if k in symv_names}),
                update=tw.takes_vec(n, dtype, "update", mis - (set() if direction else {"g"})))


# ------------------------------------------------------------------------------ (a) standalone entry points
@pytest.mark.parametrize("n,dtype", [(n, F64) for n in tw.FULL_F64] + [(n, F32) for n in tw.FULL_F32])
def test_standalone_update_replays_bit_for_bit(n, dtype):
    worst = _Worst()
    took = _standalone(n, dtype, worst)
    assert took["update"] == took["symv"] == (n % (16 // np.dtype(dtype).itemsize) == 0)
    worst.report(f"standalone update n={n} {np.dtype(dtype).name} VEC={took['update']}")


@pytest.mark.parametrize("n,dtype", [(3, F64), (512, F64), (1025, F64), (7, F32), (1024, F32), (1025, F32)])
def test_standalone_update_without_the_fused_direction(n, dtype):
    worst = _Worst()
    _standalone(n, dtype, worst, direction=False)
    worst.report(f"standalone update, no direction, n={n} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------ (b) views at odd element offsets
_VIEW_CASES = [(n, F64, 1) for n in (8, 512)] + [(n, F32, off) for n in (8, 1024) for off in (1, 2, 3)]


@pytest.mark.parametrize("which", ["all", "H", "d", "dg", "scratch", "g"])
@pytest.mark.parametrize("n,dtype,offset", _VIEW_CASES)
def test_views_at_odd_element_offsets(n, dtype, offset, which):
    """n would take the VEC instantiations; an operand that is not 16-byte aligned must send exactly the launchers that name it
    to the scalar ones (launch_symv: H, dg; launch_bfgs_update: H, d, scratch, g).  A vector access through such a pointer would
    fault or, worse, silently read the neighbouring elements: the replay and the guards see both.  The two assertions on
    ``took`` only document which path each case is meant for (they compare bfgs_twin's table with itself, not with the device)."""
    worst = _Worst()
    names = ("H", "d", "dg", "scratch", "g", "d_next", "symv_out") if which == "all" else (which,)
    took = _standalone(n, dtype, worst, offsets={k: offset for k in names})
    assert took["symv"] == (which not in ("all", "H", "dg"))
    assert took["update"] == (which == "dg")
    worst.report(f"views n={n} {np.dtype(dtype).name} offset {offset} of {which}: symv VEC={took['symv']} update VEC={took['update']}")


# ------------------------------------------------------------------------------ (c), (d) step!
def _oracle_state(ref):
    return dict(x=ref.current_point.copy(), g=ref.current_gradient.copy(),
                H=np.ascontiguousarray(ref.approximate_inverse_hessian), d=ref.next_step_direction.copy(),
                f=ref.current_objective_value, last_step_length=ref.last_step_length,
                iteration_count=ref.iteration_count, last_step_type=ref.last_step_type,
                dx=ref.delta_point.copy(), dg=ref.delta_gradient.copy())


def _read_step(opt):
    n = opt.n
    return dict(dg=opt.delta_gradient.to_host(), t=opt.scratch.to_host(), g=opt.current_gradient.to_host(),
                d=opt.next_step_direction.to_host(), H=opt.approximate_inverse_hessian.to_host().reshape(n, n),
                last_step_length=opt.last_step_length)


def _check_bfgs_step(H0, d0, got, worst, where):
    """One BFGS step of the device from (H0, d0): H replayed (overlap and delta both fitted; lam = -t_b is not readable exactly,
    so the estimate -last_step_length / ||d0||, with 3 u_T for the roundings of the step length, of lam and of the norm -- see
    bfgs_twin.device_norm: the estimate is close to the device's lam, not equal to it), H whole and equal to its transpose, scratch = H0*dg and the new direction = H_new*g_new within the
    sum bound."""
    T = H0.dtype
    n = d0.size
    H_new = got["H"]
    assert np.array_equal(H_new, H_new.T), where
    lam = -LD(got["last_step_length"]) / LD(tw.device_norm(d0))
    worst.replay(tw.replay_update(H0, d0, got["dg"], got["t"], H_new, lam=lam, acc_bits=53, lam_rel=3 * tw.unit_roundoff(T)), where)
    exact_t, _ = tw.exact_matvec(H0, got["dg"])
    worst.bound("scratch", got["t"], exact_t, tw.sum_bound(H0, got["dg"], n, T), where)
    exact_d, _ = tw.exact_matvec(H_new, got["g"])
    worst.bound("direction", got["d"], exact_d, tw.sum_bound(H_new, got["g"], n, T), where)


def _step_case(n, dtype, worst, steps, need, two_in_a_row=False):
    """States from the oracle of the same dtype (dense quadratic), each installed in the device optimizer, one step!, and the
    checks of whichever step the DEVICE took.  Trajectories from several starts until ``need`` BFGS steps have been checked (a
    quadratic in n dimensions is solved in about n steps; a trajectory is left before the overlap d.dg cancels)."""
    A = orc.quadratic_matrix(n, dtype)
    checked, twice_done = 0, not two_in_a_row
    stop = 1e-8 if dtype == F64 else 1e-3
    for seed in range(4, 12):
        x0 = (orc.pcg_fill(n, seed) - 0.5).astype(dtype)
        ref = orc.BFGS(orc.Problem(orc.QUADRATIC, n, dtype, A=A), x0, 1.0)
        opt = dzo.BFGSOptimizer(dzo.Problem(dzo.QUADRATIC, n, dtype=dtype, A=A), None, dzo.DeviceArray.from_host(x0), 1.0)
        g0 = np.linalg.norm(ref.current_gradient.astype(F64))
        for it in range(steps):
            if ref.has_terminated or np.linalg.norm(ref.current_gradient.astype(F64)) <= stop * g0:
                break
            st = _oracle_state(ref)
            opt.install_state(**st)
            opt.step(); ref.step()
            if opt.has_terminated:
                break
            assert opt.iteration_count == st["iteration_count"] + 1
            where = (n, np.dtype(dtype).name, seed, it)
            if opt.last_step_type == dzo.STEP_BFGS:
                got = _read_step(opt)
                _check_bfgs_step(st["H"], st["d"], got, worst, where)
                checked += 1
                if not twice_done:
                    # two updates in a row without anybody reading H in between: the upper triangle is stale under the second.
                    # Its state in between is `got` (the kernels are deterministic; the direction is compared to make sure).
                    opt.install_state(**st)
                    opt.step()
                    assert opt.last_step_type == dzo.STEP_BFGS and opt.iteration_count == st["iteration_count"] + 1
                    assert np.array_equal(opt.next_step_direction.to_host(), got["d"]), where
                    opt.step()
                    assert opt.last_step_type == dzo.STEP_BFGS and opt.iteration_count == st["iteration_count"] + 2 and not opt.has_terminated
                    _check_bfgs_step(got["H"], got["d"], _read_step(opt), worst, where + ("second in a row",))
                    twice_done = True
            else:
                assert opt.last_step_type == dzo.STEP_GRADIENT_DESCENT
                assert np.array_equal(opt.approximate_inverse_hessian.to_host().reshape(n, n), np.eye(n, dtype=dtype)), where
                assert np.array_equal(opt.next_step_direction.to_host(), opt.current_gradient.to_host()), where
        if checked >= need and twice_done:
            break
    assert checked >= need and twice_done, (checked, need)
    return checked


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", [3, 5, 7, 129, 513, 1025, 4, 8, 512, 1028])
def test_step_full_storage_fused_pair(n, dtype, monkeypatch):
    """symv_kernel with partials + bfgs_update_kernel<T, VEC, true, true, C>: n = 3 .. 1025 the scalar instantiation (the
    inverse overlap applied on the fly to scalar loads), 4 .. 1028 the vector one."""
    monkeypatch.delenv("DZO_TUNE_BFGS_TRI_MIN_N", raising=False)
    assert not tw.takes_tri(n, dtype)
    worst = _Worst()
    checked = _step_case(n, dtype, worst, steps=6, need=4)
    worst.report(f"step! full storage n={n} {np.dtype(dtype).name} VEC={tw.takes_vec(n, dtype, 'fused')}, {checked} BFGS steps")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", tw.TRI)
def test_step_lower_triangle(n, dtype, monkeypatch):
    """tri_pass_kernel / tri_reduce_kernel, forced at every size: windows, panels, the first interior tile, the reduce kernel's
    second trip.  The matrix handed out is whole and equals its transpose bit for bit; once per case two updates run back to
    back on a stale upper triangle."""
    monkeypatch.setenv("DZO_TUNE_BFGS_TRI_MIN_N", "2")
    assert tw.takes_tri(n, dtype, 2)
    worst = _Worst()
    orc.set_threads(8 if n >= 1024 else 1)
    try:
        checked = _step_case(n, dtype, worst, steps=3 if n == 2050 else 6, need=3 if n == 2050 else 4, two_in_a_row=True)
    finally:
        orc.set_threads(1)
    worst.report(f"step! lower triangle n={n} {np.dtype(dtype).name}, {checked} BFGS steps + two in a row")


# ------------------------------------------------------------------------------ (e) MFMA update
@pytest.mark.parametrize("n", tw.MFMA)
def test_mfma_update_elementwise(n):
    """The MFMA form rounds as an fma chain and is not symmetric: an elementwise bound instead of a replay, every element of
    every tile -- with 5 and 7 tiles per dimension a strip's last job ends early behind full ones."""
    worst = _Worst()
    H0, d, dg, g, lam = tw.update_inputs(n, F64)
    Hd, dd, yd, scratch = dzo.DeviceArray.from_host(H0), dzo.DeviceArray.from_host(d), dzo.DeviceArray.from_host(dg), dzo.DeviceArray(n)
    dzo.update_inverse_hessian_mfma_(Hd, float(lam), dd, yd, scratch)
    H_new, d_scaled, t = Hd.to_host(), dd.to_host(), scratch.to_host()
    c, W = tw.overlap_candidates(d, dg, 53, d_scaled)
    assert c.size >= 1, "no overlap within the window reproduces the scaled direction (:874)"
    worst.window["overlap"] = W
    exact_t, _ = tw.exact_matvec(H0, dg)
    worst.bound("t", t, exact_t, tw.sum_bound(H0, dg, n, F64), n)
    exact, bound = tw.mfma_bound(H0, d_scaled, t, lam, c[0], dg)
    # device H is column-major and no longer symmetric: to_host() shows its transpose
    worst.bound("H", H_new.T, exact, bound, n)
    worst.report(f"MFMA update n={n} ({n // 16} tiles per dimension)")
