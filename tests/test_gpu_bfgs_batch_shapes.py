"""The batched BFGS kernel of csrc/dzo_batch.hip (batch_step_kernel, batch_init_kernel, batch_mirror_kernel) at every shape edge
of bfgs_twin.BATCH, in both element types: all eight step instantiations (rp 1, rp 2 narrow, rp 2 wide, rp 4; double and float).

What is compared.  The step kernel keeps the LOWER triangle of every H only and dzo_bfgs_batch_get_ptr mirrors it into the upper
one before anybody reads H, so ``np.array_equal(H, H.T)`` holds whatever the kernel did and proves nothing here.  The question
is whether every lower-triangle element was updated once with the right operands, the pair (j - 1, j) that straddles the
diagonal included, and a Frobenius norm over n^2 elements cannot see one wrong element.  So after a step from a known state:

* x: some single tt among the 17 values of T around last_step_length / ||dir|| gives x_new == fma(-tt, dir, x_old) in every
  element, bit for bit; then lam = -tt exactly.  dx, dg and (Rosenbrock) the gradient are bit for bit, f and the quadratic's
  gradient within the bound of a double-accumulated sum rounded once.
* H: every element as handed out, both triangles, within bfgs_twin.batch_update_bound of the longdouble update computed from
  H0, d, dg and lam alone -- t = H0*dg stays in LDS, so in fp64 there is no replay.  tests/test_bfgs_twin.py shows that the
  bound sees an update left out, applied twice or taken with a neighbouring column's t at a single element.
* fp32: t is a double-accumulated sum rounded once, i.e. the rounding of the exact sum (bfgs_twin.t_rounded), so H is replayed
  bit for bit as in tests/test_gpu_bfgs_shapes.py.
* the next direction within the sum bound against the device's own H; a gradient-descent step leaves exactly the identity.
* fp64 against the oracle as tests/test_gpu_bfgs_steps.py does; fp32 against the oracle's decisions (both sides round the
  same wide sums, so step type, point and f agree bit for bit unless a sum straddles a rounding boundary: at most one step
  per case may differ, and it is printed).

Every test prints its worst error / bound ratio per quantity and the form it ran (run with -s); a table per form and dtype
follows the last test.  Ratios near 1 in fp32 are expected for the sums, see tests/test_gpu_bfgs_shapes.py."""
import numpy as np
import pytest

import bfgs_twin as tw
from dzo_loader import dzo
from oracle import oracle as orc
from test_gpu_bfgs_steps import _batch_read, _check_step, _oracle_state

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64, F32 = np.float64, np.float32
FIELDS = ("x", "g", "H", "d", "dx", "dg", "f", "last_step_length", "iteration_count", "last_step_type", "has_terminated")
_TABLE = {}                                   # (form, dtype name) -> worst ratios, widest windows, fp32 steps that differed


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nform, dtype: worst error/bound and widest replay windows over the whole file")
    for key in sorted(_TABLE):
        print(f"  {key[0]:<10} {key[1]}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in sorted(_TABLE[key].items())))


def _same(a, b):
    """bit for bit (array_equal would take -0.0 for 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _fma(a, x, y):
    """fma(a, x_i, y_i) in the type of x, one rounding (the oracle's out-of-place axpy)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    out = np.empty_like(x)
    getattr(orc.lib(), "orc_axpy_oop" + orc._suf(x.dtype))(orc._ptr(out), float(a), orc._ptr(x), orc._ptr(y), x.size)
    return out


class _Worst:
    def __init__(self, n, dtype):
        self.key = (tw.batch_form_name(n, dtype), np.dtype(dtype).name)
        self.ratio, self.window, self.differed = {}, {}, 0

    def note(self, name, r):
        self.ratio[name] = max(self.ratio.get(name, 0.0), float(r))

    def bound(self, name, got, exact, bound, where):
        got, exact, bound = (np.atleast_1d(v) for v in (got, exact, bound))
        assert np.isfinite(got).all(), (name, where)
        err = np.abs(got.astype(LD) - exact)
        zero = bound == 0
        assert (err[zero] == 0).all(), (name, where)
        r = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        self.note(name, r)
        assert r <= 1.0, (name, where, r, int(np.argmax(err / np.where(zero, 1, bound))))

    def replay(self, r, where):
        assert r.ok, (where, r)
        for k, v in (("overlap window", r.window_overlap), ("delta window", r.window_delta), ("pairs tried", r.tried)):
            self.window[k] = max(self.window.get(k, 0), v)

    def report(self, what):
        print(f"\n{what} [{self.key[0]}]: worst error/bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.ratio.items()))
              + ("; widest " + ", ".join(f"{k} {v}" for k, v in sorted(self.window.items())) if self.window else "")
              + (f"; {self.differed} fp32 step(s) differed from the oracle's decision" if self.key[1] == "float32" else ""))
        row = _TABLE.setdefault(self.key, {})
        for k, v in list(self.ratio.items()) + list(self.window.items()):
            row[k] = max(row.get(k, 0), v)
        if self.key[1] == "float32":
            row["steps differing from the oracle"] = row.get("steps differing from the oracle", 0) + self.differed


def _one(state, b):
    return {k: v[b] for k, v in state.items()}


def _objective_terms(prob, x):
    """sum |terms| of the objective's wide sum at x, in longdouble."""
    xl = x.astype(LD)
    if prob.kind == orc.QUADRATIC:
        return LD(0.5) * np.abs(prob.A.astype(LD) * np.multiply.outer(xl, xl)).sum()
    t1, t2 = 1 - xl[:-1], xl[1:] - xl[:-1] * xl[:-1]
    return (100 * t2 * t2 + t1 * t1).sum()


def _check_device_step(old, new, prob, worst, where):
    """The checks of one step of one instance from ``old`` (what the device held) to ``new`` (what it holds now), none of which
    depends on the oracle's optimizer.  Returns "bfgs", "gd", or "cancelled" (a BFGS step whose overlap cancels to less than a
    hundredth of its terms: x, g and f were checked, H was not)."""
    T = old["x"].dtype
    n = old["x"].size
    u, a = LD(tw.unit_roundoff(T)), (n + 2) * LD(2.0) ** -53
    assert not new["has_terminated"] and new["iteration_count"] == old["iteration_count"] + 1, where
    typ = int(new["last_step_type"])
    assert typ in (dzo.STEP_BFGS, dzo.STEP_GRADIENT_DESCENT), where
    direction = old["d"] if typ == dzo.STEP_BFGS else old["g"]
    # x: one tt for all elements
    est = LD(new["last_step_length"]) / LD(tw.device_norm(direction))
    tts = [tt for tt in tw.candidates(est, 8, T) if _same(_fma(-tt, direction, old["x"]), new["x"])]
    assert tts, (where, "no step length within 8 values of last_step_length / ||dir|| reproduces x")
    assert _same(new["dx"], new["x"] - old["x"]), where
    # g
    if prob.kind == orc.QUADRATIC:
        exact_g, _ = tw.exact_matvec(prob.A, new["x"])
        worst.bound("g", new["g"], exact_g, tw.sum_bound(prob.A, new["x"], n, T), where)
    else:
        assert _same(new["g"], prob.grad(np.ascontiguousarray(new["x"]))), where
    assert _same(new["dg"], new["g"] - old["g"]), where
    # f
    f_dev = T.type(new["f"])
    assert float(f_dev) == float(new["f"]) and new["f"] < old["f"], where
    f_ref = prob.eval(np.ascontiguousarray(new["x"]))
    worst.bound("f", np.array([f_dev]), np.array([LD(f_ref)]), np.array([a * _objective_terms(prob, new["x"]) + u * abs(LD(f_ref))]), where)
    H_new = np.ascontiguousarray(new["H"].T)                      # (the device's matrix is column-major)
    if typ == dzo.STEP_GRADIENT_DESCENT:
        assert _same(H_new, np.eye(n, dtype=T)), where
        assert _same(new["d"], new["g"]), where
        return "gd"
    H0, d0, dg = np.ascontiguousarray(old["H"].T), old["d"], new["dg"]
    exact_d, _ = tw.exact_matvec(H_new, new["g"])
    worst.bound("d_next", new["d"], exact_d, tw.sum_bound(H_new, new["g"], n, T), where)
    if tw.overlap_cancellation(d0, dg) > 100:
        return "cancelled"
    ratios = []
    for tt in tts:
        exact, bound = tw.batch_update_bound(H0, d0, dg, -tt, T)
        ratios.append(float((np.abs(H_new.astype(LD) - exact) / bound).max()))
    worst.note("H", min(ratios))
    assert min(ratios) <= 1.0, (where, ratios, "H outside the elementwise bound of the update")
    if T == F32:
        t, undecided = tw.t_rounded(H0, dg)
        runs = [tw.replay_update_undecided(H0, d0, dg, t, undecided, H_new, lam=-tt, acc_bits=53) for tt in tts]
        worst.replay(([r for r in runs if r.ok] or runs)[0], where)
        worst.window["undecided rows"] = max(worst.window.get("undecided rows", 0), len(undecided))
    return "bfgs"


def _against_oracle(ref, f_before, new, worst, where):
    """``ref`` took the same step from the same state.  fp64: _check_step of tests/test_gpu_bfgs_steps.py.  fp32: step type,
    point, f and step length bit for bit; a step that differs is counted and printed, not failed (the caller caps the count)."""
    if new["x"].dtype == F64:
        _check_step(dict(new, has_terminated=bool(new["has_terminated"])), ref, f_before, where)
        return
    same = (int(new["last_step_type"]) == ref.last_step_type and bool(new["has_terminated"]) == ref.has_terminated
            and _same(new["x"], ref.current_point) and float(new["f"]) == float(ref.current_objective_value)
            and float(new["last_step_length"]) == float(ref.last_step_length))
    if not same:
        worst.differed += 1
        print(f"\n{where}: the device's step differs from the oracle's: type {int(new['last_step_type'])} / {ref.last_step_type}, "
              f"f {float(new['f'])!r} / {float(ref.current_objective_value)!r}, length {float(new['last_step_length'])!r} / {float(ref.last_step_length)!r}")


def _problems(n, dtype, quadratic, B):
    """(device problem or kind, matrices or None, [oracle problem per instance])"""
    if not quadratic:
        return dzo.ROSENBROCK_CHAIN, None, [orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype) for _ in range(B)]
    mats = [tw.batch_matrix(orc, n, b, dtype) for b in range(B)]
    return dzo.Problem(dzo.QUADRATIC, n, dtype=dtype, A=mats[0]), np.stack(mats), [orc.Problem(orc.QUADRATIC, n, dtype, A=m) for m in mats]


def _install(batch, states, terminated):
    batch.install_state(**{k: np.stack([s[k] for s in states]) if isinstance(states[0][k], np.ndarray) else [s[k] for s in states]
                           for k in states[0]}, has_terminated=terminated)


def _step_case(n, dtype, quadratic, worst):
    """B = 3, instance 1 terminated; the other two follow an oracle trajectory each, the oracle's state installed before every
    step.  Several starts until enough BFGS steps of the DEVICE have been checked.  In fp32 the oracle's dot products (the two
    norms that scale the searches' first trial step) run in its wide mode: T(double sum), as the device forms them."""
    orc.set_dot_mode(orc.DOT_WIDE if dtype == F32 else orc.DOT_SEQUENTIAL)
    try:
        return _step_case_run(n, dtype, quadratic, worst)
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)


def _step_case_run(n, dtype, quadratic, worst):
    need = 2 if n >= 512 else 3
    checked = 0
    kind, mats, probs = _problems(n, dtype, quadratic, 3)
    for k in range(len(tw.BATCH_SEEDS)):
        X0 = np.stack([tw.batch_start(orc, n, dtype, k, b, quadratic) for b in range(3)])
        refs = [orc.BFGS(probs[b], X0[b].copy(), 1.0) for b in range(3)]
        batch = dzo.BatchedBFGS(kind, X0, 1.0, matrices=mats)
        assert batch.dtype == np.dtype(dtype)
        live = [0, 2]
        for it in range(tw.batch_steps(n)):
            live = [b for b in live if not refs[b].has_terminated]
            if not live:
                break
            _install(batch, [_oracle_state(r) for r in refs], [0 if b in live else 1 for b in range(3)])
            old = _batch_read(batch)
            f_before = [r.current_objective_value for r in refs]
            batch.step(1, poll=False)
            for b in live:
                refs[b].step()
            new = _batch_read(batch)
            for b in range(3):
                where = (n, np.dtype(dtype).name, "quadratic" if quadratic else "rosenbrock", k, it, b)
                if b not in live:
                    for key in FIELDS:
                        assert _same(old[key][b], new[key][b]), (where, key, "a terminated instance changed")
                    continue
                if new["has_terminated"][b]:                       # no step to check; the oracle has to agree (fp32: counted)
                    _against_oracle(refs[b], f_before[b], _one(new, b), worst, where)
                    live.remove(b)
                    continue
                took = _check_device_step(_one(old, b), _one(new, b), probs[b], worst, where)
                _against_oracle(refs[b], f_before[b], _one(new, b), worst, where)
                checked += took == "bfgs"
                if took == "cancelled":
                    live.remove(b)
        batch.close()
        if checked >= need:
            break
    assert checked >= need, (checked, need)
    assert worst.differed <= 1, worst.differed
    return checked


# ------------------------------------------------------------------------------ 1. a step from the oracle's state
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", tw.BATCH)
def test_step_from_the_oracles_state_rosenbrock(n, dtype):
    worst = _Worst(n, dtype)
    checked = _step_case(n, dtype, False, worst)
    f = tw.batch_form(n, dtype)
    worst.report(f"batched step n={n} {np.dtype(dtype).name} rosenbrock, {checked} BFGS steps, {f.lds_bytes} bytes of LDS"
                 + (" (attribute)" if f.needs_attribute else ""))


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", tw.BATCH_ONE_PER_FORM)
def test_step_from_the_oracles_state_quadratic_one_matrix_per_instance(n, dtype):
    worst = _Worst(n, dtype)
    checked = _step_case(n, dtype, True, worst)
    worst.report(f"batched step n={n} {np.dtype(dtype).name} quadratic, {checked} BFGS steps")


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", tw.BATCH_ONE_PER_FORM)
def test_forced_gradient_descent_step_resets_every_element_of_H(n, dtype):
    """d = -g makes the BFGS search climb, so the step is a gradient-descent one: H, installed as a symmetric guard pattern,
    must come back as exactly the identity -- the reset wrote every lower-triangle element, the mirror every upper one."""
    worst = _Worst(n, dtype)
    kind, mats, probs = _problems(n, dtype, False, 3)
    X0 = np.stack([tw.batch_start(orc, n, dtype, 0, b) for b in range(3)])
    batch = dzo.BatchedBFGS(kind, X0, 1.0)
    states = [_oracle_state(orc.BFGS(probs[b], X0[b].copy(), 1.0)) for b in range(3)]
    i = np.arange(n)
    guard = (-(2.0 ** 20) - (i[:, None] + i[None, :]) - 1000.0 * np.abs(i[:, None] - i[None, :])).astype(dtype)
    assert _same(guard, guard.T) and not (guard == 0).any() and not (guard == 1).any()
    for s in states:
        s["d"], s["H"] = -s["g"], guard
    _install(batch, states, [0, 1, 0])
    old = _batch_read(batch)
    batch.step(1, poll=False)
    new = _batch_read(batch)
    for b in (0, 2):
        assert _check_device_step(_one(old, b), _one(new, b), probs[b], worst, (n, np.dtype(dtype).name, b)) == "gd"
    for key in FIELDS:
        assert _same(old[key][1], new[key][1]), key
    batch.close()
    worst.report(f"forced gradient-descent step n={n} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------ 2. one launch or many
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", tw.BATCH_ONE_PER_FORM)
def test_four_steps_in_one_launch_are_four_launches_of_one_step(n, dtype):
    """step(4) against four step(1), H read (and so mirrored) after each: the LDS vectors carried from step to step inside a
    launch, a stale upper triangle under consecutive updates, and a mirror that leaves the lower triangle alone."""
    X0 = np.stack([tw.batch_start(orc, n, dtype, 0, b) for b in range(3)])
    one = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, X0, 1.0)
    many = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, X0, 1.0)
    prob, start = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype), _batch_read(one)
    for b in range(3):                                            # batch_init_kernel: f0, g0, H = I, d = g (legacy :762-810)
        s = _one(start, b)
        assert _same(s["x"], X0[b]) and _same(s["g"], prob.grad(X0[b].copy())) and _same(s["d"], s["g"]), (n, b)
        assert _same(s["H"], np.eye(n, dtype=dtype)) and not s["dx"].any() and not s["dg"].any(), (n, b)
        f_ref = LD(prob.eval(X0[b].copy()))
        assert abs(LD(s["f"]) - f_ref) <= (n + 2) * LD(2.0) ** -53 * _objective_terms(prob, X0[b]) + LD(tw.unit_roundoff(dtype)) * abs(f_ref), (n, b)
        assert s["f"] == dtype(s["f"]) and s["last_step_length"] == 1.0 and s["last_step_type"] == dzo.STEP_NULL
        assert s["iteration_count"] == 0 and not s["has_terminated"]
    one.step(4, poll=False)
    for _ in range(4):
        many.step(1, poll=False)
        got = _batch_read(many)
    want = _batch_read(one)
    assert (want["iteration_count"] == 4).all() and (want["last_step_type"] == dzo.STEP_BFGS).any()
    for key in FIELDS:
        assert _same(want[key], got[key]), (n, np.dtype(dtype).name, key)
    one.close(); many.close()
    print(f"\none launch or many n={n} {np.dtype(dtype).name} [{tw.batch_form_name(n, dtype)}]: every field bit for bit after 4 steps")


# ------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", [130, 450])
def test_an_instance_does_not_depend_on_its_place_or_its_neighbours(n, dtype):
    """The same start alone and as the first, the middle and the last of a batch of 7 whose other instances take other step
    types (two of them start with d = -g, a gradient-descent step): the same bits."""
    x = tw.batch_start(orc, n, dtype, 0, 0)
    alone = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, x[None, :], 1.0)
    X0 = np.stack([x if b in (0, 3, 6) else tw.batch_start(orc, n, dtype, 1, b) for b in range(7)])
    seven = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, X0, 1.0)
    g = seven.current_gradient.to_host()
    d = g.copy()
    d[[1, 4]] = -g[[1, 4]]
    seven.next_step_direction.upload(d)
    alone.step(1, poll=False); seven.step(1, poll=False)
    types = seven.last_step_type.to_host()
    assert types[1] == types[4] == dzo.STEP_GRADIENT_DESCENT and types[0] == types[2] == dzo.STEP_BFGS, types
    alone.step(2, poll=False); seven.step(2, poll=False)
    want, got = _batch_read(alone), _batch_read(seven)
    assert want["iteration_count"][0] == 3
    for b in (0, 3, 6):
        for key in FIELDS:
            assert _same(want[key][0], got[key][b]), (n, np.dtype(dtype).name, b, key)
    assert not _same(got["x"][1], got["x"][0]) and not _same(got["x"][2], got["x"][0])
    alone.close(); seven.close()


# ------------------------------------------------------------------------------ 4. a batch beyond a grid's y dimension
def test_reading_H_of_more_than_65535_instances():
    """batch_mirror_kernel takes the instance from blockIdx.y, and the device reports 65535 as a grid's largest y dimension,
    while batch_create_impl accepts any batch.  Measured on the MI355X: the runtime launches dim3(gx, 65539) all the same and
    every instance is mirrored, so the launch stays as it is and this test holds it there.  B = 65536 + 3 instances of n = 2,
    all starts equal but the last three; two steps, H read (and mirrored) after each."""
    n, B = 2, 65536 + 3
    worst = _Worst(n, F64)
    prob = orc.Problem(orc.ROSENBROCK_CHAIN, n)
    X0 = np.tile(tw.batch_start(orc, n, F64, 0, 0), (B, 1))
    for b in range(3):
        X0[B - 3 + b] = tw.batch_start(orc, n, F64, 1, b)
    batch = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, X0, 1.0)
    states = [_batch_read(batch)]
    for _ in range(2):
        batch.step(1, poll=False)
        states.append(_batch_read(batch))
    last = states[-1]
    for key in FIELDS:
        rows = last[key][:65536].reshape(65536, -1)
        assert (rows.view(np.uint8) == rows[:1].view(np.uint8)).all(), key
    for it in (0, 1):
        for b in (0, B - 3, B - 2, B - 1):
            old, new = _one(states[it], b), _one(states[it + 1], b)
            _check_device_step(old, new, prob, worst, (it, b))
            ref = orc.BFGS(prob, old["x"].copy(), 1.0)
            ref.install_state(old["x"], old["g"], old["H"], old["d"], old["f"], old["last_step_length"], old["iteration_count"],
                              old["last_step_type"], old["dx"], old["dg"])
            ref.step()
            _against_oracle(ref, old["f"], new, worst, (it, b))
    batch.close()
    worst.report(f"batch of {B} instances, n={n}")


# ------------------------------------------------------------------------------ 5. two live batches on one instantiation
@pytest.mark.parametrize("big,small", [(1024, 514), (512, 450)])
def test_a_second_smaller_batch_does_not_take_the_first_ones_lds(big, small):
    """Both sizes run the same instantiation with more than 48 KiB of dynamic LDS.  batch_create_impl sets the kernel's
    hipFuncAttributeMaxDynamicSharedMemorySize to the request of the batch being created, so the smaller batch, created
    second, lowers it under the larger one's request.  Measured on the MI355X: the launch of the larger batch is accepted all
    the same and computes the same bits as alone, so batch_create_impl stays as it is and this test holds it there."""
    assert tw.batch_form_name(big, F64) == tw.batch_form_name(small, F64)
    assert tw.batch_form(small, F64).needs_attribute and tw.batch_form(big, F64).lds_bytes > tw.batch_form(small, F64).lds_bytes
    starts = {n: np.stack([tw.batch_start(orc, n, F64, 0, b) for b in range(2)]) for n in (big, small)}
    alone = {}
    for n in (big, small):
        batch = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, starts[n], 1.0)
        batch.step(2, poll=False)
        alone[n] = _batch_read(batch)
        batch.close()
    first = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, starts[big], 1.0)
    second = dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, starts[small], 1.0)
    first.step(2, poll=False)                                     # (a refused launch would raise DzoError before anything ran)
    second.step(2, poll=False)
    for n, batch in ((big, first), (small, second)):
        got = _batch_read(batch)
        assert (got["iteration_count"] == 2).all()
        for key in FIELDS:
            assert _same(alone[n][key], got[key]), (n, key)
    first.close(); second.close()
