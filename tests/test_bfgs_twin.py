"""tests/bfgs_twin.py against things it does not depend on: the replay checker must accept the CPU oracle's
``update_inverse_hessian!`` at every full-storage shape of the GPU tests and reject five kinds of subtly wrong result; the sum
bound must hold for a double-accumulated product and fail when one term is missing; the path functions must say what the
launchers of csrc/dzo_bfgs.hip say.  For the batched kernel of csrc/dzo_batch.hip: the shape table against the source, the
elementwise bound of the update (it accepts a numpy evaluation with its sums in three orders, it rejects four planted errors at a
single element), and the cap on the rows of t whose fp32 rounding the replay has to search.  No GPU."""
import os
import re

import numpy as np
import pytest

import bfgs_twin as tw
from oracle import oracle as orc

LD = np.longdouble
CASES = [(n, np.float64) for n in tw.FULL_F64] + [(n, np.float32) for n in tw.FULL_F32]
ACC = {np.float64: 53, np.float32: 24}                 # the oracle accumulates its sums in T


def _oracle_update(n, dtype, H0=None):
    H0s, d, dg, g, lam = tw.update_inputs(n, dtype)
    H0 = H0s if H0 is None else H0
    H = np.asfortranarray(H0.copy())
    ds = d.copy()
    t = orc.bfgs_update(H, float(lam), ds, dg.copy())
    return dict(H0=H0, d=d, dg=dg, lam=lam, t=t, d_scaled=ds, H_new=np.array(H, order="C"))


def _replay(u, H_new=None, **kw):
    T = u["H0"].dtype.type
    return tw.replay_update(u["H0"], u["d"], u["dg"], u["t"], u["H_new"] if H_new is None else H_new, d_scaled=u["d_scaled"],
                            lam=u["lam"], acc_bits=ACC[T], **kw)


def _next(x, k=1):
    """the value of x's type k values up."""
    a = np.array([x])
    return tw._unordered(tw._ordered(a) + k, a.dtype)[0]


@pytest.mark.parametrize("n,dtype", CASES)
def test_replay_accepts_the_oracle_and_rejects_five_mutants(n, dtype):
    u = _oracle_update(n, dtype)
    H0, H_new = u["H0"], u["H_new"]
    r = _replay(u)
    assert r.ok, r
    assert r.window_overlap <= tw.CAP and r.window_delta <= tw.CAP
    print(f"n={n} {np.dtype(dtype).name}: overlap window {r.window_overlap}, delta window {r.window_delta}, {r.tried} pairs tried")
    # ... and without d_scaled / lam, as on the step path, where only H, d, dg and t can be read
    r2 = tw.replay_update(H0, u["d"], u["dg"], u["t"], H_new, acc_bits=ACC[dtype])
    assert r2.ok and r2.delta == r.delta and np.array_equal(u["d"] * (dtype(1) / r2.overlap), u["d_scaled"])
    rng = np.random.default_rng(n)
    # 1. one element moved by one ulp
    i, j = rng.integers(n), rng.integers(n)
    M = H_new.copy()
    M[i, j] = _next(M[i, j])
    assert not _replay(u, M).ok
    # 2. one column left at H0
    j = rng.integers(n)
    M = H_new.copy()
    M[:, j] = H0[:, j]
    assert not _replay(u, M).ok
    # 3. the last row and column left at H0
    M = H_new.copy()
    M[-1, :] = H0[-1, :]
    M[:, -1] = H0[:, -1]
    assert not _replay(u, M).ok
    # 4. t_i*s_j + s_i*t_j rounded once (what contraction into fma does), everything else as written
    s, t = u["d_scaled"], u["t"]
    once = (np.multiply.outer(t.astype(LD), s.astype(LD)) + np.multiply.outer(s.astype(LD), t.astype(LD))).astype(dtype)
    M = H0 + (r.delta * np.multiply.outer(s, s) - once)
    if np.array_equal(M, H_new):
        assert n <= 3                                   # (n (n - 1) / 2 <= 3 values off the diagonal -- on it 2 t_i s_i is exact --
        #                                                 so few that the two roundings can agree with the one everywhere)
    else:
        assert not _replay(u, M).ok
    # 5. the transpose of a non-symmetric result: H0 not symmetric, so t = H0*dg is not H0'*dg
    if n > 1:
        A = H0.copy()
        A[np.triu_indices(n, 1)] *= dtype(1.25)
        ua = _oracle_update(n, dtype, A)
        assert _replay(ua).ok
        assert not np.array_equal(ua["H_new"], ua["H_new"].T)
        assert not _replay(ua, ua["H_new"].T).ok


def test_replay_rejects_an_overlap_off_by_one_value_and_a_delta_outside_its_bound():
    """d_scaled from a neighbouring overlap: :874 is checked by itself; and a delta that reproduces H but is not
    lam*overlap + dg.t (a wrong lam) fails the check that comes afterwards."""
    u = _oracle_update(129, np.float64)
    r = _replay(u)
    bad = dict(u, d_scaled=u["d"] * (1.0 / _next(r.overlap, 3 * tw.CAP)))
    assert not _replay(bad).ok
    wrong_lam = dict(u, lam=np.float64(0.38))
    rr = _replay(wrong_lam)
    assert not rr.ok and "bound" in rr.reason


def test_a_window_beyond_the_cap_fails_instead_of_being_skipped():
    rng = np.random.default_rng(3)
    n = 64
    H0 = tw.spd(n, 3, np.float64)
    d = rng.standard_normal(n)
    dg = rng.standard_normal(n)
    dg -= d * (d @ dg) / (d @ d) * (1 - 1e-9)            # overlap cancels to 1e-9 of its terms
    r = tw.replay_update(H0, d, dg, H0 @ dg, H0.copy())
    assert not r.ok and r.window_overlap > tw.CAP and "cap" in r.reason


def test_candidates_are_the_nearest_value_then_its_neighbours_outward():
    for dtype in (np.float32, np.float64):
        c = tw.candidates(LD(1) / 3, 3, dtype)
        x = dtype(LD(1) / 3)
        assert c.dtype == dtype and c[0] == x and list(c[1::2]) == [_next(x, k) for k in (1, 2, 3)]
        assert list(c[2::2]) == [_next(x, -k) for k in (1, 2, 3)]
        assert c[1] == np.nextafter(x, dtype(1)) and c[2] == np.nextafter(x, dtype(0))
        c = tw.candidates(-LD(2.0) ** -3, 2, dtype)       # negative, across a binade edge
        assert c[0] == dtype(-0.125) and c[1] == np.nextafter(dtype(-0.125), dtype(0)) and c[2] == np.nextafter(dtype(-0.125), dtype(-1))
        assert tw.ulp(1.0, dtype) == np.finfo(dtype).eps and tw.ulp(1.9999, dtype) == np.finfo(dtype).eps
        assert tw.ulp(0.75, dtype) == np.finfo(dtype).eps / 2 and tw.ulp(-2.0, dtype) == 2 * np.finfo(dtype).eps


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 7, 513, 1028])
def test_sum_bound_holds_for_a_double_accumulated_product_and_sees_a_missing_term(n, dtype):
    rng = np.random.default_rng(n)
    H = tw.spd(n, n, dtype)
    v = rng.standard_normal(n).astype(dtype)
    exact, S = tw.exact_matvec(H, v)
    bound = tw.sum_bound(H, v, n, dtype)
    got = (H.astype(np.float64) @ v.astype(np.float64)).astype(dtype)          # double accumulation, one rounding to T
    assert (np.abs(got.astype(LD) - exact) <= bound).all()
    # sequential and reversed orders too: the bound is for ANY order
    for order in (np.arange(n), np.arange(n)[::-1]):
        acc = np.zeros(n)
        for j in order:
            acc += H[:, j].astype(np.float64) * float(v[j])                    # (H symmetric: column j is row j)
        assert (np.abs(acc.astype(dtype).astype(LD) - exact) <= bound).all()
    # one term of one row dropped: the largest of row n // 2
    i = n // 2
    j = int(np.argmax(np.abs(H[i].astype(LD) * v.astype(LD))))
    if n > 1:
        Hm = H.astype(np.float64)
        Hm[i, j] = 0
        bad = (Hm @ v.astype(np.float64)).astype(dtype)
        err = np.abs(bad.astype(LD) - exact)
        assert err[i] > bound[i] and (np.delete(err, i) <= np.delete(bound, i)).all()


def test_mfma_bound_holds_for_an_fma_chain_and_sees_a_skipped_tile():
    n = 80
    u = _oracle_update(n, np.float64)
    exact, bound = tw.mfma_bound(u["H0"], u["d_scaled"], u["t"], u["lam"], tw.overlap_candidates(u["d"], u["dg"], 53, u["d_scaled"])[0][0], u["dg"])
    assert (np.abs(u["H_new"].astype(LD) - exact) <= bound).all()           # the reference's own rounding is inside it
    M = u["H_new"].copy()
    M[16:32, 48:64] = u["H0"][16:32, 48:64]
    assert (np.abs(M.astype(LD) - exact) > bound)[16:32, 48:64].any()


# ------------------------------------------------------------------------------ which instantiation runs
def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "dzoptimization.jl_amd", "csrc", name)) as f:
        return f.read()


def test_path_functions_restate_the_launchers():
    """The three ``vec`` conditions and ``o->tri`` as the source states them; a change to a launcher has to change
    bfgs_twin.VEC_OPERANDS / takes_tri knowingly.

    Deliberately tied to the source text: whole lines and a regex over the ``vec`` conditions.  When this fails after an edit
    of dzo_bfgs.hip or dzo_common.h, first decide whether the conditions changed -- then update VEC_OPERANDS / takes_tri and
    the shape tables' comments -- and only then the strings below; a pure reformat needs the strings alone."""
    src = _source("dzo_bfgs.hip")
    conds = re.findall(r"const bool vec = \(n % Vec16<T>::N == 0\)((?: && (?:al16\(\w+\)|\(!g \|\| al16\(g\)\)))+);", src)
    assert len(conds) == 3                                                  # launch_symv, launch_bfgs_update_fused, launch_bfgs_update
    names = [tuple(re.findall(r"al16\((\w+)\)", c)) for c in conds]
    assert names == [tw.VEC_OPERANDS["symv"], tw.VEC_OPERANDS["fused"], tw.VEC_OPERANDS["update"]]
    assert "o->tri = !o->no_hessian && o->n % 2 == 0 && big && o->n < 65535LL * kTriCW;" in src
    assert 'const int min_n = tune_int("DZO_TUNE_BFGS_TRI_MIN_N", INT_MIN);' in src                 # (INT_MIN: the variable is unset)
    assert "const bool big = min_n != INT_MIN ? o->n >= min_n : (size_t)o->n * (size_t)o->n * es >= (128u << 20);" in src
    assert re.search(r"constexpr int kTriCW = 32;", src) and tw.TRI_MAX_N == 65535 * 32 and tw.TRI_DEFAULT_BYTES == 128 << 20
    common = _source("dzo_common.h")
    assert "Vec16<double> { using type = double2; static constexpr int N = 2; }" in common
    assert "Vec16<float>  { using type = float4;  static constexpr int N = 4; }" in common
    # the restatement, over a grid
    for dtype, per in ((np.float64, 2), (np.float32, 4)):
        for n in range(1, 40):
            for launcher, ops in tw.VEC_OPERANDS.items():
                assert tw.takes_vec(n, dtype, launcher) == (n % per == 0)
                for op in ("H", "d", "dg", "scratch", "g", "v"):
                    assert tw.takes_vec(n, dtype, launcher, (op,)) == (n % per == 0 and op not in ops)
        es = np.dtype(dtype).itemsize
        for n in (2, 3, 30, 31, 1024, 2050, 4095, 4096, 5792, 5794, 65535 * 32 - 2, 65535 * 32):
            assert tw.takes_tri(n, dtype) == (n % 2 == 0 and n * n * es >= 128 * 2 ** 20 and n < 65535 * 32)
            for m in (2, 32, 4096):
                assert tw.takes_tri(n, dtype, m) == (n % 2 == 0 and n >= m and n < 65535 * 32)
    # what the tables are meant to run
    assert [tw.takes_vec(n, np.float64, "fused") for n in (3, 5, 7, 129, 513, 1025, 4, 8, 512, 1028)] == [False] * 6 + [True] * 4
    assert [tw.takes_vec(n, np.float32, "fused") for n in (3, 5, 7, 129, 513, 1025, 4, 8, 512, 1028)] == [False] * 6 + [True] * 4
    assert all(tw.takes_tri(n, dt, 2) for n in tw.TRI for dt in (np.float32, np.float64))
    assert not any(tw.takes_tri(n, np.float64) for n in tw.FULL_F64 + tw.TRI)         # the default keeps them on full storage
    assert all(n % 16 == 0 for n in tw.MFMA) and [n // 16 for n in tw.MFMA] == [1, 3, 5, 7, 16]


# ------------------------------------------------------------------------------ the batched kernel (csrc/dzo_batch.hip)
F64, F32 = np.float64, np.float32
STEP_BFGS = 2


def test_batch_form_restates_the_source_at_every_table_entry():
    """rp, the wide form, UJ and the LDS request as batch_create_impl and batch_step_kernel state them (whole lines of the
    source: a change there has to change bfgs_twin.batch_form knowingly), the form each entry of BATCH is listed under, and the
    table's promise: the first and last size of every form and both sides of both 48 KiB edges."""
    src = _source("dzo_batch.hip")
    assert "b->rp = n <= 256 ? 1 : (n <= 512 ? 2 : 4);" in src
    assert 'b->wide = (b->rp == 2 && n > tune_int("DZO_TUNE_BATCH_RP2_WIDE_ABOVE", 448)) ? 1 : 0;' in src
    assert "b->lds_bytes = 9 * np * es + (5 * np + 16) * sizeof(double) + 16;" in src
    assert "constexpr int UJ = RP == 1 ? 4 : (RP == 2 ? (WIDE ? 4 : 2) : 2);" in src
    assert "if (b->lds_bytes > 48 * 1024) {" in src
    stated = {"rp1": [2, 4, 6, 8, 10, 14, 16, 18, 30, 32, 34, 62, 64, 66, 126, 128, 130, 254, 256],
              "rp2 narrow": [258, 260, 262, 264, 266, 384, 436, 438, 446, 448],
              "rp2 wide": [450, 510, 512],
              "rp4": [514, 516, 644, 646, 768, 770, 1022, 1024]}
    assert tw.BATCH == sum((stated[f] for f in tw.BATCH_FORMS), [])
    want = {"rp1": (1, False, 4), "rp2 narrow": (2, False, 2), "rp2 wide": (2, True, 4), "rp4": (4, False, 2)}
    for dtype, es in ((F64, 8), (F32, 4)):
        for name, sizes in stated.items():
            for n in sizes:
                f = tw.batch_form(n, dtype)
                assert (f.rp, f.wide, f.uj) == want[name] and tw.batch_form_name(n, dtype) == name, (n, f)
                assert f.lds_bytes == 9 * n * es + (5 * n + 16) * 8 + 16 and f.needs_attribute == (f.lds_bytes > 49152)
                assert n <= 256 * f.rp                                      # every row pair has a thread
        # first and last size of each form: the even n either side of it takes another form
        for name, sizes in stated.items():
            lo, hi = sizes[0], sizes[-1]
            assert lo == 2 or tw.batch_form_name(lo - 2, dtype) != name
            assert hi == 1024 or tw.batch_form_name(hi + 2, dtype) != name
        # the attribute edge: the last size without and the first with it are both in the table
        edge = [n for n in range(2, 1026, 2) if tw.batch_form(n, dtype).needs_attribute][0]
        assert edge == (438 if dtype == F64 else 646) and edge in tw.BATCH and edge - 2 in tw.BATCH
    assert [tw.batch_form_name(n, F64) for n in tw.BATCH_ONE_PER_FORM] == list(tw.BATCH_FORMS)
    assert all(n in tw.BATCH for n in tw.BATCH_ONE_PER_FORM)


def _batch_oracle(n, dtype, k, b, quadratic):
    if quadratic:
        prob = orc.Problem(orc.QUADRATIC, n, dtype, A=tw.batch_matrix(orc, n, b, dtype))
    else:
        prob = orc.Problem(orc.ROSENBROCK_CHAIN, n, dtype)
    return orc.BFGS(prob, tw.batch_start(orc, n, dtype, k, b, quadratic), 1.0)


def _batch_oracle_updates(n, dtype, k, b, quadratic=False, steps=None):
    """(H0, d, dg, lam) of every BFGS step of one oracle trajectory; lam = T(-last_step_length / ||d||), close to the oracle's."""
    ref = _batch_oracle(n, dtype, k, b, quadratic)
    out = []
    for _ in range(tw.batch_steps(n) if steps is None else steps):
        if ref.has_terminated:
            break
        H0, d = np.ascontiguousarray(ref.approximate_inverse_hessian), ref.next_step_direction.copy()
        ref.step()
        if ref.last_step_type == STEP_BFGS and not ref.has_terminated:
            lam = dtype(-LD(ref.last_step_length) / LD(tw.device_norm(d)))
            out.append((H0, d, ref.delta_gradient.copy(), lam))
    return out


def _sum_forward(a):
    return np.cumsum(a, axis=-1)[..., -1]


def _sum_reversed(a):
    return np.cumsum(a[..., ::-1], axis=-1)[..., -1]


def _sum_halves(a):
    m = a.shape[-1]
    return a[..., 0] if m == 1 else _sum_halves(a[..., :m // 2]) + _sum_halves(a[..., m // 2:])


def _as_the_kernel(H0, d, dg, lam, wide_sum):
    """The update in numpy as the batched kernel evaluates it: the three sums in double (``wide_sum`` gives the order) rounded
    once to T, every other operation in T.  Returns (H_new, s, t, delta)."""
    T = H0.dtype.type
    D = np.float64
    t = wide_sum(H0.astype(D) * dg.astype(D)[None, :]).astype(T)
    overlap = T(wide_sum(d.astype(D) * dg.astype(D)))
    dgt = T(wide_sum(dg.astype(D) * t.astype(D)))
    inv = T(1) / overlap
    delta = lam * overlap + dgt
    s = d * inv
    return tw.update_expression(H0, s, t, delta), s, t, delta


@pytest.mark.parametrize("quadratic", [False, True], ids=["rosenbrock", "quadratic"])
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n", [6, 130, 258, 514])
def test_batch_update_bound_accepts_three_summation_orders_and_rejects_four_planted_errors(n, dtype, quadratic):
    ups = _batch_oracle_updates(n, dtype, 0, 0, quadratic, steps=3)
    assert len(ups) >= 2
    worst, seen = 0.0, {k: 0.0 for k in ("left out", "twice", "t from j + 1", "partner of the straddling pair")}
    for H0, d, dg, lam in ups:
        if tw.overlap_cancellation(d, dg) > 100:
            continue
        exact, bound = tw.batch_update_bound(H0, d, dg, lam, dtype)
        assert np.array_equal(bound, bound.T) and (bound > 0).all()
        for wide_sum in (_sum_forward, _sum_reversed, _sum_halves):
            H_new, s, t, delta = _as_the_kernel(H0, d, dg, lam, wide_sum)
            ratio = float((np.abs(H_new.astype(LD) - exact) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (n, wide_sum.__name__, ratio)
        # one lower-triangle element of the (last, pairwise) result wrong in four ways, each at the element where it shows best
        lower = np.tril(np.ones((n, n), bool), -1)
        t_next = np.roll(t, -1)                                                # t_{j + 1} in place of t_j (the last column wraps)
        shifted = H0 + (delta * np.multiply.outer(s, s) - (np.multiply.outer(t, s) + np.multiply.outer(s, t_next)))
        sub = np.zeros((n, n), bool)
        sub[np.arange(1, n, 2), np.arange(0, n - 1, 2)] = True                  # (j, j - 1), j odd: the partner of the pair (j - 1, j)
        plants = {"left out": (H0, lower), "twice": (H_new + (H_new - H0), lower), "t from j + 1": (shifted, lower),
                  "partner of the straddling pair": (H0, sub)}
        for name, (wrong, where) in plants.items():
            score = np.where(where, np.abs(wrong.astype(LD) - H_new.astype(LD)) / bound, 0)
            i, j = np.unravel_index(int(np.argmax(score)), score.shape)
            M = H_new.copy()
            M[i, j] = wrong[i, j]
            over = np.abs(M.astype(LD) - exact) > bound
            assert over[i, j] and over.sum() == 1, (n, name, i, j, float(score[i, j]))
            seen[name] = max(seen[name], float((score[where] > 2).mean()))
    assert worst > 0
    print(f"\nn={n} {np.dtype(dtype).name} {'quadratic' if quadratic else 'rosenbrock'}: worst error/bound over three orders {worst:.3f}; "
          + "share of the elements at which it is seen for certain: " + ", ".join(f"{k} {v:.2f}" for k, v in seen.items()))


@pytest.mark.parametrize("n", tw.BATCH)
def test_undecided_rows_of_t_stay_under_the_cap_on_the_trajectories_of_the_gpu_test(n):
    """The fp32 replay searches 2^k values of t for k undecided rows: k <= UNDECIDED_CAP at every step of every trajectory the
    GPU test follows (expected: about n 2^-29 per row, so none).  And t_rounded does report a row that sits on a tie."""
    most = 0
    orc.set_dot_mode(orc.DOT_WIDE)                                            # as the GPU test runs the fp32 oracle
    try:
        for k in range(len(tw.BATCH_SEEDS)):
            for b in (0, 2):
                for H0, d, dg, lam in _batch_oracle_updates(n, F32, k, b):
                    t, undecided = tw.t_rounded(H0, dg)
                    most = max(most, len(undecided))
                    assert len(undecided) <= tw.UNDECIDED_CAP, (n, k, b, undecided)
    finally:
        orc.set_dot_mode(orc.DOT_SEQUENTIAL)
    print(f"\nn={n}: at most {most} undecided rows per step")


def test_t_rounded_reports_a_tie_and_the_replay_searches_it():
    H0 = np.array([[1, 2.0 ** -24], [2.0 ** -24, 1]], F32)                      # row 0: 1 + 2^-24, exactly between 1 and 1 + 2^-23
    dg = np.array([1, 1], F32)
    t, undecided = tw.t_rounded(H0, dg)
    assert t[0] == F32(1) and len(undecided) == 2 and undecided[0][0] in (0, 1)
    assert {(i, float(v)) for i, v in undecided} == {(0, 1 + 2.0 ** -23), (1, 1 + 2.0 ** -23)}
    d = np.array([0.5, 0.25], F32)
    lam = F32(-0.5)
    for t_dev in (np.array([1, 1], F32), np.array([1 + 2.0 ** -23, 1], F32), np.array([1 + 2.0 ** -23, 1 + 2.0 ** -23], F32)):
        overlap = F32(d @ dg)
        H_new = tw.update_expression(H0, d * (F32(1) / overlap), t_dev, lam * overlap + F32(dg @ t_dev))
        assert tw.replay_update_undecided(H0, d, dg, t, undecided, H_new, lam=lam).ok
    H_bad = H_new.copy()
    H_bad[1, 0] = np.nextafter(H_bad[1, 0], F32(9))
    assert not tw.replay_update_undecided(H0, d, dg, t, undecided, H_bad, lam=lam).ok
