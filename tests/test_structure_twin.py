"""CPU checks of tests/structure_twin.py against things it does not depend on: the fingerprint of a cluster and of its image
under a rigid motion, a reflection and a relabelling agree to the derived rounding bounds; the bit-exact rows agree with the
longdouble rows of pairwise_twin; the greedy labels name representatives on a non-transitive chain; non-finite fingerprints
get -1; known structures placed first keep their indices.  No GPU."""
import numpy as np
import pytest

import pairwise_twin as tw
import quench_twin as qt
import structure_twin as st

DTYPES = [np.float64, np.float32]


def _cluster(n, seed):
    return np.concatenate(tw.jittered(tw.cluster(n, seed), seed + 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [13, 38, 70])
def test_fingerprint_is_invariant_to_the_rounding_bound(n, dtype):
    """|fp(cluster) - fp(image)| per element is at most gamma_N sum_j |e_ij| for the energies (the largest over i, on both
    sides: sorting is 1-Lipschitz in the largest difference) and gamma_N sum_c (|r_ic| + |c_c|)^2 for the distances, with
    gamma_N = N eps / (1 - N eps) and eps the unit roundoff of the element type."""
    p = np.asarray(_cluster(n, 3), dtype=dtype).astype(np.float64)
    q = np.asarray(st.image(p, seed=11 + n), dtype=dtype).astype(np.float64)
    fp, Ep = st.fingerprint(p, dtype)
    fq, Eq = st.fingerprint(q, dtype)
    g = st.gamma(n, dtype)
    bound_e = g * float(max(st.row_scales(p)[1].max(), st.row_scales(q)[1].max()))
    bound_d = g * float(max(st.distance_scales(p)[1].max(), st.distance_scales(q)[1].max()))
    err_e = np.abs(fp[:n].astype(np.float64) - fq[:n].astype(np.float64)).max()
    err_d = np.abs(fp[n:].astype(np.float64) - fq[n:].astype(np.float64)).max()
    print("n = %d %s: energies differ by %.3e (bound %.3e), distances by %.3e (bound %.3e)" % (n, np.dtype(dtype).name, err_e, bound_e, err_d, bound_d))
    assert 0 < bound_e and 0 < bound_d
    assert err_e <= bound_e and err_d <= bound_d
    assert abs(float(Ep) - float(Eq)) <= n * bound_e
    assert not np.array_equal(np.asarray(p, dtype=dtype), np.asarray(q, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_and_energy_agree_with_the_longdouble_sums(dtype):
    n = 38
    p = np.asarray(_cluster(n, 5), dtype=dtype).astype(np.float64)
    fp, E, e, d = st.fingerprint(p, dtype, parts=True)
    exact, S = st.row_scales(p)
    # the pair term itself carries a few roundings on top of the sum's: (N + 32) eps, the bound of quench_twin.decision_margin
    assert np.all(np.abs(e.astype(np.longdouble) - exact) <= (n + 32) * st.EPS[np.dtype(dtype)] * S)
    E_exact, S_all = qt.exact_energy(p)
    assert abs(np.longdouble(E) - E_exact) <= (n + 32) * st.EPS[np.dtype(dtype)] * S_all
    dd, D = st.distance_scales(p)
    assert np.all(np.abs(d.astype(np.longdouble) - dd) <= st.gamma(n, dtype) * D)
    assert np.array_equal(fp[:n], np.sort(e)) and np.array_equal(fp[n:], np.sort(d))
    assert np.all(np.diff(fp[:n]) >= 0) and np.all(np.diff(fp[n:]) >= 0)
    if np.dtype(dtype) == np.float64:                        # the fp64 energy of the quench twin, to rounding
        assert abs(float(E) - float(qt.energy_gradient(p, dtype)[0])) <= 1e-12 * abs(float(E))


def test_sort_puts_values_that_are_not_numbers_last():
    p = _cluster(13, 1)
    p[5], p[13 + 5], p[26 + 5] = p[2], p[13 + 2], p[26 + 2]   # one coincident pair
    fp, E = st.fingerprint(p, np.float64)
    assert np.isnan(fp[11]) and np.isnan(fp[12]) and np.all(np.isfinite(fp[:11])) and np.all(np.isfinite(fp[13:]))
    assert np.isnan(E)


def test_greedy_labels_on_a_chain_name_representatives():
    a, b, c = np.zeros(4), np.zeros(4), np.zeros(4)
    b[2], c[2] = 0.6e-3, 1.2e-3                              # a ~ b, b ~ c, a !~ c at tol = 1e-3
    F = np.stack([a, b, c])
    assert st.matches(a, b, 1e-3)[0] and st.matches(b, c, 1e-3)[0] and not st.matches(a, c, 1e-3)[0]
    labels, reps = st.classify(F, 1e-3)
    assert labels.tolist() == [0, 0, 2] and reps.tolist() == [0, 2]


def test_the_match_rule_is_relative_above_one_and_absolute_below():
    assert st.matches([100.0], [100.05], 1e-3)[0] and not st.matches([100.0], [100.2], 1e-3)[0]
    assert st.matches([0.01], [0.0109], 1e-3)[0] and not st.matches([0.01], [0.0111], 1e-3)[0]
    assert st.matches([1.0, 2.0], [1.0, 2.0], 0.0)[0]
    assert st.relative_distance([100.0, 0.0], [100.2, 0.0]) == pytest.approx(0.2 / 100.2)


def test_non_finite_fingerprints_get_minus_one_and_never_lead():
    F = np.array([[1.0, np.nan], [1.0, 2.0], [np.inf, 2.0], [1.0, 2.0], [np.inf, 2.0]])
    labels, reps = st.classify(F, 1e-6)
    assert labels.tolist() == [-1, 1, -1, 1, -1] and reps.tolist() == [1]
    assert not st.matches(F[2], F[4], 1.0)[0]               # inf <= tol * inf would pass without the finiteness rule


def test_known_structures_placed_first_keep_their_indices():
    rng = np.random.default_rng(0)
    known = [st.fingerprint(_cluster(13, s), np.float64)[0] for s in (1, 2, 3)]
    found = [st.fingerprint(st.image(_cluster(13, s), seed=s), np.float64)[0] for s in (3, 7, 1, 3, 7)]
    tol = 1e-9
    labels, reps = st.classify(np.stack(known + found), tol)
    assert labels.tolist() == [0, 1, 2, 2, 4, 0, 2, 4] and reps.tolist() == [0, 1, 2, 4]
    order = rng.permutation(5)
    labels2, _ = st.classify(np.stack(known + [found[k] for k in order]), tol)
    assert labels2[:3].tolist() == [0, 1, 2]
