"""The CPU twin of the transition-state candidates (tests/pathway_twin.py) against things it does not depend on: hand-made
profiles with the answer written down, a tangent formed in longdouble, and the properties of the compaction.  No device."""
import numpy as np
import pytest

import pathway_twin as pw


@pytest.mark.parametrize("profile, expected", [
    ([0, 1, 2, 3, 4], []),                                   # rising
    ([4, 3, 2, 1, 0], []),                                   # falling
    ([0, 2, 1, 0, -1], [1]),                                 # a peak at image 1
    ([0, 1, 2, 3, 1], [3]),                                  # a peak at image M - 2
    ([0, 1, 3, 3, 1], [2]),                                  # a plateau: its first image only
    ([0, 3, 3, 1, 0], [1]),                                  # ... whose second image equals its left neighbour: no candidate
    ([3, 3, 1, 0, 0], []),                                   # E_1 == E_0: not a candidate, and the ends never are
    ([0, 1, 0, 1, 0], [1, 3]),                               # alternating
    ([0, 1, 0, 1, 1], [1, 3]),                               # >= towards the right end
    ([9, 1, 0, 1, 9], []),                                   # the ends are the highest: never candidates
    ([0, np.nan, 0, 0, 0], []),                              # a NaN is no candidate ...
    ([0, 1, np.nan, 1, 0], []),                              # ... and makes none of its neighbours
    ([0, 1, 0], [1]), ([0, 0, 0], []), ([1, 1, 0], []), ([0, 1, 1], [1]),
])
def test_candidate_rule_on_hand_made_profiles(profile, expected):
    for dtype in (np.float32, np.float64):
        assert pw.candidate_images(np.array(profile, dtype=dtype)) == expected


@pytest.mark.parametrize("M", [3, 4, 5, 32])
def test_profile_kinds_have_the_candidates_they_are_named_for(M):
    e, kinds = pw.profiles(len(pw.KINDS), M, np.float64, seed=M)
    found = {k: pw.candidate_images(e[b]) for b, k in enumerate(kinds)}
    mid = max(1, (M - 2) // 2)
    assert found["rising"] == found["falling"] == found["nan"] == found["valley"] == []
    assert found["peak_first"] == [1] and found["peak_last"] == [M - 2]
    assert found["plateau"] == [mid] and e[kinds.index("plateau"), mid] == e[kinds.index("plateau"), mid + 1]
    b = kinds.index("equal_left")
    assert e[b, mid] == e[b, mid - 1] and mid not in found["equal_left"]
    assert found["equal_left"] == ([mid - 1] if mid - 1 >= 1 else [])
    assert found["alternating"] == list(range(1, M - 1, 2)) and len(found["alternating"]) == (M - 1) // 2
    assert np.isnan(e[kinds.index("nan")]).sum() == 1


def test_no_band_holds_more_than_half_its_images():
    rng = np.random.default_rng(5)
    for M in (3, 4, 7, 32):
        for _ in range(200):
            e = rng.integers(0, 4, size=M).astype(np.float64)    # many ties
            c = pw.candidate_images(e)
            assert len(c) <= (M - 1) // 2 and all(q - p >= 2 for p, q in zip(c, c[1:])), (e, c)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_particles", [1, 7, 65])
def test_compaction_order_and_tangents(dtype, n_particles):
    dt = np.dtype(dtype)
    batch, M = 2 * len(pw.KINDS), 6
    rng = np.random.default_rng(n_particles)
    band = rng.normal(size=(batch, M, 3 * n_particles)).astype(dt)
    e, _ = pw.profiles(batch, M, dt, seed=1)
    out = pw.candidates(band, e, dt)
    assert out["count"] == out["offsets"][-1] == len(out["band_index"]) > 0 and out["offsets"][0] == 0
    per_band = [len(pw.candidate_images(e[b])) for b in range(batch)]
    assert np.array_equal(np.diff(out["offsets"]), per_band) and 0 in per_band[1:-1]
    keys = list(zip(out["band_index"].tolist(), out["image_index"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                       # band-major, images ascending
    eps = np.finfo(dt).eps
    for c, (b, m) in enumerate(keys):
        assert out["offsets"][b] <= c < out["offsets"][b + 1]
        assert np.array_equal(out["points"][c], band[b, m]) and out["energies"][c] == e[b, m]
        # the tangent once more in longdouble: a candidate always takes the energy-weighted mix
        L = np.longdouble
        dp, dm = band[b, m + 1].astype(L) - band[b, m].astype(L), band[b, m].astype(L) - band[b, m - 1].astype(L)
        ar, al = abs(L(e[b, m + 1]) - L(e[b, m])), abs(L(e[b, m - 1]) - L(e[b, m]))
        hi, lo = max(ar, al), min(ar, al)
        t = hi * dp + lo * dm if e[b, m + 1] > e[b, m - 1] else lo * dp + hi * dm
        tau = t / np.sqrt((t * t).sum())
        # d+, d- and the weights are rounded in T before they are mixed: a few eps of T relative to the unit tangent
        assert np.abs(out["tangents"][c].astype(L) - tau).max() <= 16 * eps * max(1.0, float(np.abs(dp).max() + np.abs(dm).max()) * float(hi) / float(np.sqrt((t * t).sum())))
        assert abs(float(np.sqrt((out["tangents"][c].astype(np.float64) ** 2).sum())) - 1.0) <= 4 * eps * np.sqrt(3 * n_particles)
