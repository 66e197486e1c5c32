"""The candidate unit on the device (csrc/dzo_pathway.hip) against its CPU twin (tests/pathway_twin.py) and against the band
unit, and the connect cycle built on it (``dzo.connect_pathways``) end to end on LJ7 and LJ13.

No tolerance in the first half: offsets, indices, points, energies and tangents are compared as bit patterns with the twin (the
header states the candidate rule, every fma and the order of the sum; the library is built without contraction), a band alone
against the same band inside a batch, and a candidate's tangent against the tangent ``neb_apply`` records for that image.  Every
output of the C entry point is a window inside a larger array of canaries.

The second half checks what a reported pathway claims, not how many pairs connect (except on LJ7 in float64, where the float64
CPU restatement of the cycle connects all six pairs in its first cycle and the test asks for all six within three):
tests/pathway_cases.py has the checks, which go through numpy's own Lennard-Jones energy and gradient.  The counts are printed."""
import ctypes
import functools

import numpy as np
import pytest

import pathway_cases as pc
import pathway_twin as pw
from dzo_loader import dzo

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
CANARY = 12345.0
GUARD = 64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _guarded(shape, np_dtype):
    size = int(np.prod(shape))
    buf = dzo.DeviceArray.from_host(np.full(size + 2 * GUARD, CANARY, dtype=np_dtype))
    return buf, buf.view(GUARD, shape)


def _guards_hold(buffers, written=True):
    for name, (buf, window) in buffers.items():
        h = buf.to_host()
        assert np.all(h[:GUARD] == h.dtype.type(CANARY)) and np.all(h[-GUARD:] == h.dtype.type(CANARY)), name + ": wrote outside its output"
        if written:
            assert not np.any(window.to_host() == h.dtype.type(CANARY)), name + ": an element of the output was not written"


def _candidates(band, energies, n, capacity):
    """The C entry point on host arrays (batch, M, 3n) and (batch, M) with guarded outputs of `capacity` rows:
    (return code, count, dict of host arrays, the guarded buffers)."""
    batch, m, _ = band.shape
    dt = band.dtype
    dband, de = dzo.DeviceArray.from_host(band), dzo.DeviceArray.from_host(energies)
    out = {"points": _guarded((capacity, 3 * n), dt), "tangents": _guarded((capacity, 3 * n), dt), "energies": _guarded((capacity,), dt),
           "band_index": _guarded((capacity,), np.int32), "image_index": _guarded((capacity,), np.int32),
           "offsets": _guarded((batch + 1,), np.int32)}
    count = ctypes.c_int64(-1)
    rc = dzo.lib().dzo_pathway_batch_candidates(n, m, batch, dzo.F64 if dt == np.float64 else dzo.F32, dband.ptr, de.ptr, capacity,
                                                *[out[k][1].ptr for k in ("points", "tangents", "energies", "band_index", "image_index", "offsets")],
                                                ctypes.byref(count))
    assert np.array_equal(_bits(dband.to_host()), _bits(band)) and np.array_equal(_bits(de.to_host()), _bits(energies))   # neither is changed
    return rc, count.value, {k: w.to_host() for k, (_, w) in out.items()}, out


def _same(got, want, rows=None):
    for key in ("band_index", "image_index", "points", "energies", "tangents"):
        g, w = (got[key], want[key]) if rows is None else (got[key][:rows], want[key][:rows])
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", [1, 3, 300])
@pytest.mark.parametrize("n_images", [3, 4, 32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 257])
def test_candidates_bit_for_bit_against_the_twin(n, n_images, batch, dtype):
    """Every kind of profile (tests/pathway_twin.py: rising, falling, a peak at image 1 and at image M - 2, a plateau, an image
    equal to its left neighbour, alternating, a NaN, a valley), bands without a candidate between bands with some."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(1000 * n + 10 * n_images + batch)
    band = rng.normal(size=(batch, n_images, 3 * n)).astype(dt)
    energies, kinds = pw.profiles(batch, n_images, dt, seed=n_images)
    want = pw.candidates(band, energies, dt)
    assert want["count"] >= 1 and (batch < 3 or 0 in np.diff(want["offsets"])[1:-1])
    rc, count, got, buffers = _candidates(band, energies, n, want["count"])
    assert rc == 0 and count == want["count"]
    _guards_hold(buffers)
    assert np.array_equal(got["offsets"], want["offsets"])
    _same(got, want)
    # the Python wrapper: the same candidates from its own, larger arrays
    cand = dzo.band_candidates(dzo.DeviceArray.from_host(band), n, n_images, energies=dzo.DeviceArray.from_host(energies))
    assert cand.count == count and np.array_equal(cand.offsets, want["offsets"]) and cand.points.shape == (count, 3 * n)
    _same(dict(points=cand.points.to_host(), tangents=cand.tangents.to_host(), energies=cand.energies, band_index=cand.band_index,
               image_index=cand.image_index), want)
    # a band alone computes the bits it computes inside the batch
    if batch > 1:
        with_some = np.flatnonzero(np.diff(want["offsets"]) > 0)
        for b in sorted({int(with_some[0]), int(with_some[len(with_some) // 2]), int(with_some[-1])}):
            lo, hi = want["offsets"][b], want["offsets"][b + 1]
            rc1, count1, alone, _ = _candidates(band[b:b + 1], energies[b:b + 1], n, hi - lo)
            assert rc1 == 0 and count1 == hi - lo and alone["offsets"].tolist() == [0, hi - lo]
            for key in ("points", "tangents", "energies", "image_index"):
                assert np.array_equal(_bits(alone[key]), _bits(got[key][lo:hi])), (b, key)
    # one row too few: the documented code, the true count, complete offsets, the rows that fit, and nothing outside them
    rc, count, short, buffers = _candidates(band, energies, n, want["count"] - 1)
    assert rc == dzo.PATHWAY_OVERFLOW == 7 and count == want["count"]
    assert b"do not fit a capacity" in dzo.lib().dzo_last_error()
    _guards_hold(buffers, written=want["count"] > 1)
    assert np.array_equal(short["offsets"], want["offsets"])
    _same(short, want, rows=want["count"] - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [7, 64, 65])
def test_tangents_are_the_band_units(n, dtype):
    """Random bands (a jittered lattice, so that every energy is finite): one ``neb_apply`` on a copy, then the candidates of
    the original with ``neb_apply``'s energies.  Every candidate's tangent is the band unit's for that image, bit for bit."""
    dt = np.dtype(dtype)
    batch, m = 4, 9
    rng = np.random.default_rng(n)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    lattice = 1.12 * np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)[:n]
    band = (lattice.T.reshape(1, 1, 3 * n) + 0.08 * rng.normal(size=(batch, m, 3 * n))).astype(dt)
    original = dzo.DeviceArray.from_host(band)
    moved = original.copy()
    record = dzo.neb_apply(moved, dzo.DeviceArray.zeros(band.size, dt), n, m)
    assert np.isfinite(record["energies"]).all()
    cand = dzo.band_candidates(original, n, m, energies=dzo.DeviceArray.from_host(record["energies"]))
    assert cand.count >= batch and np.array_equal(_bits(original.to_host()), _bits(band))
    tangents = cand.tangents.to_host()
    for c, (b, i) in enumerate(zip(cand.band_index, cand.image_index)):
        assert np.array_equal(_bits(tangents[c]), _bits(record["tangents"][b, i])), (c, b, i)
    assert np.array_equal(_bits(cand.energies), _bits(record["energies"][cand.band_index, cand.image_index]))
    assert np.array_equal(_bits(cand.band_energies), _bits(record["energies"]))
    # the profile evaluated by the call itself: the energies of the band unit, so the same candidates
    own = dzo.band_candidates(original, n, m)
    assert np.array_equal(_bits(own.band_energies), _bits(record["energies"])) and np.array_equal(_bits(own.tangents.to_host()), _bits(tangents))


def test_arguments_are_checked():
    f = dzo.lib().dzo_pathway_batch_candidates
    band, e = dzo.DeviceArray.zeros(3 * 4 * 5 * 2), dzo.DeviceArray.zeros(5 * 2)
    pts, tan, ce = dzo.DeviceArray.zeros(3 * 4 * 4), dzo.DeviceArray.zeros(3 * 4 * 4), dzo.DeviceArray.zeros(4)
    bi, ii, off = (dzo.DeviceArray((8,), np.int32) for _ in range(3))
    count = ctypes.c_int64(-1)
    good = [4, 5, 2, dzo.F64, band.ptr, e.ptr, 4, pts.ptr, tan.ptr, ce.ptr, bi.ptr, ii.ptr, off.ptr, ctypes.byref(count)]
    assert f(*good) == 0 and count.value == 0                # a flat profile has no candidate
    assert off.to_host()[:3].tolist() == [0, 0, 0]

    def call(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        return f(*args)

    for changes in (dict(a0=0), dict(a1=2), dict(a1=33), dict(a2=0), dict(a3=9), dict(a4=None), dict(a5=None), dict(a6=-1), dict(a7=None),
                    dict(a8=None), dict(a9=None), dict(a10=None), dict(a11=None), dict(a12=None), dict(a13=None)):
        assert call(**changes) == 1, changes                 # DZO_ERR_INVALID
    assert call(a0=1025) == 5 and call(a2=dzo.PATHWAY_MAX_BATCH + 1) == 5            # DZO_ERR_UNSUPPORTED
    assert call(a4=np.zeros(band.size).ctypes.data) == 3                             # DZO_ERR_ASSERT: a host pointer
    # capacity 0 counts, and may leave the candidate arrays out
    assert call(a6=0, a7=None, a8=None, a9=None, a10=None, a11=None) == 0


# ------------------------------------------------------------------------------ the connect cycle, end to end
def _report(name, res):
    print("%s: %d of %d pairs connected; per cycle %s; %d minima, %d saddles in the database" % (
        name, int(res.connected.sum()), len(res.connected), [(c["bands"], c["candidates"], c["new_saddles"], c["connected"]) for c in res.cycles],
        res.graph.n_minima, res.graph.n_saddles))


@functools.lru_cache(maxsize=None)
def _lj7():
    minima = pc.lj7_minima(dzo)
    minima.setflags(write=False)
    return minima


def _lj7_pairs(dtype):
    minima = _lj7()
    first, second = zip(*[(i, j) for i in range(4) for j in range(i + 1, 4)])
    a = minima[list(first)].astype(dtype)
    b = pc.moved(minima[list(second)], np.random.default_rng(77)).astype(dtype)
    return first, second, a, b


def test_lj7_every_pair_is_connected_in_float64():
    n, displacement = 7, 0.02
    first, second, a, b = _lj7_pairs(np.float64)
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(b), n, 9, tol=1e-5, displacement=displacement,
                               band_iterations=600, max_cycles=3, align=dict(random_trials=25), quench_options=dict(max_steps=4000))
    _report("LJ7 float64", res)
    assert res.graph.n_minima >= 4 and res.pairs.tolist() == [[i, j] for i, j in zip(first, second)]   # every end classified onto its node
    assert np.abs(res.minimum_energies[:4] - np.array(pc.LJ7_MINIMA)).max() <= 1e-5
    assert res.connected.all(), res.connected                # a condition, not a tolerance
    checked = pc.check_pathways(dzo, res, n, displacement, 1e-5, known_saddles=pc.LJ7_SADDLES)
    assert checked >= 1
    assert [c["connected"] for c in res.cycles] == sorted(c["connected"] for c in res.cycles)
    assert np.all(res.barriers > 0) and np.all(res.cycles_used >= 1) and np.all(res.cycles_used <= 3)


def test_lj7_paths_are_valid_in_float32():
    """The fp32 settings of README.md: grad_tol = 3e-5, zero_tol = 1e-3.  Validity only; the count is printed."""
    n, displacement = 7, 0.02
    _, _, a, b = _lj7_pairs(np.float32)
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(b), n, 9, tol=1e-3, displacement=displacement,
                               band_iterations=600, max_cycles=3, grad_tol=3e-5, zero_tol=1e-3, align=dict(random_trials=25),
                               quench_options=dict(max_steps=4000))
    _report("LJ7 float32", res)
    assert res.minima.dtype == np.float32 and res.graph.n_minima >= 4
    pc.check_pathways(dzo, res, n, displacement, 1e-3, known_saddles=pc.LJ7_SADDLES)


@functools.lru_cache(maxsize=None)
def _lj13():
    minima = pc.lj13_minima(dzo, count=12)                   # ascending in energy, the icosahedron first
    minima.setflags(write=False)
    return minima


def test_lj13_paths_are_valid_and_the_database_is_shared():
    n, displacement = 13, 0.02
    minima = _lj13()[:5]
    first, second = zip(*pc.LJ13_PAIRS)
    a = minima[list(first)]
    b = pc.moved(minima[list(second)], np.random.default_rng(13))
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(b), n, 9, tol=1e-5, displacement=displacement,
                               band_iterations=600, max_cycles=4, quench_options=dict(max_steps=4000))
    _report("LJ13 float64", res)
    # two pairs that share an end share its node, in whatever frame and labelling the end came
    assert res.pairs.tolist() == [[i, j] for i, j in pc.LJ13_PAIRS]
    assert abs(res.minimum_energies[0] - pc.LJ13_ICOSAHEDRON) <= 1e-5
    pc.check_pathways(dzo, res, n, displacement, 1e-5)
    counts = [c["connected"] for c in res.cycles]
    assert counts == sorted(counts) and (not counts or counts[-1] == int(res.connected.sum()))
    assert len(res.cycles) <= 4 and np.all(res.cycles_used <= 4)


def test_lj13_distant_pairs_take_several_cycles():
    """The icosahedron against the eight highest of the twelve lowest minima, bands of five images: pairs several steps apart,
    which one cycle does not connect (measured: 5, 7 and 8 of 8 after one, two and three cycles).  What is checked is what the later cycles
    add to the first: the distances of the minima a cycle found, bands between intermediate minima, saddles found twice, and
    that every path reported at the end is a chain of real transition states."""
    n, displacement = 13, 0.02
    minima = _lj13()
    second = list(range(4, 12))
    a = np.repeat(minima[:1], len(second), axis=0)
    b = pc.moved(minima[second], np.random.default_rng(5))
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(b), n, 5, tol=1e-5, displacement=displacement,
                               band_iterations=600, max_cycles=4, quench_options=dict(max_steps=4000))
    _report("LJ13 float64, distant pairs", res)
    assert np.all(res.pairs[:, 0] == 0) and sorted(res.pairs[:, 1].tolist()) == list(range(1, 9))     # eight pairs share one node
    assert len(res.cycles) >= 2, "the case is meant to need more than one cycle"
    assert res.graph.n_minima > 9 and res.cycles[1]["bands"] >= 1                   # intermediate minima entered the database
    counts = [c["connected"] for c in res.cycles]
    assert counts == sorted(counts) and counts[-1] == int(res.connected.sum()) >= 1
    assert pc.check_pathways(dzo, res, n, displacement, 1e-5) >= 1
    # every band of a later cycle joins two database members that no saddle joined yet and that were tried at most twice
    assert all(res.graph.attempts(i, j) <= 2 for i in range(res.graph.n_minima) for j in range(i))
    assert np.all(res.cycles_used[res.connected] <= len(res.cycles)) and np.all(res.attempts_used >= 1)


def test_connect_saddles_descent_steps_follow_the_gradient_on_lj13():
    """``connect_saddles(descent_steps=...)``: the minima a saddle joins are the ones its two steepest-descent paths end in.
    The saddles are those a cycle over the distant LJ13 pairs collects (bands of nine images).  With the descent every end has
    the energy the numpy steepest descent lands on, within 1e-5; with ``descent_steps=0`` the call is the one there was before,
    bit for bit, and how many of its ends the L-BFGS quench alone takes elsewhere is printed (it was one, into the icosahedron,
    when the keyword was added), not asserted."""
    n, displacement = 13, 0.02
    minima = _lj13()
    a = np.repeat(minima[:1], 8, axis=0)
    res = dzo.connect_pathways(dzo.DeviceArray.from_host(a), dzo.DeviceArray.from_host(minima[4:12].copy()), n, 9, tol=1e-5, displacement=displacement,
                               band_iterations=600, max_cycles=4, quench_options=dict(max_steps=4000))
    saddles, modes = res.saddles.to_host().reshape(-1, 3 * n), res.saddle_modes.to_host().reshape(-1, 3 * n)
    k = len(saddles)
    assert k >= 8
    _, landed, g_left = pc.steepest_descent(np.concatenate([saddles + displacement * modes, saddles - displacement * modes]))
    assert g_left.max() <= 1e-5
    with_descent = dzo.connect_saddles(res.saddles, res.saddle_modes, n, displacement, 1e-5, max_steps=4000, descent_steps=2000)
    assert with_descent.end_stuck.all() and np.all(with_descent.edges >= 0)
    ends = with_descent.minimum_energies[with_descent.edges]                         # (k, 2): the + side, the - side
    assert np.abs(ends - np.stack([landed[:k], landed[k:]], axis=1)).max() <= 1e-5
    plain = dzo.connect_saddles(res.saddles, res.saddle_modes, n, displacement, 1e-5, max_steps=4000)
    zero = dzo.connect_saddles(res.saddles, res.saddle_modes, n, displacement, 1e-5, max_steps=4000, descent_steps=0)
    assert np.array_equal(_bits(plain.ends.to_host()), _bits(zero.ends.to_host())) and np.array_equal(plain.edges, zero.edges)
    ok = plain.edges >= 0
    elsewhere = np.abs(np.where(ok, plain.minimum_energies[np.where(ok, plain.edges, 0)], np.nan) - np.stack([landed[:k], landed[k:]], axis=1)) > 1e-5
    print("LJ13, %d saddles: the L-BFGS quench alone takes %d of %d ends to another minimum than steepest descent" % (k, int(elsewhere.sum()), 2 * k))
