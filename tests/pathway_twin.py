"""CPU twin of the transition-state candidates of many bands (csrc/dzo_pathway.hip; the rule is specified in include/dzo.h,
"Transition-state candidates of many bands"), in numpy.  A helper module for tests/test_pathway_twin.py (which checks it against
things it does not depend on) and tests/test_gpu_pathway.py (which checks the device against it).  Not a conftest, no fixtures.

The candidate rule is two plain comparisons in the element type; the tangent is ``neb_twin.tangent`` (item 2 of the band rule,
fp64 sums in the order of the sums of the device), so that a candidate's tangent carries the bits the band unit records; the
compaction is band-major with the image index ascending inside a band.  ``profiles`` builds the energy profiles the tests run
on: one of each kind the rule distinguishes, with exact ties where a kind needs them."""
import numpy as np

import neb_twin as nt

# in this order, so that a batch of one has a candidate and a batch of three a band without one between two that have some
KINDS = ("peak_first", "rising", "alternating", "falling", "peak_last", "plateau", "nan", "equal_left", "valley")


def is_candidate(e_prev, e, e_next):
    """Interior image: E_m > E_{m-1} and E_m >= E_{m+1}, so a plateau yields its first image and a NaN yields nothing."""
    return bool(e > e_prev) and bool(e >= e_next)


def candidate_images(energies):
    """The candidate images of one profile (M,), ascending; the ends are never candidates."""
    e = np.asarray(energies)
    return [m for m in range(1, len(e) - 1) if is_candidate(e[m - 1], e[m], e[m + 1])]


def candidates(band, energies, dtype):
    """The device's outputs for ``band`` (batch, M, 3N) and ``energies`` (batch, M): a dict of ``count``, ``offsets``
    (batch + 1, int32), ``band_index``, ``image_index`` (count, int32), ``points``, ``tangents`` (count, 3N) and ``energies``
    (count) in ``dtype``."""
    dt = np.dtype(dtype)
    x, e = np.asarray(band, dtype=dt), np.asarray(energies, dtype=dt)
    batch, M, n = x.shape
    offsets, bi, ii, pts, tan, en = [0], [], [], [], [], []
    for b in range(batch):
        for m in candidate_images(e[b]):
            bi.append(b)
            ii.append(m)
            pts.append(x[b, m])
            en.append(e[b, m])
            tan.append(nt.tangent(x[b, m - 1], x[b, m], x[b, m + 1], e[b, m - 1], e[b, m], e[b, m + 1], dt)[0])
        offsets.append(len(bi))
    return dict(count=len(bi), offsets=np.array(offsets, dtype=np.int32), band_index=np.array(bi, dtype=np.int32),
                image_index=np.array(ii, dtype=np.int32), points=np.array(pts, dtype=dt).reshape(len(bi), n),
                tangents=np.array(tan, dtype=dt).reshape(len(bi), n), energies=np.array(en, dtype=dt))


def levels(kind, M):
    """The profile of ``kind`` as integer levels (M,), -1 marking a NaN: equal levels become equal energies."""
    m = np.arange(M)
    mid = max(1, (M - 2) // 2)
    if kind == "rising":
        return m.copy()
    if kind == "falling":
        return m[::-1].copy()
    if kind == "peak_first":
        return M - np.abs(m - 1)
    if kind == "peak_last":
        return M - np.abs(m - (M - 2))
    if kind == "plateau":                                    # E_mid == E_{mid+1}: the first image only
        lv = M - np.abs(m - mid)
        lv[mid + 1] = lv[mid]
        return lv
    if kind == "equal_left":                                 # E_mid == E_{mid-1}: image mid is no candidate
        lv = M - np.abs(m - mid)
        lv[mid - 1] = lv[mid]
        return lv
    if kind == "alternating":                                # the most a band can hold: every odd interior image
        return 1 + (m % 2) * (1 + m)
    if kind == "nan":                                        # a peak with a NaN next to it, and one that is the NaN
        lv = M - np.abs(m - mid)
        lv[mid + 1 if M > 3 else mid] = -1
        return lv
    if kind == "valley":
        return np.abs(m - mid) + 1
    raise ValueError(kind)


def profiles(batch, M, dtype, seed):
    """(energies (batch, M) in ``dtype``, kinds): band b has the profile KINDS[b % len(KINDS)] on a random increasing table of
    energies of its own, so that bands without a candidate lie between bands that have some."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    e = np.empty((batch, M), dtype=dt)
    kinds = []
    for b in range(batch):
        kind = KINDS[b % len(KINDS)]
        lv = levels(kind, M)
        table = np.sort(rng.normal(scale=3.0, size=2 * M + 4)).astype(dt)
        assert len(np.unique(table)) == len(table)
        e[b] = np.where(lv < 0, dt.type(np.nan), table[np.maximum(lv, 0)])
        kinds.append(kind)
    return e, kinds
