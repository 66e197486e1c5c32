"""The L1 vector primitives on the device (csrc/dzo_vec.hip) against their CPU twin (tests/vec_twin.py), bit for bit.

Sizes: vec_twin.sizes() -- 1, 2, 3, N +- 1, 64 N +- 1, 256 N +- 1, 1024 N - 1 .. 1024 N + N + 1, 2 * 1024 N + 1 and the first
size at which the grid-stride loop makes a second trip on this device (N = 2 fp64 / 4 fp32 elements per 16-byte vector).
Alignment: every operand is a view into an allocation with GUARD canary elements on both sides, at an element offset of
0 .. N - 1 from the 16-byte grid, independently per operand (vec_twin.alignments()); after every call the canaries are
intact and the read-only operands kept their bytes.  At the second-trip size: all aligned and one mixed combination.

1. elementwise: axpy_, axpby_, rmul_, scale_ (in place, out of place, dst aliasing x), trial_point_, fill_, negate_, copy_;
2. special values at vec_twin.positions(n);
3. reductions: dot, norm, norm2, inv_norm equal the twin's ordered sum, twice; a NaN / inf at every position reaches the result;
4. isequal: one differing element at every position, at every alignment.
"""
import functools
import math

import numpy as np
import pytest

import vec_twin as vt
from dzo_loader import dzo
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
CANARY = 12345.0
GUARD = 64
ALPHA, BETA = 0.37, -1.7


@functools.lru_cache(maxsize=None)
def _cus():
    return dzo.device_info()["compute_units"]


def _cases():
    """(dtype, index into sizes()): the last size depends on the device's grid cap, so it is looked up at run time."""
    out = []
    for d in DTYPES:
        names = ["n%d" % n for n in vt.sizes(d, second_trip=False)] + ["second_trip"]
        out += [pytest.param(d, i, id="%s-%s" % (d, name)) for i, name in enumerate(names)]
    return out


def _size(dtype, i):
    return vt.sizes(dtype, _cus())[i]


def _is_second_trip(dtype, n):
    return n == vt.second_trip_size(dtype, _cus())


def _alignments(dtype, n, operands):
    return vt.alignments(dtype, operands, full=not _is_second_trip(dtype, n))


class Guarded:
    """A host vector uploaded into the middle of a canary-filled allocation, `off` elements off the 16-byte grid."""

    def __init__(self, host, off):
        self.host = np.array(host, copy=True)
        self.n, self.lo = self.host.size, GUARD + off
        full = np.full(self.lo + self.n + GUARD, CANARY, dtype=self.host.dtype)
        full[self.lo:self.lo + self.n] = self.host
        self.buf = dzo.DeviceArray.from_host(full)
        assert self.buf.ptr % 16 == 0
        self.dev = self.buf.view(self.lo, self.n)

    def upload(self, host):
        """Replace the payload."""
        self.host = np.array(host, copy=True)
        self.dev.upload(self.host)

    def poke(self, p, value):
        """Change element p alone, on the device and in the host copy."""
        self.host[p] = value
        self.buf.view(self.lo + p, 1).upload(self.host[p:p + 1])

    def read(self):
        """The payload, after checking that nothing around it was written."""
        h = self.buf.to_host()
        c = h.dtype.type(CANARY)
        assert np.all(h[:self.lo] == c) and np.all(h[self.lo + self.n:] == c), "wrote outside the operand"
        return h[self.lo:self.lo + self.n]

    def unchanged(self):
        got = self.read()
        assert np.array_equal(vt.bits(got), vt.bits(self.host)), "a read-only operand was modified"


def _data(n, dtype, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(dtype) for _ in range(3)]


def _check(out, want, what):
    got = out.read()
    assert vt.same(got, want), (what, np.flatnonzero(~((vt.bits(got) == vt.bits(want)) | (np.isnan(got) & np.isnan(want))))[:5])


def _elementwise_wants(x, y, dtype):
    """The twin's results for _run_elementwise, computed once for all alignments."""
    return {"axpy": vt.axpy(ALPHA, x, y), "axpby": vt.axpby(ALPHA, x, BETA, y), "rmul": vt.scal(ALPHA, y), "scale_y": vt.scal(BETA, y),
            "scale_x": vt.scal(BETA, x), "trial_point": vt.trial_point(ALPHA, x, y), "fill": vt.fill(x.size, 0.1, dtype),
            "negate": vt.negate(y), "copy": vt.copy(x)}


def _run_elementwise(x, y, d, want, offs3):
    """Every elementwise primitive on the given host operands, each at its own alignment; results against the twin."""
    ox, oy, od = offs3
    tag = (x.dtype.name, x.size, offs3)
    X, Y = Guarded(x, ox), Guarded(y, oy)
    dzo.axpy_(ALPHA, X.dev, Y.dev)
    _check(Y, want["axpy"], ("axpy",) + tag)
    Y.upload(y)
    dzo.axpby_(ALPHA, X.dev, BETA, Y.dev)
    _check(Y, want["axpby"], ("axpby",) + tag)
    Y.upload(y)
    dzo.rmul_(Y.dev, ALPHA)
    _check(Y, want["rmul"], ("rmul",) + tag)
    Y.upload(y)
    dzo.scale_(Y.dev, BETA)
    _check(Y, want["scale_y"], ("scale in place",) + tag)
    Y.upload(y)
    dzo.scale_(Y.dev, BETA, Y.dev)
    _check(Y, want["scale_y"], ("scale dst is x",) + tag)
    Y.upload(y)
    dzo.negate_(Y.dev)
    _check(Y, want["negate"], ("negate",) + tag)
    Y.upload(y)
    D = Guarded(d, od)
    dzo.scale_(D.dev, BETA, X.dev)
    _check(D, want["scale_x"], ("scale out of place",) + tag)
    D.upload(d)
    dzo.trial_point_(D.dev, ALPHA, X.dev, Y.dev)                # dst = fma(t, d = X, x = Y)
    _check(D, want["trial_point"], ("trial_point",) + tag)
    Y.unchanged()
    D.upload(d)
    dzo.fill_(D.dev, 0.1)
    _check(D, want["fill"], ("fill",) + tag)
    D.upload(d)
    dzo.copy_(D.dev, X.dev)
    _check(D, want["copy"], ("copy",) + tag)
    X.unchanged()


# ------------------------------------------------------------------------------ 1. elementwise
@pytest.mark.parametrize("dtype,i", _cases())
def test_elementwise_bit_for_bit(dtype, i):
    n = _size(dtype, i)
    x, y, d = _data(n, dtype, 11 * n + 1)
    want = _elementwise_wants(x, y, dtype)
    for offs in _alignments(dtype, n, 3):
        _run_elementwise(x, y, d, want, offs)


# ------------------------------------------------------------------------------ 2. special values
def _specials(dtype):
    tiny = np.finfo(dtype).smallest_subnormal
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny], dtype=dtype)


@pytest.mark.parametrize("dtype,i", _cases())
def test_special_values_at_the_seams(dtype, i):
    """NaN, +-inf, +-0 and a subnormal at every position of positions(n), in x, in y and in both (rotated, so that every
    position sees every value).  The multipliers are powers of two, so every product is exact and the twin's results are
    those of one rounding also outside the normal range."""
    n = _size(dtype, i)
    dt = np.dtype(dtype)
    pos = vt.positions(n, dt, _cus())
    sp = _specials(dt)
    offs_list = _alignments(dtype, n, 2)[:2] if _is_second_trip(dtype, n) else [(0, 0), (1, 1), (1, 0)]
    for rot in range(len(sp) if not _is_second_trip(dtype, n) else 1):
        x, y, _ = _data(n, dtype, 13 * n + rot)
        for k, p in enumerate(pos):
            x[p] = sp[(k + rot) % len(sp)]
            if (k + rot) % 3:
                y[p] = sp[(2 * k + rot + 1) % len(sp)]
        want = {"axpy": vt.axpy(2.0, x, y), "axpby": vt.axpby(-2.0, x, 2.0, y), "xmx": vt.trial_point(-1.0, x, x),
                "negate": vt.negate(x), "scale": vt.scal(2.0, x)}
        fin = ~np.isnan(x)
        assert np.array_equal(np.isnan(want["xmx"]), ~np.isfinite(x))
        for ox, oy in offs_list:
            X, Y = Guarded(x, ox), Guarded(y, oy)
            dzo.axpy_(2.0, X.dev, Y.dev)
            _check(Y, want["axpy"], ("axpy", n, rot, ox, oy))
            Y.upload(y)
            dzo.axpby_(-2.0, X.dev, 2.0, Y.dev)
            _check(Y, want["axpby"], ("axpby", n, rot, ox, oy))
            dzo.trial_point_(Y.dev, -1.0, X.dev, X.dev)         # x - x: +0, and NaN where x is not finite
            _check(Y, want["xmx"], ("trial_point", n, rot, ox, oy))
            X.unchanged()
            # negate!: the sign bit flips on zeros and infinities too
            dzo.negate_(X.dev)
            neg = X.read()
            assert np.array_equal(np.signbit(neg[fin]), ~np.signbit(x[fin])) and np.array_equal(np.abs(neg[fin]), np.abs(x[fin]))
            assert np.all(np.isnan(neg[~fin])) and vt.same(neg, want["negate"]), ("negate", n, rot, ox)
            X.upload(x)
            dzo.scale_(X.dev, 2.0)
            _check(X, want["scale"], ("scale", n, rot, ox))
    # axpby!(a, x, 0, y) forms 0 * y: a NaN in y is a NaN in the result, at every position alone
    x, y, _ = _data(n, dtype, 17 * n)
    base = vt.axpby(ALPHA, x, 0.0, y)
    assert not np.isnan(base).any()
    for ox, oy in offs_list[:2]:
        X, Y = Guarded(x, ox), Guarded(y, oy)
        for p in pos:
            Y.upload(y)
            Y.poke(p, np.nan)
            want = base.copy(); want[p] = np.nan
            dzo.axpby_(ALPHA, X.dev, 0.0, Y.dev)
            assert vt.same(Y.read(), want), (p, ox, oy)
        X.unchanged()
    # fill! converts its double argument: (T)value
    for value in (0.1, 1e300, -1e300, 1e-300, -0.0, math.nan, 16777217.0):
        D = Guarded(y, 1)
        dzo.fill_(D.dev, value)
        got = D.read()
        with np.errstate(all="ignore"):
            want = dt.type(value)
        assert vt.same(got, np.full(n, want, dt)), value
        if dt == np.float32 and value in (1e300, 1e-300, 16777217.0):
            assert got[0] == {1e300: np.inf, 1e-300: 0.0, 16777217.0: 16777216.0}[value]


# ------------------------------------------------------------------------------ 3. reductions
def _assert_sum(got, want, what, bound):
    if np.float64(got).view(np.int64) != np.float64(want).view(np.int64):
        limit, k = bound()
        raise AssertionError("%s: device %r, twin %r, difference %.3e; the derived bound gamma_%d sum|x_i y_i| is %.3e -- %s"
                             % (what, got, want, abs(got - want), k, limit,
                                "within it: another ORDER of the same terms" if abs(got - want) <= limit else "beyond it: terms were LOST"))


@pytest.mark.parametrize("dtype,i", _cases())
def test_reductions_bit_for_bit(dtype, i):
    n = _size(dtype, i)
    cus = _cus()
    x, y, _ = _data(n, dtype, 19 * n + 3)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    scale_xy, scale_xx = float(np.abs(xd * yd).sum()), float((xd * xd).sum())
    twin_xy, twin_xx = {}, {}                                  # by instantiation: the twin's sum is computed once for each
    for ox, oy in _alignments(dtype, n, 2):
        vec_xy, vec_xx = ox == 0 and oy == 0, ox == 0
        if vec_xy not in twin_xy:
            twin_xy[vec_xy] = vt.dot(x, y, cus, vec_xy)
        if vec_xx not in twin_xx:
            twin_xx[vec_xx] = vt.dot(x, x, cus, vec_xx)
        ss = twin_xx[vec_xx]
        bound_xy = lambda: vt.dot_bound(n, dtype, cus, vec_xy, scale_xy)
        bound_xx = lambda: vt.dot_bound(n, dtype, cus, vec_xx, scale_xx)
        X, Y = Guarded(x, ox), Guarded(y, oy)
        for call in range(2):                                   # deterministic: the same bits on a second call
            _assert_sum(dzo.dot(X.dev, Y.dev), twin_xy[vec_xy], ("dot", dtype, n, ox, oy, call), bound_xy)
            _assert_sum(dzo.norm2(X.dev), _round(ss, dtype), ("norm2", dtype, n, ox, call), bound_xx)
            _assert_sum(dzo.norm(X.dev), _norm(ss, dtype), ("norm", dtype, n, ox, call), bound_xx)
            _assert_sum(dzo.inv_norm(X.dev), _inv_norm(ss, dtype), ("inv_norm", dtype, n, ox, call), bound_xx)
        X.unchanged(); Y.unchanged()


def _round(ss, dtype):
    return float(np.float32(ss)) if np.dtype(dtype) == np.float32 else ss


def _norm(ss, dtype):
    return float(np.sqrt(np.float32(ss))) if np.dtype(dtype) == np.float32 else float(np.sqrt(np.float64(ss)))


def _inv_norm(ss, dtype):
    T = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    return float(T(1.0) / np.sqrt(T(ss)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_twins_roundings_are_the_ones_used_above(dtype):
    x = np.random.default_rng(2).standard_normal(1001).astype(dtype)
    ss = vt.dot(x, x, _cus())
    assert vt.norm2(x, _cus()) == _round(ss, dtype) and vt.norm(x, _cus()) == _norm(ss, dtype) and vt.inv_norm(x, _cus()) == _inv_norm(ss, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_reductions(dtype):
    e = dzo.DeviceArray(0, dtype)
    assert dzo.dot(e, e) == 0.0 and not np.signbit(dzo.dot(e, e))
    assert dzo.norm(e) == 0.0 and dzo.norm2(e) == 0.0 and dzo.inv_norm(e) == np.inf
    assert dzo.isequal(e, e)


@pytest.mark.parametrize("dtype,i", _cases())
def test_a_nan_or_inf_anywhere_reaches_the_sum(dtype, i):
    n = _size(dtype, i)
    dt = np.dtype(dtype)
    x, y, _ = _data(n, dtype, 23 * n + 5)
    y[y == 0] = 1.0
    for ox, oy in _alignments(dtype, n, 2)[:2]:
        X, Y = Guarded(x, ox), Guarded(y, oy)
        for p in vt.positions(n, dt, _cus()):
            keep = x[p]
            X.poke(p, np.nan)
            assert math.isnan(dzo.dot(X.dev, Y.dev)) and math.isnan(dzo.dot(Y.dev, X.dev)), (p, ox, oy)
            assert math.isnan(dzo.norm(X.dev)) and math.isnan(dzo.norm2(X.dev)) and math.isnan(dzo.inv_norm(X.dev)), (p, ox)
            X.poke(p, np.inf)
            assert dzo.dot(X.dev, Y.dev) == math.copysign(math.inf, y[p]), (p, ox, oy)
            assert dzo.norm(X.dev) == math.inf and dzo.norm2(X.dev) == math.inf and dzo.inv_norm(X.dev) == 0.0, (p, ox)
            X.poke(p, keep)
        X.unchanged(); Y.unchanged()


# ------------------------------------------------------------------------------ 4. isequal
@pytest.mark.parametrize("dtype,i", _cases())
def test_isequal_sees_one_element_anywhere(dtype, i):
    n = _size(dtype, i)
    dt = np.dtype(dtype)
    a, _, _ = _data(n, dtype, 29 * n + 7)
    for oa, ob in _alignments(dtype, n, 2):
        A, B = Guarded(a, oa), Guarded(a, ob)
        assert dzo.isequal(A.dev, B.dev) and dzo.isequal(B.dev, A.dev) and orc.isequal(A.host, B.host)
        for p in vt.positions(n, dt, _cus()):
            keep = a[p]
            # one ulp
            B.poke(p, np.nextafter(keep, dt.type(np.inf)))
            assert not dzo.isequal(A.dev, B.dev) and not dzo.isequal(B.dev, A.dev), ("ulp", p, oa, ob)
            assert not orc.isequal(A.host, B.host)
            # +0 against -0
            A.poke(p, 0.0); B.poke(p, -0.0)
            assert not dzo.isequal(A.dev, B.dev) and not orc.isequal(A.host, B.host), ("zero", p, oa, ob)
            # a NaN equals a NaN of another sign and payload
            A.poke(p, np.nan); B.poke(p, vt.other_nan(dt))
            assert vt.bits(A.host)[p] != vt.bits(B.host)[p]
            assert dzo.isequal(A.dev, B.dev) and orc.isequal(A.host, B.host), ("nan", p, oa, ob)
            A.poke(p, keep); B.poke(p, keep)
            assert dzo.isequal(A.dev, B.dev), ("restored", p, oa, ob)
        A.unchanged(); B.unchanged()
