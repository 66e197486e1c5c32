"""csrc/dzo_phi_search.h on the CPU: the state machine that both drivers of the dense BFGS step's line searches run (the host-driven
bfgs_dual_search and the device-driven finish_phi6_advance_kernel), with its speculative requests, against the oracle's sequential
search.  tools/phi_search_table.cpp, built with -Wall -Werror and the address and undefined-behaviour sanitizers and run as a process
of its own, drives the machine the way the drivers do (begin; post, evaluate every active slot, consume; until it stops asking) on
small objectives; the oracle runs the same searches over a Python callback that evaluates the same objectives in numpy, bit for bit.
The grid is required to take every exit of the search in both dtypes, to use speculative values and to drop them.

The tool's second mode runs the header's own sequential loop (phi_sequential_run: what bfgs_sequential_search of dzo_bfgs.hip runs
over its evaluator) over an evaluator of the same objectives with an optional constraint.  There
nothing is parked: for every query, the tiny-step path and infeasible points included, the result, the evaluation count and the
evaluated points are the oracle's."""
import collections
import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "phi_search_table.cpp")
DTYPES = [np.float32, np.float64]
FIRST, DOUBLING, SHRINKING, QUADRATIC, DONE, SEQUENTIAL = range(6)         # dzo_phi_search.h
EXITS = ["f0 not finite", "t0 not a step", "zero direction", "tiny step", "doubling: fb > fa", "doubling: max_increases",
         "doubling: not finite", "doubling: stagnation", "halving: found", "halving: to zero", "quadratic: accepted",
         "quadratic: rejected", "quadratic: skipped"]
# the sequential driver parks nothing: it takes the tiny-step path (:91-101, :107-123) itself, and serves constraints
SEQUENTIAL_EXITS = [name for name in EXITS if name != "tiny step"] + [
    "tiny: moved on", "tiny: step overflows", "tiny: infeasible", "tiny: clamped back to x", "infeasible trial"]
NO_CONSTRAINT, CLAMP, REFUSE = range(3)                                     # tools/phi_search_table.cpp's cons


def objective(kind, c, m, p):
    """kind 0: sum c_i d_i; 1: sum c_i (d_i d_i); 2: sum c_i ((d_i d_i) (d_i d_i)); d_i = p_i - m_i.  Every operation rounded to the
    dtype, summed in index order: what the driver computes."""
    acc = p.dtype.type(0)
    with np.errstate(all="ignore"):
        for ci, mi, pi in zip(c, m, p):
            w = pi - mi
            if kind >= 1:
                w = w * w
            if kind == 2:
                w = w * w
            acc = acc + ci * w
    return acc


def fma(a, b, c):
    """fma(a, b, c) of three finite numpy scalars of one dtype, correctly rounded: exact in rationals, then the nearest of the
    candidate and its two neighbours, ties to the even significand."""
    dt = type(c)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = dt(float(exact))
    uint = np.uint32 if dt is np.float32 else np.uint64
    cands = [v for v in (near, np.nextafter(near, dt(-np.inf)), np.nextafter(near, dt(np.inf))) if np.isfinite(v)]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(uint)) & 1))


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


class CallbackBFGS(orc.BFGS):
    """orc.BFGS over a Python objective (orc_bfgs_create: the constructor that orc_bfgs_create_problem forwards to).  The callback
    records every point it is given.  constrained: with a constraint callback that serves the query's `cons` (kind, lo, hi) -- CLAMP
    projects onto the box, REFUSE calls every point outside it infeasible."""

    def __init__(self, dtype, n, constrained=False):
        self.dtype, self.n, self.suf = np.dtype(dtype), n, "_f64" if dtype is np.float64 else "_f32"
        ct = C.c_double if dtype is np.float64 else C.c_float
        self.points, self.query = [], None

        def of(_ctx, xp, nn):
            p = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
            self.points.append(p)
            return 0.0 if self.query is None else float(objective(self.query["kind"], self.query["c"], self.query["m"], p))

        def gf(_ctx, gp, _xp, nn):
            np.ctypeslib.as_array(gp, shape=(nn,))[:] = 1

        def cf(_ctx, xp, nn):
            kind, lo, hi = (NO_CONSTRAINT, 0, 0) if self.query is None else self.query["cons"]
            p = np.ctypeslib.as_array(xp, shape=(nn,))
            if kind == CLAMP:
                p[:] = np.clip(p, lo, hi)
            return int(kind != REFUSE or bool(np.all((p >= lo) & (p <= hi))))

        self._of = C.CFUNCTYPE(ct, C.c_void_p, C.POINTER(ct), C.c_int64)(of)
        self._cf = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(ct), C.c_int64)(cf)
        self._gf = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(ct), C.POINTER(ct), C.c_int64)(gf)
        create = getattr(orc.lib(), "orc_bfgs_create" + self.suf)
        create.restype = C.c_void_p
        create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_int64]
        x0 = np.zeros(n, dtype=dtype)
        self.h = create(C.cast(self._of, C.c_void_p), C.cast(self._gf, C.c_void_p),
                        C.cast(self._cf, C.c_void_p) if constrained else None, None, x0.ctypes.data_as(C.c_void_p), 1.0, n)
        assert self.h

    def search(self, q, f0):
        """(t_best, f_best, evaluations, the points evaluated) of the query's search.  The oracle's trial point is x - t d (:945):
        d = -sign * dir gives fma(sign * t, dir, x) exactly."""
        self.query = q
        self.current_point[:] = q["x"]
        self.next_step_direction[:] = -q["dir"] if q["sign"] > 0 else q["dir"]
        L = orc.lib()
        getattr(L, "orc_bfgs_set_s" + self.suf)(self.h, 0, float(f0))
        getattr(L, "orc_bfgs_set_i" + self.suf)(self.h, 4, 0)
        self.set_max_increases(q["max_increases"])
        self.points = []
        t, f = self.line_search(False, float(q["t0"]))
        return t, f, self.objective_evaluations, self.points


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("phi") / "phi_search_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])

    def ask(queries, sequential=False):
        path = exe + ".queries"
        with open(path, "w") as f:
            for q in queries:
                reals = [float(v).hex() for name in ("x", "dir", "c", "m") for v in q[name]]
                f0 = q["f0"]
                f.write("%d %d %d %s %d %s %s %d %s %d %s %s\n" % (
                    0 if q["dtype"] is np.float32 else 1, q["kind"], len(q["x"]), " ".join(reals), f0 is not None,
                    float(0.0 if f0 is None else f0).hex(), float(q["t0"]).hex(), q["max_increases"], float(q["sign"]).hex(),
                    q["cons"][0], float(q["cons"][1]).hex(), float(q["cons"][2]).hex()))
        out = subprocess.run([exe] + ["--sequential"] * sequential + [path], capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(queries)
        answers = []
        for q, ln in zip(queries, lines):
            w, n = ln.split(), len(q["x"])
            if sequential:
                a = dict(zip(("state", "increases", "quadratic_asked", "evals", "unchanged", "infeasible", "at_x", "compared"), map(int, w[:8])))
                a.update(zip(("t_best", "f_best", "f0", "x1", "f1", "x2", "f2", "last_f"), (int(v, 16) for v in w[8:16])))
                rest = w[16:]
                assert len(rest) == a["evals"] * (2 + n)
                a["consumed"] = [dict(t=int(r[0], 16), f=int(r[1], 16), point=[int(v, 16) for v in r[2:]])
                                 for r in (rest[i:i + 2 + n] for i in range(0, len(rest), 2 + n))]
                answers.append(a)
                continue
            a = dict(zip(("state", "increases", "quadratic_asked", "evals", "rounds", "posted", "grad_index"), map(int, w[:7])))
            a.update(zip(("t_best", "f_best", "f0", "x1", "f1", "x2", "f2"), (int(v, 16) for v in w[7:14])))
            rest = w[15:]
            assert len(rest) == int(w[14]) * (4 + n)
            a["consumed"] = [dict(round=int(r[0]), slot=int(r[1]), t=int(r[2], 16), f=int(r[3], 16), point=[int(v, 16) for v in r[4:]])
                             for r in (rest[i:i + 4 + n] for i in range(0, len(rest), 4 + n))]
            answers.append(a)
        return answers
    return ask


def query(dtype, kind, x, dir, c, m, t0, f0=None, max_increases=0, sign=-1.0, cons=(NO_CONSTRAINT, 0.0, 0.0)):
    arr = lambda v: np.asarray(v, dtype=dtype).reshape(-1)                  # noqa: E731
    return dict(dtype=dtype, kind=kind, x=arr(x), dir=arr(dir), c=arr(c), m=arr(m), t0=dtype(t0), f0=None if f0 is None else dtype(f0),
                max_increases=max_increases, sign=sign, cons=(cons[0], dtype(cons[1]), dtype(cons[2])))


def queries_of(dtype):
    eps, tiny = np.finfo(dtype).eps, np.finfo(dtype).tiny
    big = dtype(1e19 if dtype is np.float32 else 1e154)                     # big^2 is finite, (2 big)^2 is not
    bowl = dict(kind=1, x=[1.0], dir=[1.0], c=[1.0], m=[0.0])               # f(t) = (1 - t)^2 along x - t dir
    qs = []
    for f0 in (np.inf, -np.inf, np.nan):                                    # :64-66
        qs.append(query(dtype, t0=0.5, f0=f0, **bowl))
    for t0 in (0.0, -1.0, np.inf, np.nan):
        qs.append(query(dtype, t0=t0, **bowl))
    for z in (0.0, -0.0):                                                   # :83-85
        qs.append(query(dtype, 1, [1.0, 2.0], [z, z], [1.0, 1.0], [0.0, 0.0], t0=0.5))
    for sign in (-1.0, 1.0):                                                # :91-101: the first trial point is x itself
        qs.append(query(dtype, t0=eps / 8, sign=sign, **bowl))
        qs.append(query(dtype, 1, [1.0, -3.0, 2.0], [1.0, 0.0, -0.5], [1.0, 2.0, 0.5], [0.0, 0.0, 0.0], t0=eps / 16, sign=sign))
        qs.append(query(dtype, 2, [4.0, 4.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0], t0=tiny, sign=sign))
    for t0 in (2.0 ** -6, 0.1, 0.3, 1.0):                                   # doubling past the minimum: fb > fa
        qs.append(query(dtype, t0=t0, **bowl))
    for inc in (1, 2, 5):                                                   # ... stopped by max_increases first
        qs.append(query(dtype, t0=2.0 ** -8, max_increases=inc, **bowl))
        qs.append(query(dtype, 0, [0.0], [1.0], [-1.0], [0.0], t0=1.0, max_increases=inc, sign=1.0))
    qs.append(query(dtype, 1, [0.0], [big], [-1.0], [0.0], t0=1.0))          # ... by an overflow: f = -(t big)^2 -> -inf
    qs.append(query(dtype, 0, [0.0], [1.0], [-1.0], [0.0], t0=1.0, sign=1.0))    # f = -t, doubled until t itself overflows
    qs.append(query(dtype, 1, [1.0], [1.0], [1.0], [2.0], t0=dtype(0.6) * eps, sign=1.0))   # :150: 1 + 0.6 eps and 1 + 1.2 eps are one point
    qs.append(query(dtype, 1, [1.0, 0.5], [1.0, 0.0], [1.0, 1.0], [2.0, 0.0], t0=dtype(0.7) * eps, sign=1.0))
    for t0 in (3.0, 4.0, 64.0, 2.0 ** 20):                                  # halving back under f0
        qs.append(query(dtype, t0=t0, **bowl))
        qs.append(query(dtype, 2, [1.0, -1.0], [1.0, -1.0], [1.0, 0.5], [0.0, 0.0], t0=t0))
    for t0 in (tiny, tiny * 8, 1.0):                                        # ... never: every value is above the f0 given, down to hs == 0
        qs.append(query(dtype, 1, [0.0], [1.0], [1.0], [0.0], t0=t0, f0=-1.0))
    qs.append(query(dtype, t0=1.0, **bowl))                                 # bracket (1, 0, 2, 1): the parabola's minimum is x1 again, rejected
    qs.append(query(dtype, 1, [1.0], [1.0], [0.0], [0.0], t0=0.5, max_increases=2))      # a constant: d1 = d2 = 0, no quadratic point
    qs.append(query(dtype, 1, [1.0], [1.0], [0.0], [0.0], t0=0.5))          # ... doubled until the point overflows and f is NaN
    rng = np.random.default_rng(7)
    for kind in (0, 1, 2):
        for n in (1, 2, 3):
            for _ in range(40):
                c = rng.uniform(0.1, 2.0, n) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
                qs.append(query(dtype, kind, rng.uniform(-2, 2, n), rng.uniform(-2, 2, n) * rng.choice([1.0, 1.0, 0.0], n), c,
                                rng.uniform(-2, 2, n), t0=2.0 ** rng.uniform(-12, 6), max_increases=int(rng.choice([0, 0, 1, 3, 6])),
                                sign=float(rng.choice([-1.0, 1.0])), f0=rng.choice([None, None, None, -5.0, 5.0])))
    return qs


def exits_of(q, a, f0):
    """Which exits of the search the machine took, from what it was given and where it ended."""
    val = lambda name: struct.unpack("<d", struct.pack("<Q", a[name]))[0]   # noqa: E731
    if not np.isfinite(f0):
        return ["f0 not finite"]
    if not (q["t0"] > 0) or not np.isfinite(q["t0"]):
        return ["t0 not a step"]
    if not np.any(q["dir"] != 0):
        return ["zero direction"]
    if a["state"] == SEQUENTIAL:
        return ["tiny step"]
    f1, f2 = val("f1"), val("f2")
    if a["increases"] > 0:                                                  # the order of the tests of :147-150
        if q["max_increases"] > 0 and a["increases"] >= q["max_increases"]:
            out = ["doubling: max_increases"]
        elif not np.isfinite(f2):
            out = ["doubling: not finite"]
        elif f2 > f1:
            out = ["doubling: fb > fa"]
        else:
            out = ["doubling: stagnation"]
    else:
        out = ["halving: to zero" if val("x1") == 0 and val("x2") == 0 else "halving: found"]
    if not a["quadratic_asked"]:
        return out + ["quadratic: skipped"]
    fb = float(f0)
    fb = f1 if f1 < fb else fb
    fb = f2 if f2 < fb else fb
    fq = val("last_f") if "last_f" in a else struct.unpack("<d", struct.pack("<Q", a["consumed"][-1]["f"]))[0]
    return out + ["quadratic: accepted" if fq < fb else "quadratic: rejected"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_machine_searches_as_the_oracle_does_and_the_grid_takes_every_exit(driver, dtype):
    qs = queries_of(dtype)
    answers = driver(qs)
    oracles = {n: CallbackBFGS(dtype, n) for n in (1, 2, 3)}
    taken = collections.Counter()
    spec_used = collections.Counter()
    dropped_later = 0
    for i, (q, a) in enumerate(zip(qs, answers)):
        x, n = q["x"], len(q["x"])
        f0 = objective(q["kind"], q["c"], q["m"], x) if q["f0"] is None else q["f0"]
        assert a["f0"] == bits(f0), i                                       # the driver's objective is numpy's
        t, f, evals, points = oracles[n].search(q, f0)
        startable = np.isfinite(f0) and q["t0"] > 0 and np.isfinite(q["t0"]) and np.any(q["dir"] != 0)
        stays = startable and all(fma(dtype(q["sign"]) * q["t0"], d, xi) == xi for d, xi in zip(q["dir"], x))
        assert (a["state"] == SEQUENTIAL) == bool(stays), i
        if a["state"] == SEQUENTIAL:
            # nothing counted; and the oracle took its :91-101 loop: it never evaluated the first trial point, which is x --
            # it went on doubling, and what it evaluated first (if the step stayed finite) is a later doubling's point
            assert a["evals"] == 0 and a["consumed"] == [] and a["grad_index"] == -1, i
            assert not points or not np.array_equal(points[0], x), i
            if points:
                step, first = q["t0"], None
                with np.errstate(all="ignore"):
                    while first is None or np.array_equal(first, x):
                        step = step + step
                        first = np.array([fma(dtype(q["sign"]) * step, d, xi) for d, xi in zip(q["dir"], x)])
                assert np.array_equal(points[0], first), i
        else:
            assert a["state"] == DONE, i
            assert (a["t_best"], a["f_best"]) == (bits(t), bits(f)), (i, q)
            assert a["evals"] == evals == len(points) == len(a["consumed"]), (i, q)
            assert [e["point"] for e in a["consumed"]] == [[bits(v) for v in p] for p in points], (i, q)
            # a speculative value used: consumed from slot 1 or 2, in the round of the primary request before it
            for prev, e in zip(a["consumed"], a["consumed"][1:]):
                if e["slot"] > 0:
                    assert e["round"] == prev["round"], i
                    spec_used["doubling" if a["increases"] > 0 else "halving"] += 1
            # ... and dropped: posted, not consumed, and not counted (evals is the oracle's count, above)
            assert a["posted"] >= len(a["consumed"]), i
            later_posted = a["posted"] - 3 if a["rounds"] > 1 else 0        # (the first round posts three)
            dropped_later += later_posted > sum(1 for e in a["consumed"] if e["round"] > 1)
        taken.update(exits_of(q, a, f0))
    assert all(taken[name] > 0 for name in EXITS), {name: taken[name] for name in EXITS}
    assert spec_used["doubling"] > 0 and spec_used["halving"] > 0, spec_used
    assert dropped_later > 0                                                # (beyond the first round, which always drops one of its three)


def sequential_queries_of(dtype):
    """The grid of the speculative test, plus what only the sequential driver serves: the exits of the tiny-step path and constraints."""
    eps = np.finfo(dtype).eps
    huge = 2.0 ** (100 if dtype is np.float32 else 1000)
    bowl = dict(kind=1, x=[1.0], dir=[1.0], c=[1.0], m=[0.0])               # f(t) = (1 - t)^2 along x - t dir
    qs = queries_of(dtype)
    qs.append(query(dtype, 0, [huge], [1 / huge], [1.0], [0.0], t0=1.0))    # :91-101: t overflows before huge - t / huge moves
    for t0 in (eps / 8, eps / 1024):                                        # :119: 1 + t clamped back to the bound, which is x
        qs.append(query(dtype, 1, [1.0], [-1.0], [1.0], [0.0], t0=t0, cons=(CLAMP, 0.0, 1.0)))
    qs.append(query(dtype, 1, [1.0, 0.5], [-1.0, 0.0], [1.0, 1.0], [0.0, 0.0], t0=eps / 8, cons=(CLAMP, 0.0, 1.0)))
    qs.append(query(dtype, t0=eps / 8, cons=(REFUSE, 1.0, 1.0), **bowl))    # :111: every point but x is infeasible
    qs.append(query(dtype, t0=eps / 8, cons=(CLAMP, 0.0, 1.0), **bowl))     # tiny, but the point moves inwards: the search goes on
    qs.append(query(dtype, t0=eps / 8, cons=(REFUSE, 0.0, 1.0), **bowl))
    for t0 in (2.0 ** -6, 0.1):                                             # doubling into the infeasible region: typemax(T) > fa
        qs.append(query(dtype, t0=t0, cons=(REFUSE, 0.75, 1.0), **bowl))
        qs.append(query(dtype, t0=t0, cons=(CLAMP, 0.75, 1.0), **bowl))     # ... onto the bound twice: :150
    for t0 in (4.0, 64.0):                                                  # the first point infeasible: halving back into the box
        qs.append(query(dtype, t0=t0, cons=(REFUSE, 0.0, 1.0), **bowl))
        qs.append(query(dtype, t0=t0, cons=(CLAMP, -0.5, 1.0), **bowl))
    qs.append(query(dtype, t0=0.25, cons=(REFUSE, 0.4, 1.0), **bowl))       # bracket (0.25, 0.5): the parabola's minimum is infeasible
    rng = np.random.default_rng(11)
    for kind in (0, 1, 2):
        for n in (1, 2, 3):
            for _ in range(12):
                x = rng.uniform(-1, 1, n)
                qs.append(query(dtype, kind, x, rng.uniform(-2, 2, n), rng.uniform(0.1, 2.0, n), rng.uniform(-2, 2, n),
                                t0=2.0 ** rng.uniform(-40, 4), max_increases=int(rng.choice([0, 0, 3])), sign=float(rng.choice([-1.0, 1.0])),
                                cons=(int(rng.choice([CLAMP, REFUSE])), -1.0 - rng.uniform(0, 1), 1.0 + rng.uniform(0, 1))))
    return qs


def sequential_exits_of(q, a, f0):
    """exits_of for the sequential driver, which also says what the tiny-step path met."""
    out, rest = [], exits_of(q, a, f0)
    if rest[0] in EXITS[:3]:                                                # nothing to search along
        return rest
    if a["unchanged"] > 0:
        if a["evals"] == 0:
            return ["tiny: infeasible" if a["infeasible"] else "tiny: step overflows"]
        if a["at_x"]:
            return ["tiny: clamped back to x"]
        out.append("tiny: moved on")
    if a["infeasible"] > 0:
        out.append("infeasible trial")
    return out + rest


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_sequential_loop_searches_as_the_oracle_does_tiny_steps_and_constraints_included(driver, dtype):
    """The header's own sequential loop (phi_sequential_run) over the tool's evaluator: for EVERY query the oracle's result, the
    oracle's evaluation count, and the oracle's evaluated points in order -- no evaluation that the oracle does not make."""
    qs = sequential_queries_of(dtype)
    answers = driver(qs, sequential=True)
    oracles = {(n, c): CallbackBFGS(dtype, n, constrained=c) for n in (1, 2, 3) for c in (False, True)}
    taken = collections.Counter()
    for i, (q, a) in enumerate(zip(qs, answers)):
        f0 = objective(q["kind"], q["c"], q["m"], q["x"]) if q["f0"] is None else q["f0"]
        assert a["f0"] == bits(f0), i
        t, f, evals, points = oracles[len(q["x"]), q["cons"][0] != NO_CONSTRAINT].search(q, f0)
        assert a["state"] == DONE, (i, q)
        assert (a["t_best"], a["f_best"]) == (bits(t), bits(f)), (i, q)
        assert a["evals"] == evals == len(points), (i, q)
        assert [e["point"] for e in a["consumed"]] == [[bits(v) for v in p] for p in points], (i, q)
        exits = sequential_exits_of(q, a, f0)
        # :150 is asked for last: only of a doubling that the three cheaper tests of :147-149 let pass
        assert a["compared"] == a["increases"] - any(e.startswith("doubling:") and e != "doubling: stagnation" for e in exits), (i, q)
        taken.update(exits)
    assert [name for name in SEQUENTIAL_EXITS if taken[name] == 0] == []


def test_reading_test_of_the_search():
    """One definition of each decision for the dense optimizer: the header's.  One speculative caller on the host, one on the device
    and one sequential caller; the header free of HIP.  The batched step kernel keeps its own search (measured slower as the header
    loop's evaluator), and nothing else of the search."""
    csrc = os.path.join(ROOT, "dzoptimization.jl_amd", "csrc")
    header = open(os.path.join(csrc, "dzo_phi_search.h")).read()
    bfgs = open(os.path.join(csrc, "dzo_bfgs.hip")).read()
    batch = open(os.path.join(csrc, "dzo_batch.hip")).read()
    assert [ln for ln in header.splitlines() if ln.startswith("#include")] == ["#include <cmath>", "#include <cstdint>"]
    assert "PhiSearch" not in bfgs and "PhiDev" not in bfgs and "phi_dev_feed" not in bfgs and "phi_search_feed" not in bfgs
    assert (header + bfgs).count("max_increases > 0") == 1 and header.count("max_increases > 0") == 1   # the shared feed
    assert batch.count("max_increases > 0") == 1                            # ... and the batched kernel's own bracket
    assert "bfgs_bracket" not in bfgs and "bfgs_quadratic_search" not in bfgs
    code = "\n".join(line.split("//")[0] for line in bfgs.splitlines())
    sequential = code[code.index("static int32_t bfgs_sequential_search("):code.index("struct PhiBuffers {")]
    assert code.count("phi_sequential_search(") == 1 and sequential.count("phi_sequential_search(") == 1
    assert code.count("phi_sequential_run(") == 0 and code.count("phi_tiny_double(") == 0
    batch_code = "\n".join(line.split("//")[0] for line in batch.splitlines())
    assert "phi_" not in batch_code and "b_rosen_" not in batch               # (its elementwise Rosenbrock pieces are dzo_rosen.h's)
    kernel = code[code.index("void finish_phi6_advance_kernel("):code.index("static int dev_search_rounds()")]
    host = code[code.index("static int32_t bfgs_dual_search("):code.index("struct BfgsSearchDev {")]
    for name in ("phi_consume(", "phi_post("):
        assert kernel.count(name) == 1 and host.count(name) == 1, name
    assert code.count("phi_consume(") == 2 and host.count("phi_begin(") == 1
    assert code.count("phi_feed(") == 0 and code.count("phi_result(") == 1 and code.count("phi_quadratic_request(") == 0
    assert "% 4) * 6" not in code                                           # the pool index has one name, phi_pool_index
