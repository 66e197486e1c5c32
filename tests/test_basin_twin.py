"""tests/basin_twin.py on the CPU, against things it does not depend on: its jump ahead against advancing one draw at a time
and against csrc/dzo_pcg.h compiled on the host (tools/pcg_jump_table.cpp, built with -Wall -Werror and the address and
undefined-behaviour sanitizers and run as a process of its own); its draws against tempering_twin's; and a simulated run of a
few 13-atom walkers on quench_twin.Quench."""
import os
import subprocess

import numpy as np
import pytest

import basin_twin as bt
import pairwise_twin as pw
import tempering_twin as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "pcg_jump_table.cpp")
N = 13
JUMPS = [0, 1, 4 * N + 1, 4 * 1023]
SEEDS = [0, 1, 12345, 2 ** 64 - 1]


def _sequential(state, k):
    return tt.pcg_raw(state, k)[1]


def test_jump_equals_sequential_advancing():
    for seed in SEEDS:
        s = tt.pcg_state(seed)
        for k in JUMPS + [2, 3, 64, 255, 4 * 64, 4 * 1024 + 1]:
            assert bt.pcg_jump(s, k) == _sequential(s, k), (seed, k)
    s = tt.pcg_state(7)
    assert bt.pcg_jump(bt.pcg_jump(s, 53), 4092) == bt.pcg_jump(s, 53 + 4092)
    assert bt.pcg_jump(s, 2 ** 64) == s                     # the period


def test_host_build_of_the_header_prints_the_same_states(tmp_path):
    exe = str(tmp_path / "pcg_jump_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    for seed in SEEDS:
        s = tt.pcg_state(seed)
        out = subprocess.run([exe, "%x" % s] + [str(k) for k in JUMPS], check=True, capture_output=True, text=True).stdout.split("\n")
        for k, line in zip(JUMPS, out):
            kk, jumped, advanced, draw, a, c = (int(v, 16) for v in line.split())
            assert kk == k and jumped == advanced == bt.pcg_jump(s, k), (seed, k)
            assert draw == int(tt.pcg_raw(advanced, 1)[0][0])
            assert (a * s + c) % 2 ** 64 == jumped


def test_hop_draws_follow_the_tempering_formulas():
    s = tt.pcg_state(99)
    for dtype in (np.float64, np.float32):
        normals, u, after = bt.hop_draws(s, N, dtype)
        assert after == bt.pcg_jump(s, 4 * N + 1) and normals.shape == (N, 3) and normals.dtype == dtype
        raw, _ = tt.pcg_raw(s, 4 * N + 1)
        for i in range(N):
            # particle i: the draws d1 .. d4 of a tempering step whose d0 and d5 are anything
            six = np.concatenate([[0], raw[4 * i:4 * i + 4], [0]])
            _, n3, _, _ = tt.step_draws(six.reshape(1, 6), N, dtype)
            assert np.array_equal(n3[0], normals[i])
            assert bt.pcg_jump(s, 4 * i) == _sequential(s, 4 * i)
        assert u == np.dtype(dtype).type(float(raw[4 * N]) * 2.0 ** -32) and 0 <= u <= 1


def test_trial_keeps_particles_that_leave_the_sphere():
    p = np.concatenate(pw.icosahedron13()).astype(np.float64)
    normals, _, _ = bt.hop_draws(tt.pcg_state(3), N, np.float64)
    moved_all, inside = bt.trial(p, 0.05, normals, np.inf, np.float64)
    assert inside.all() and not np.any(moved_all == p)
    assert np.array_equal(moved_all.reshape(3, N), p.reshape(3, N) + np.float64(0.05) * normals.T)
    kept, inside = bt.trial(p, 0.05, normals, 1e-3, np.float64)
    assert not inside.any() and np.array_equal(kept, p)
    R = float(np.sqrt((moved_all.reshape(3, N) ** 2).sum(axis=0)).mean())
    some, inside = bt.trial(p, 0.05, normals, R, np.float64)
    assert 0 < inside.sum() < N
    assert np.array_equal(some.reshape(3, N)[:, inside], moved_all.reshape(3, N)[:, inside])
    assert np.array_equal(some.reshape(3, N)[:, ~inside], p.reshape(3, N)[:, ~inside])


@pytest.fixture(scope="module")
def walkers():
    """three LJ13 walkers from jittered icosahedra, radius 0.4 at temperature 0.8, six hops each"""
    out = []
    for k in range(3):
        start = np.concatenate(pw.jittered(pw.icosahedron13(), 10 + k, 0.05))
        w = bt.Walker(start, 1.25, 0.4, 3.0, seed=40 + k)
        for _ in range(6):
            w.hop()
        out.append(w)
    return out


def test_simulated_walkers(walkers):
    codes = set()
    for k, w in enumerate(walkers):
        assert w.hops == 6 and w.num_accept + w.num_reject == 6
        assert w.state == bt.pcg_jump(tt.pcg_state(40 + k), 6 * (4 * N + 1))           # 4N + 1 draws per hop
        best, e, x = None, None, None
        for i, h in enumerate(w.log):
            assert h["after"] == bt.pcg_jump(h["state"], 4 * N + 1)
            assert i == 0 or h["state"] == w.log[i - 1]["after"]
            assert h["klass"] != tt.UNDECIDED and h["code"] == (bt.CODE_ACCEPTED if h["klass"] == tt.MUST_ACCEPT else bt.CODE_REJECTED)
            assert h["e_q"] <= bt.qt.energy_gradient(h["trial"])[0]                    # a quench does not raise the energy
            codes.add(h["code"])
            if i > 0:
                assert h["e_before"] == e
            if h["code"] == bt.CODE_ACCEPTED:                                          # an accepted state is the quenched one
                e, x = h["e_q"], h["x_q"]
            elif i == 0:
                e = h["e_before"]
            lowest = min(hh["e_q"] for hh in w.log[:i + 1])
            assert best is None or min(lowest, w.log[0]["e_before"]) <= best           # BEST is monotone
            best = min(lowest, w.log[0]["e_before"])
        assert w.best_e == best and w.e == e
        if x is not None:
            assert np.array_equal(w.x, x)
        assert w.best_e <= w.e and w.best_e == bt.qt.energy_gradient(w.best_x)[0]
        assert w.iterations == sum(h["iterations"] for h in w.log)
    assert codes == {bt.CODE_ACCEPTED, bt.CODE_REJECTED}, "the walkers take both branches of the decision"
    assert min(w.best_e for w in walkers) < -44.3268                                   # the icosahedron


def test_decide_classes():
    t = np.float64
    assert bt.decide(t(-1.0), t(0.0), t(0.99), 1.0, t) == (tt.MUST_ACCEPT, bt.CODE_ACCEPTED)
    assert bt.decide(t(0.0), t(0.0), t(1.0), 1.0, t) == (tt.MUST_ACCEPT, bt.CODE_ACCEPTED)       # delta <= 0
    assert bt.decide(t(1.0), t(0.0), t(0.5), 1.0, t) == (tt.MUST_REJECT, bt.CODE_REJECTED)       # exp(-1) = 0.37
    assert bt.decide(t(1.0), t(0.0), t(0.3), 1.0, t) == (tt.MUST_ACCEPT, bt.CODE_ACCEPTED)
    assert bt.decide(t(np.inf), t(0.0), t(0.0), 1.0, t)[1] == bt.CODE_NOT_FINITE
    assert bt.decide(t(np.nan), t(0.0), t(0.0), 1.0, t)[1] == bt.CODE_NOT_FINITE
    assert bt.decide(t(-3.0), t(np.nan), t(0.0), 1.0, t) == (tt.MUST_REJECT, bt.CODE_REJECTED)   # a NaN energy stays
    u = t(np.exp(-1.0))
    assert bt.decide(t(1.0), t(0.0), u, 1.0, t)[0] == tt.UNDECIDED                              # within the band of exp's rounding
