"""The batched L-BFGS quench (csrc/dzo_lbfgs_batch.hip) at the shapes where its three step kernels change what they do, and at
history lengths from 1 to 32 with the ring turning past its end.  tests/test_gpu_quench.py runs N = 13, 38, 200 at history
length 10; here every (N, m) of tests/quench_checks.py CASES runs in both element types:

* the wave kernel at N = 2..4, with dropped padding pairs inside the 4-unrolled trip (61, 63) and as a full wave (64);
* the block kernel with three waves that own nothing (65, 66), around the first thread with a second particle (255..257), and
  with up to four particles per thread (513, 1023, 1024);
* the last (N, m) whose history ring fits the LDS and the first whose ring goes to device memory, per element type.

a. objective and gradient against the longdouble twin, within the derived (N + 32) u S, at the start and after six steps
   (N <= 4: after one, see quench_checks.SEEDS);
b. every direction against the oracle and the twin over m + 8 single steps, and the ring moving by one each step;
c. every step replayed: the point is fma(2^-h, d, x_old) exactly, every decision the twin's where its energies are apart;
d. one launch of m + 5 steps against m + 5 launches of one step and against step(m) + step(5), bit for bit.
(b) holds the launches of one step, whose ring starts at head 0, to the oracle; (d) ties the moving head to them.
"""
import numpy as np
import pytest

import pairwise_twin as tw
import quench_checks as qc
import quench_twin as qt
from dzo_loader import dzo

LD = np.longdouble
gpu = pytest.mark.gpu
cases = pytest.mark.parametrize("n,m", qc.CASES)
dtypes = pytest.mark.parametrize("dtype", qc.DTYPES)


@pytest.fixture(scope="module")
def device():
    dzo.init(0)


# ------------------------------------------------------------------------------ the table (no GPU)
def test_shape_table_covers_every_path_on_both_sides_of_its_limits():
    """quench_checks.path restates the constructor's choice; if kClLdsMax or the LDS layout changes, this names the cases that
    moved."""
    assert qc.LDS_MAX == 162816 and qc.lds_request(98, 32, np.float64) == 16 * 32 + 128 + 69 * 3 * 98 * 8
    for dtype in qc.DTYPES:
        taken = {qc.path(n, m, dtype) for n, m in qc.CASES}
        assert taken == {qc.WAVE, qc.BLOCK_LDS, qc.BLOCK_SLAB}, (np.dtype(dtype).name, taken)
        for fits, spills in qc.LDS_EDGES[np.dtype(dtype)]:
            assert fits in qc.CASES and spills in qc.CASES
            assert qc.path(*fits, dtype) == qc.BLOCK_LDS and qc.lds_request(*fits, dtype) <= qc.LDS_MAX, (fits, qc.lds_request(*fits, dtype))
            assert qc.path(*spills, dtype) == qc.BLOCK_SLAB and qc.lds_request(*spills, dtype) > qc.LDS_MAX, (spills, qc.lds_request(*spills, dtype))
            # neighbours: one more particle at the same history length, or one more pair at the same N
            assert (spills[0] - fits[0], spills[1] - fits[1]) in ((1, 0), (0, 1)), (fits, spills)
    assert qc.path(64, 32, np.float64) == qc.WAVE and qc.path(65, 1, np.float32) == qc.BLOCK_LDS
    assert qc.path(1024, 1, np.float64) == qc.BLOCK_SLAB and qc.path(1024, 4, np.float32) == qc.BLOCK_LDS
    ns, ms = {n for n, _ in qc.CASES}, {m for _, m in qc.CASES}
    assert {2, 3, 4, 61, 63, 64, 65, 66, 255, 256, 257, 513, 1023, 1024} <= ns and {1, 2, 3, 10, 32} <= ms
    assert max(ns) == qc.MAX_N == dzo.LBFGS_BATCH_MAX_PARTICLES and max(ms) == qc.MAX_M == dzo.LBFGS_BATCH_MAX_HISTORY
    for n, m in qc.CASES:
        assert len(qc.seeds_of(n, m)) == qc.batch_of(n) and m + 8 <= 45


# ------------------------------------------------------------------------------ a. against the longdouble twin
@gpu
@dtypes
@cases
def test_objective_and_gradient_against_the_twin(device, n, m, dtype):
    dev, opt = qc.make(qc.starts(n, m, dtype), n, m)
    u = qc.U[np.dtype(dtype)]
    for k in (0, qc.steps_before_the_second_look(n)):
        if k:
            opt.step(k)
        st = qc.state(opt)
        qc.consistent(opt, n, st, (n, m, k))
        assert qc.same(dzo.pairwise_batch_energy_gradient(opt.points, n), st["OBJECTIVES"]), (n, m, k, "energies without a gradient buffer")
        worst_e = worst_g = 0.0
        for b in range(opt.batch):
            p = st["POINTS"][b].astype(np.float64)
            x, y, z = p[:n], p[n:2 * n], p[2 * n:]
            E, S = tw.energy(x, y, z)
            err = abs(LD(st["OBJECTIVES"][b]) - E)
            bound = LD(n + 32) * u * S
            worst_e = max(worst_e, float(err / bound))
            assert err <= bound, (n, m, k, b, float(err), float(bound))
            g, Srow, _ = tw.gradient(x, y, z)
            errg = np.abs(st["GRADIENTS"][b].reshape(3, n).astype(LD) - g)
            boundg = LD(n + 32) * u * Srow[None, :]
            worst_g = max(worst_g, float(np.max(errg / boundg)))
            assert np.all(errg <= boundg), (n, m, k, b, float(np.max(errg / boundg)))
        print(f"N={n} m={m} {np.dtype(dtype).name} after {k} steps: worst error / bound: energy {worst_e:.4f}, gradient {worst_g:.4f}")


# ------------------------------------------------------------------------------ b. directions and the ring across the wrap
@gpu
@dtypes
@cases
def test_direction_against_the_oracle_across_the_wrap(device, n, m, dtype):
    dev, opt = qc.make(qc.starts(n, m, dtype), n, m)
    worst = qc.check_directions_and_ring(opt, n, m, dtype, m + 8)
    print(f"N={n} m={m} {np.dtype(dtype).name}: worst direction error / tolerance {worst:.4f} (tolerance {qc.tol_direction(m, dtype):.1e})")


# ------------------------------------------------------------------------------ c. step replay
@gpu
@dtypes
@cases
def test_step_replay(device, n, m, dtype):
    t = np.dtype(dtype).type
    window = qc.window(n, dtype)
    dev, opt = qc.make(qc.starts(n, m, dtype), n, m)
    undecided = trials = 0
    cur = qc.state(opt)
    for k in range(window + 4):                              # the point is replayed on every step, decisions inside the window
        before = cur
        opt.step(1)
        cur = qc.state(opt)
        for b in range(opt.batch):
            if before["IS_STUCK"][b]:
                continue
            x_old, d, h = before["POINTS"][b], cur["DIRECTIONS"][b], int(cur["LAST_HALVINGS"][b])
            if not cur["IS_STUCK"][b]:
                assert qc.same(cur["POINTS"][b], x_old + t(2.0 ** -h) * d), (n, m, k, b, h)     # 2^-h d is exact: the bits of the fma
            if k >= window:
                continue
            last = h if not cur["IS_STUCK"][b] else h - 1
            old = qt.exact_energy(x_old)
            for hh in range(last + 1):
                x_t = x_old + t(2.0 ** -hh) * d
                diff, bound = qt.decision_margin(x_old, x_t, dtype, old)
                trials += 1
                if abs(diff) <= bound:
                    undecided += 1
                    continue
                if hh == h and not cur["IS_STUCK"][b]:
                    assert diff <= bound, (n, m, k, b, hh, "accepted a trial that does not decrease", float(diff), float(bound))
                else:
                    assert diff >= -bound, (n, m, k, b, hh, "rejected a trial that decreases", float(diff), float(bound))
    print(f"N={n} m={m} {np.dtype(dtype).name}: {undecided} of {trials} trials undecided in the first {window} steps")
    assert trials >= window * opt.batch and undecided == 0


# ------------------------------------------------------------------------------ d. one launch against many
@gpu
@dtypes
@cases
def test_one_launch_against_many(device, n, m, dtype):
    st = qc.check_one_launch_against_many(qc.starts(n, m, dtype), n, m, m + 5)
    assert np.all((st["HISTORY_COUNTS"] == m) | (st["IS_STUCK"] != 0))
