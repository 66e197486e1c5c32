"""What the handle classes of the Python binding send to the C ABI, call by call (CPU only, no library, no device).

``dzo.lib`` is replaced by a recorder: every symbol is a callable that appends ``(symbol, args)`` to a list and returns 0 (or the
code set in ``rc``).  Through a ``ctypes.byref`` it stores what the library would: a made-up handle through a ``c_void_p``,
``i32`` / ``i64`` through a ``c_int32`` / ``c_int64``.  Device arrays wrap made-up addresses, so nothing is allocated.  Recorded
arguments are normalised: a handle to its address, a ``byref`` to ``("byref", type)``, a ``double *`` of a host array to the
tuple of its first ``host_len`` values (read at the time of the call)."""
import ctypes as C
import gc

import numpy as np
import pytest

from dzo_loader import dzo

BVP, B32, B64 = (("byref", t.__name__) for t in (C.c_void_p, C.c_int32, C.c_int64))
MASK = (1 << 64) - 1
N, B = 2, 3                                     # particles per cluster, clusters per handle
BETA, RADII = (2.0, 1.0, 0.5), (0.1, 0.2, 0.3)
ISSUED = []                                     # every made-up handle of the running test (the ``c_void_p`` objects themselves)


class Recorder:
    def __init__(self):
        self.calls, self.rc, self.fill, self.peek = [], {}, {}, {}
        self.i32, self.i64, self.host_len, self.next_handle = 0, 0, B, 0x5000

    def _norm(self, a):
        if type(a).__name__ == "CArgObject":
            return ("byref", type(a._obj).__name__)
        if isinstance(a, C.c_void_p):
            return a.value
        if isinstance(a, C.POINTER(C.c_double)):
            return tuple(a[:self.host_len])
        return a

    def __getattr__(self, name):
        def fn(*args):
            rec = tuple(self._norm(a) for a in args)
            if name in self.peek:                                   # the bytes behind the last argument, a host address
                rec = rec[:-1] + (C.string_at(args[-1], self.peek[name]),)
            self.calls.append((name, rec))
            for a in args:
                obj = getattr(a, "_obj", None) if type(a).__name__ == "CArgObject" else None
                if isinstance(obj, C.c_void_p):
                    obj.value, self.next_handle = self.next_handle, self.next_handle + 0x10
                    ISSUED.append(obj)
                elif isinstance(obj, C.c_int32):
                    obj.value = self.i32
                elif isinstance(obj, C.c_int64):
                    obj.value = self.i64
            if name.endswith("_read") and (name, args[1]) in self.fill:
                src = np.ascontiguousarray(self.fill[name, args[1]])
                C.memmove(args[-1], src.ctypes.data, src.nbytes)
            return b"x" if name == "dzo_last_error" else self.rc.get(name, 0)
        return fn

    def named(self, symbol):
        return [args for name, args in self.calls if name == symbol]


@pytest.fixture
def fake(monkeypatch):
    f = Recorder()
    monkeypatch.setattr(dzo, "lib", lambda: f)
    monkeypatch.setattr(dzo, "_lib", object())
    monkeypatch.setattr(dzo, "_inited", True)
    yield f
    for h in ISSUED:                            # a failed test's traceback keeps its objects: their handles must not reach a
        h.value = None                          # real library once ``dzo.lib`` is back
    ISSUED.clear()


def dev(shape, ptr, dtype=np.float64):
    return dzo.DeviceArray(shape, dtype, ptr=ptr, owner=False)


def points(ptr=0x1000, dtype=np.float64):
    return dev(3 * N * B, ptr, dtype)


# every maker returns (handle object, what must outlive it, create symbol, prefix)
def make_tempering():
    return dzo.ParallelTempering(points(), N, BETA, RADII, 3.0, base_seed=-1), None, "dzo_tempering_create", "dzo_tempering_"


def make_lbfgs():
    return dzo.BatchedLBFGS(points(), N, 0.01, 4), None, "dzo_lbfgs_batch_create", "dzo_lbfgs_batch_"


def make_adgd():
    return dzo.BatchedAdGD(points(), N, 0.02), None, "dzo_adgd_batch_create", "dzo_adgd_batch_"


def make_basin():
    return (dzo.BasinHopping(points(), N, BETA, RADII, 4.0, 0.03, 5, 40, base_seed=-2), None, "dzo_basin_hopping_create",
            "dzo_basin_hopping_")


def make_modefollow():
    return dzo.ModeFollowing(points(), N, 1, 0.25, 1e-3, 1e-9), None, "dzo_modefollow_batch_create", "dzo_modefollow_batch_"


def make_hybridef():
    return (dzo.HybridModeFollowing(points(), N, dev((B, 3 * N), 0x2000), 0.11, 9, 3, 0.06, 0.02, 7, 2, 1e-2, 1e-5, 1e-8, seed=-3),
            None, "dzo_hybridef_batch_create", "dzo_hybridef_batch_")


def make_bfgs_batch():
    return dzo.BatchedBFGS(dzo.ROSENBROCK_CHAIN, dev((B, 4), 0x3000), 0.5), None, "dzo_bfgs_batch_create", "dzo_bfgs_batch_"


def make_problem():
    return dzo.Problem(dzo.ROSENBROCK_CHAIN, 6), None, "dzo_problem_create", "dzo_problem_"


def comm_handle():
    ISSUED.append(C.c_void_p(0x7000))
    return ISSUED[-1]


def make_comm():
    return dzo.Comm(comm_handle()), None, None, "dzo_comm_"


def make_lbfgs_single():
    problem = dzo.Problem(dzo.ROSENBROCK_CHAIN, 6)
    return dzo.LBFGSOptimizer(None, problem, None, dev(6, 0x4000), 1.5, 5), problem, "dzo_lbfgs_create_problem", "dzo_lbfgs_"


def make_adgd_single():
    problem = dzo.Problem(dzo.ROSENBROCK_CHAIN, 6)
    return dzo.AdGDOptimizer(None, problem, None, dev(6, 0x4000), 1.5), problem, "dzo_adgd_create_problem", "dzo_adgd_"


def make_bfgs_single():
    problem = dzo.Problem(dzo.ROSENBROCK_CHAIN, 6)
    return dzo.BFGSOptimizer(problem, None, dev(6, 0x4000), 1.5), problem, "dzo_bfgs_create_problem", "dzo_bfgs_"


MAKERS = [make_tempering, make_lbfgs, make_adgd, make_basin, make_modefollow, make_hybridef, make_bfgs_batch, make_problem, make_comm,
          make_lbfgs_single, make_adgd_single, make_bfgs_single]
STEPPERS = [make_lbfgs, make_adgd, make_modefollow, make_hybridef]
F64 = dzo.F64


# ------------------------------------------------------------------------------ construction
def test_tempering_create(fake):
    pt = make_tempering()[0]
    assert fake.calls == [("dzo_tempering_create", (0, N, B, F64, 0x1000, BETA, RADII, 3.0, MASK, BVP))]
    assert pt.h.value == 0x5000 and (pt.n_particles, pt.n_replicas, pt.record_capacity) == (N, B, 0) and pt.replicas.ptr == 0x1000
    with pytest.raises(AssertionError):
        dzo.ParallelTempering(points(), N, BETA, RADII[:2], 3.0)
    with pytest.raises(AssertionError, match="replicas must hold"):
        dzo.ParallelTempering(dev(3 * N * B + 1, 0x1000), N, BETA, RADII, 3.0)
    assert len(fake.calls) == 1


def test_batched_optimizers_create(fake):
    opt = make_lbfgs()[0]
    assert fake.calls == [("dzo_lbfgs_batch_create", (0, N, B, F64, 0x1000, 0.01, 4, BVP))]
    assert (opt.n_particles, opt.batch, opt.history_length, opt.dtype) == (N, B, 4, np.float64) and opt.points.ptr == 0x1000
    fake.calls.clear()
    opt32 = dzo.BatchedAdGD(points(0x1100, np.float32), N, 0.02, radial=dzo.RADIAL_LENNARD_JONES)
    assert fake.calls == [("dzo_adgd_batch_create", (0, N, B, dzo.F32, 0x1100, 0.02, BVP))]
    assert opt32.h.value == 0x5010 and opt32.batch == B
    for cls, args in ((dzo.BatchedLBFGS, (0.01, 4)), (dzo.BatchedAdGD, (0.02,))):
        with pytest.raises(AssertionError, match="points must hold 3 \\* n_particles \\* batch elements"):
            cls(dev(3 * N * B + 1, 0x1000), N, *args)


def test_basin_hopping_create(fake):
    bh = make_basin()[0]
    assert fake.calls == [("dzo_basin_hopping_create", (0, N, B, F64, 0x1000, BETA, RADII, 4.0, 0.03, 5, 40, MASK - 1, BVP))]
    assert (bh.batch, bh.history_length, bh.quench_steps, bh.record_capacity, bh.constraining_radius) == (B, 5, 40, 0, 4.0)
    with pytest.raises(AssertionError):
        dzo.BasinHopping(points(), N, BETA, RADII[:2], 4.0)
    with pytest.raises(AssertionError, match="points must hold"):
        dzo.BasinHopping(points(), N, BETA[:2], RADII[:2], 4.0)       # the batch is the number of walkers, not size / 3N
    assert len(fake.calls) == 1


def test_mode_following_create(fake):
    mf = make_modefollow()[0]
    assert fake.calls == [("dzo_modefollow_batch_create", (0, N, B, F64, 0x1000, 1, 0.25, 1e-3, 1e-9, BVP))]
    assert (mf.n_particles, mf.batch) == (N, B)
    fake.calls.clear()
    he = make_hybridef()[0]
    assert fake.calls == [("dzo_hybridef_batch_create", (0, N, B, F64, 0x1000, 0x2000, 0.11, 9, 3, 0.06, 0.02, 7, 2, 1e-2, 1e-5, 1e-8,
                                                         MASK - 2, BVP))]
    assert (he.n_particles, he.batch) == (N, B)
    fake.calls.clear()
    drawn = dzo.HybridModeFollowing(points(), N)                # no directions: drawn in the kernel from the seed
    assert drawn.h and fake.calls == [("dzo_hybridef_batch_create", (0, N, B, F64, 0x1000, None, 0.1, 10, 2, 0.05, 0.01, 8, 1, 1e-3, 1e-4, 1e-10, 0, BVP))]
    with pytest.raises(AssertionError, match="directions must be laid out like points"):
        dzo.HybridModeFollowing(points(), N, dev(3 * N * B - 1, 0x2000))
    for cls in (dzo.ModeFollowing, dzo.HybridModeFollowing):
        with pytest.raises(AssertionError, match="points must hold"):
            cls(dev(3 * N * B + 1, 0x1000), N)


@pytest.mark.parametrize("make", [make_lbfgs, make_adgd, make_modefollow, make_hybridef])
def test_no_particles_reach_the_c_argument_check(fake, make):
    """``n_particles <= 0`` is the library's to refuse: the constructor passes it on with batch 0."""
    _, _, create, _ = make()
    cls, fake.rc[create] = type(make()[0]), 1
    fake.calls.clear()
    extra = {dzo.BatchedLBFGS: (0.01, 4), dzo.BatchedAdGD: (0.02,)}.get(cls, ())
    for n in (0, -1):
        with pytest.raises(dzo.DzoError):
            cls(dev(0, 0x1000), n, *extra)
    assert [(name, args[1:3]) for name, args in fake.calls if name == create] == [(create, (0, 0)), (create, (-1, 0))]


def test_problem_and_single_instance_create(fake):
    p = dzo.Problem(dzo.QUADRATIC, 6, np.float32, A=dev((6, 6), 0x8000, np.float32), c=dev(6, 0x8100, np.float32), lam=0.25, l2=0.5,
                    box_gradient=(-1.0, 2.0), box_constraint=(-3.0, 4.0))
    h = p.h.value
    assert fake.calls == [("dzo_problem_create", (dzo.QUADRATIC, 6, dzo.F32, 0x8000, 0x8100, 0.25, BVP)), ("dzo_problem_set_l2", (h, 0.5)),
                          ("dzo_problem_set_box_gradient", (h, 1, -1.0, 2.0)), ("dzo_problem_set_box_constraint", (h, 1, -3.0, 4.0))]
    fake.calls.clear()
    assert p(dev(6, 0x8200, np.float32)) == 0.0
    p.gradient_(dev(6, 0x8300, np.float32), dev(6, 0x8200, np.float32))
    assert fake.calls == [("dzo_problem_eval", (h, 0x8200, ("byref", "c_double"))), ("dzo_problem_grad", (h, 0x8300, 0x8200))]
    fake.calls.clear()
    opt, problem, _, _ = make_lbfgs_single()
    ph, oh = problem.h.value, opt.h.value
    assert fake.calls == [("dzo_problem_create", (dzo.ROSENBROCK_CHAIN, 6, F64, None, None, 0.0, BVP)),
                          ("dzo_lbfgs_create_problem", (ph, 5, 0x4000, 1.5, BVP))]
    fake.calls.clear()
    fake.i64 = 7
    assert opt.step() is opt and opt.iteration_count == 7 and opt.is_stuck is True and opt.current_objective_value == 0.0
    field = opt.current_gradient
    assert field.ptr == fake.next_handle - 0x10 and opt._get_ptr(5, 3) == fake.next_handle - 0x10
    host = field.to_host()
    assert (host.shape, host.dtype) == ((6,), np.float64)
    assert fake.calls == [("dzo_lbfgs_step", (oh,)), ("dzo_lbfgs_get_i", (oh, 1, B64)), ("dzo_lbfgs_get_i", (oh, 0, B64)),
                          ("dzo_lbfgs_get_s", (oh, 0, ("byref", "c_double"))), ("dzo_lbfgs_get_ptr", (oh, 2, 0, BVP)),
                          ("dzo_lbfgs_get_ptr", (oh, 5, 3, BVP)), ("dzo_lbfgs_read", (oh, 2, 0, host.ctypes.data))]
    fake.calls.clear()
    adgd, problem2, _, _ = make_adgd_single()
    ah = adgd.h.value
    assert fake.named("dzo_adgd_create_problem") == [(problem2.h.value, 0x4000, 1.5, BVP)]
    fake.calls.clear()
    adgd.step()
    host = adgd.delta_point.to_host()
    assert adgd.current_point.ptr and adgd.current_step_size == 0.0 and adgd.fused_steps == 7
    assert fake.calls == [("dzo_adgd_step", (ah,)), ("dzo_adgd_read", (ah, 1, host.ctypes.data)), ("dzo_adgd_get_ptr", (ah, 0, BVP)),
                          ("dzo_adgd_get_s", (ah, 2, ("byref", "c_double"))), ("dzo_adgd_get_i", (ah, 3, B64))]
    fake.calls.clear()
    bfgs, problem3, _, _ = make_bfgs_single()
    bh = bfgs.h.value
    assert fake.calls[1:] == [("dzo_bfgs_create_problem", (problem3.h.value, 0x4000, 1.5, BVP))]
    fake.calls.clear()
    bfgs.step()
    hess = bfgs.approximate_inverse_hessian
    assert hess.shape == (6, 6) and hess.ptr == fake.next_handle - 0x10 and bfgs.has_terminated is True
    assert fake.calls == [("dzo_bfgs_step", (bh,)), ("dzo_bfgs_get_ptr", (bh, 5, BVP)), ("dzo_bfgs_get_i", (bh, 0, B64))]
    fake.calls.clear()
    gd = dzo.GradientDescentOptimizer(problem3, None, None, dev(6, 0x4000), 0.5)
    gh = gd.h.value
    gd.step()
    gd.close()
    assert fake.calls == [("dzo_gd_create_problem", (problem3.h.value, 0x4000, 0.5, BVP)), ("dzo_gd_step", (gh,)), ("dzo_bfgs_destroy", (gh,))]


def test_bfgs_batch_create_step_and_fields(fake):
    b = make_bfgs_batch()[0]
    h = b.h.value
    assert fake.calls == [("dzo_bfgs_batch_create", (dzo.ROSENBROCK_CHAIN, B, 4, F64, 0x3000, 0.5, BVP))]
    fake.calls.clear()
    assert b.step(3, poll=False) is None
    assert b.step(2, poll=True) is False
    fake.i32, fake.i64 = 1, 2
    assert b.step() is True and b.count_active() == 2 and b.device == 1
    x, done = b._p(0, (B, 4)), b.has_terminated
    assert (x.shape, x.dtype, done.shape, done.dtype) == ((B, 4), np.float64, (B,), np.int32) and done.ptr == x.ptr + 0x10
    b.set_max_increases(5)
    assert fake.calls == [("dzo_bfgs_batch_step", (h, 3, None)), ("dzo_bfgs_batch_step", (h, 2, B32)), ("dzo_bfgs_batch_step", (h, 1, B32)),
                          ("dzo_bfgs_batch_count_active", (h, B64)), ("dzo_bfgs_batch_device", (h, B32)),
                          ("dzo_bfgs_batch_get_ptr", (h, 0, BVP)), ("dzo_bfgs_batch_get_ptr", (h, 4, BVP)),
                          ("dzo_bfgs_batch_set_max_increases", (h, 5))]
    fake.calls.clear()
    problem = dzo.Problem(dzo.QUADRATIC, 4)
    on = dzo.BatchedBFGS(problem, dev((B, 4), 0x3000), 0.5)
    mats = dzo.BatchedBFGS(problem, dev((B, 4), 0x3000), 0.5, matrices=dev((B, 4, 4), 0x3100))
    assert fake.calls[1:] == [("dzo_bfgs_batch_create_problem", (problem.h.value, B, 0x3000, 0.5, -1, BVP)),
                              ("dzo_bfgs_batch_create_problem_matrices", (problem.h.value, B, 0x3100, 16, 0x3000, 0.5, -1, BVP))]
    comm = dzo.Comm(comm_handle())
    fake.calls.clear()
    assert comm.nranks == 1 and dzo.batches_all_done([on, mats]) is True
    assert [name for name, _ in fake.calls] == ["dzo_comm_info", "dzo_bfgs_batch_all_done"] and fake.calls[0][1][0] == 0x7000


# ------------------------------------------------------------------------------ stepping
@pytest.mark.parametrize("make", STEPPERS)
def test_step_and_count_active(fake, make):
    opt, _, _, prefix = make()
    h = opt.h.value
    fake.calls.clear()
    assert opt.step(3, wait=False) is None
    assert opt.step(2) is False and opt.count_active() == 0
    fake.i32, fake.i64 = 1, 5
    assert opt.step() is True and opt.count_active() == 5 and type(opt.count_active()) is int
    assert fake.calls == [(prefix + "step", (h, 3, None)), (prefix + "step", (h, 2, B32)), (prefix + "count_active", (h, B64)),
                          (prefix + "step", (h, 1, B32)), (prefix + "count_active", (h, B64)), (prefix + "count_active", (h, B64))]


def test_set_max_halvings_and_the_smaller_entry_points(fake):
    for make in (make_lbfgs, make_adgd, make_basin):
        opt, _, _, prefix = make()
        fake.calls.clear()
        opt.set_max_halvings(7.0)
        assert fake.calls == [(prefix + "set_max_halvings", (opt.h.value, 7))]
    # a class has the methods its unit has entries for, no more
    assert not any(hasattr(dzo.BasinHopping, name) for name in ("step", "count_active", "run"))
    assert not any(hasattr(cls, "set_max_halvings") for cls in (dzo.ModeFollowing, dzo.HybridModeFollowing, dzo.ParallelTempering))
    mf = make_modefollow()[0]
    he = make_hybridef()[0]
    fake.calls.clear()
    mf.set_start_mode(2.0)
    mf.set_directions(dev((B, 3 * N), 0x2100))
    he.set_directions(dev((B, 3 * N), 0x2200))
    assert fake.calls == [("dzo_modefollow_batch_set_start_mode", (mf.h.value, 2)), ("dzo_modefollow_batch_set_directions", (mf.h.value, 0x2100)),
                          ("dzo_synchronize", ()), ("dzo_hybridef_batch_set_directions", (he.h.value, 0x2200)), ("dzo_synchronize", ())]
    for handle in (mf, he):
        with pytest.raises(AssertionError):
            handle.set_directions(dev((B, 3 * N + 1), 0x2100))


def test_basin_hop_chunks_and_tempering_moves(fake):
    bh = make_basin()[0]
    h = bh.h.value
    fake.calls.clear()
    bh.hop(7, adapt=True, hops_per_launch=3)
    bh.hop(2, adapt=False, wait=False)
    bh.set_record(4)
    assert fake.calls == [("dzo_basin_hopping_hop", (h, 3, 0)), ("dzo_basin_hopping_hop", (h, 3, 0)), ("dzo_basin_hopping_hop", (h, 1, 1)),
                          ("dzo_synchronize", ()), ("dzo_basin_hopping_hop", (h, 2, 0)), ("dzo_basin_hopping_set_record", (h, 4))]
    assert bh.record_capacity == 4
    pt = make_tempering()[0]
    h = pt.h.value
    fake.calls.clear()
    pt.temper(8)
    pt.temper(8, dev((B, 8), 0x9000))
    pt.swap(True)
    pt.run(4, 2, dev(16 * B, 0x9000))
    pt.set_record(6)
    assert fake.calls == [("dzo_tempering_temper", (h, 8, None, 0)), ("dzo_tempering_temper", (h, 8, 0x9000, B)), ("dzo_tempering_swap", (h, 1)),
                          ("dzo_tempering_run", (h, 4, 2, 0x9000, 16)), ("dzo_tempering_set_record", (h, 6))]
    assert pt.record_capacity == 6


# ------------------------------------------------------------------------------ the chunked loop
def _steps(fake, prefix):
    return [args[1] for args in fake.named(prefix + "step")]


@pytest.mark.parametrize("make, default", [(make_modefollow, 10), (make_hybridef, 20)])
def test_run_steps_in_chunks_until_nobody_is_active(fake, make, default):
    opt, _, _, prefix = make()
    h = opt.h.value
    count, step = (prefix + "count_active", (h, B64)), lambda k: (prefix + "step", (h, k, B32))
    fake.calls.clear()
    fake.i64 = 5                                                # somebody is active and no step reports done
    assert opt.run(max_steps=25, steps_per_call=10) == 25
    assert fake.calls == [count, step(10), step(10), step(5)]
    fake.calls.clear()
    assert opt.run(45) == 45
    assert fake.calls == [count] + [step(default)] * (45 // default) + [step(45 % default)]
    fake.calls.clear()
    fake.i32 = 1                                                # the first step reports done
    assert opt.run(max_steps=25, steps_per_call=10) == 10
    assert fake.calls == [count, step(10)]
    fake.calls.clear()
    fake.i64 = 0                                                # nobody is active
    assert opt.run(max_steps=25, steps_per_call=10) == 0
    assert fake.calls == [count]


@pytest.mark.parametrize("optimizer, prefix", [("lbfgs", "dzo_lbfgs_batch_"), ("adgd", "dzo_adgd_batch_")])
def test_tempering_quench_steps_a_copy_in_chunks(fake, optimizer, prefix):
    pt = make_tempering()[0]
    for i32, i64, expected in ((0, 5, [10, 10, 5]), (1, 5, [10]), (0, 0, [])):
        fake.calls.clear()
        fake.i32, fake.i64 = i32, i64
        energies, minima, opt = pt.quench(6, 0.02, steps_per_launch=10, max_steps=25, optimizer=optimizer)
        copy = fake.named("dzo_memcpy_d2d")
        assert [name for name, _ in fake.calls[:3]] == ["dzo_malloc", "dzo_memcpy_d2d", prefix + "create"]
        assert copy == [(minima.ptr, 0x1000, 8 * 3 * N * B)] and minima.ptr != 0x1000 and opt.points is minima
        create = fake.named(prefix + "create")[0]
        assert create[:6] == (0, N, B, F64, minima.ptr, 0.02) and (create[6] == 6 if optimizer == "lbfgs" else len(create) == 7)
        assert fake.named(prefix + "count_active") == [(opt.h.value, B64)] and _steps(fake, prefix) == expected
        assert all(args == (opt.h.value, k, B32) for args, k in zip(fake.named(prefix + "step"), expected))
        assert fake.calls[-1][:1] + fake.calls[-1][1][:2] == (prefix + "read", opt.h.value, opt._what["current_objective_values"])
        assert energies.shape == (B,)
        del energies, minima, opt                               # (their destroy and free calls come before the next clear)
    with pytest.raises(AssertionError, match="optimizer must be"):
        pt.quench(optimizer="bfgs")


def test_quench_to_rest_hands_over_to_fresh_handles(fake):
    """Two handles: the first leaves every instance stuck after 7 steps, the second does not lower any energy, so all are at
    rest.  Never a done flag, so the chunks are 10, 10, 5 of 25 and then 10, 8 of the 18 that are left."""
    read = "dzo_lbfgs_batch_read"
    fake.fill = {(read, dzo.LBFGS_BATCH_OBJECTIVES): np.array([-1.0, -2.0, -3.0]), (read, dzo.LBFGS_BATCH_IS_STUCK): np.ones(B, np.int32),
                 (read, dzo.LBFGS_BATCH_ITERATION_COUNTS): np.array([7, 3, 5], np.int64)}
    fake.i64 = 5
    at_rest = dzo.quench_to_rest(points(), N, 6, 0.02, steps_per_launch=10, max_steps=25)
    assert at_rest.tolist() == [True] * B
    creates, destroys = fake.named("dzo_lbfgs_batch_create"), fake.named("dzo_lbfgs_batch_destroy")
    assert creates == [(0, N, B, F64, 0x1000, 0.02, 6, BVP)] * 2 and destroys == [(0x5000,), (0x5010,)]
    assert fake.named("dzo_lbfgs_batch_step") == [(0x5000, 10, B32), (0x5000, 10, B32), (0x5000, 5, B32), (0x5010, 10, B32), (0x5010, 8, B32)]
    order = [name.rsplit("_", 1)[-1] for name, _ in fake.calls]
    assert order == ["create", "active", "step", "step", "step", "read", "read", "read", "destroy",
                     "create", "active", "step", "step", "read", "read", "read", "destroy"]
    fake.calls.clear()
    fake.i64 = 0                                                # nobody active: no step, and one step is counted per handle
    fake.fill[read, dzo.LBFGS_BATCH_ITERATION_COUNTS] = np.zeros(B, np.int64)
    assert dzo.quench_to_rest(points(), N, max_steps=1).tolist() == [False] * B
    assert len(fake.named("dzo_lbfgs_batch_create")) == 1 == len(fake.named("dzo_lbfgs_batch_destroy")) and not fake.named("dzo_lbfgs_batch_step")


# ------------------------------------------------------------------------------ read, ptr, _set
WHATS = {make_tempering: "TEMPERING_", make_lbfgs: "LBFGS_BATCH_", make_adgd: "ADGD_BATCH_", make_basin: "BASIN_HOPPING_",
         make_modefollow: "MODEFOLLOW_", make_hybridef: "HYBRIDEF_"}
NOT_WHAT = ("MAX_PARTICLES", "MAX_HISTORY", "ACTIVE", "CONVERGED", "FAILED")


@pytest.mark.parametrize("make", list(WHATS))
def test_read_and_ptr_of_every_array(fake, make):
    obj, _, _, prefix = make()
    h = obj.h.value
    if hasattr(obj, "set_record"):
        obj.set_record(4)
    whats = sorted(v for k, v in vars(dzo).items() if k.startswith(WHATS[make]) and not k.endswith(NOT_WHAT))
    assert whats == list(range(len(whats))) and len(whats) >= 11
    for what in whats:
        shape, dtype = obj._shape(what)
        assert int(np.prod(shape)) > 0
        fake.calls.clear()
        out = obj.read(what)
        address = obj.ptr(what)
        assert (out.shape, out.dtype) == (shape, np.dtype(dtype)) and out.flags.c_contiguous
        assert address == fake.next_handle - 0x10
        assert fake.calls == [(prefix + "read", (h, what, out.ctypes.data)), (prefix + "get_ptr", (h, what, BVP))]
    with pytest.raises(KeyError):
        obj.read(len(whats))
    fake.calls.clear()
    fake.rc[prefix + "read"] = 1
    with pytest.raises(dzo.DzoError, match="invalid argument.*x"):
        obj.read(0)
    assert [name for name, _ in fake.calls] == [prefix + "read", "dzo_last_error"]


def test_properties_read_the_array_they_name(fake):
    lb, ad, bh, pt = make_lbfgs()[0], make_adgd()[0], make_basin()[0], make_tempering()[0]
    fake.fill = {("dzo_lbfgs_batch_read", dzo.LBFGS_BATCH_IS_STUCK): np.array([1, 0, 2], np.int32)}
    fake.calls.clear()
    assert lb.is_stuck.tolist() == [True, False, True] and lb.is_stuck.dtype == bool
    assert ad.current_step_sizes.shape == (B,) and lb.step_directions.shape == (B, 3 * N) and lb.last_halvings.dtype == np.int32
    assert bh.best_energies.shape == (B,) and pt.coordinates.shape == (B, 3, N) and pt.rng_states.dtype == np.uint64
    assert [(name, args[1]) for name, args in fake.calls] == [
        ("dzo_lbfgs_batch_read", dzo.LBFGS_BATCH_IS_STUCK), ("dzo_lbfgs_batch_read", dzo.LBFGS_BATCH_IS_STUCK),
        ("dzo_adgd_batch_read", dzo.ADGD_BATCH_CURRENT_STEP_SIZES), ("dzo_lbfgs_batch_read", dzo.LBFGS_BATCH_DIRECTIONS),
        ("dzo_lbfgs_batch_read", dzo.LBFGS_BATCH_LAST_HALVINGS), ("dzo_basin_hopping_read", dzo.BASIN_HOPPING_BEST_ENERGIES),
        ("dzo_tempering_read", dzo.TEMPERING_REPLICAS), ("dzo_tempering_read", dzo.TEMPERING_RNG_STATES)]


@pytest.mark.parametrize("make, radii, states", [(make_tempering, "TEMPERING_RADII", "TEMPERING_RNG_STATES"),
                                                 (make_basin, "BASIN_HOPPING_RADII", "BASIN_HOPPING_RNG_STATES")])
def test_set_sends_the_values_in_the_array_s_own_type(fake, make, radii, states):
    obj, _, _, prefix = make()
    h = obj.h.value
    fake.calls.clear()
    fake.peek[prefix + "set"] = 8 * B
    obj.perturbation_radii = [1, 2, 3]                          # integers: converted to the element type
    obj.rng_states = np.array([7, 8, MASK], dtype=np.uint64)
    obj._set(getattr(dzo, radii), np.array([0.5, 0.25, 0.125]))
    assert fake.calls == [(prefix + "set", (h, getattr(dzo, radii), np.array([1.0, 2.0, 3.0]).tobytes())),
                          (prefix + "set", (h, getattr(dzo, states), np.array([7, 8, MASK], np.uint64).tobytes())),
                          (prefix + "set", (h, getattr(dzo, radii), np.array([0.5, 0.25, 0.125]).tobytes()))]
    with pytest.raises(AssertionError):
        obj.perturbation_radii = [1.0, 2.0]
    assert len(fake.calls) == 3


# ------------------------------------------------------------------------------ the free functions that adopt ``points``
def test_free_functions_pass_particles_and_batch(fake):
    pts, n3 = points(), 3 * N
    assert dzo.pairwise_batch_energy_gradient(pts, N, dev(n3 * B, 0x1200)).shape == (B,)
    assert dzo.pairwise_batch_hessian(pts, N).shape == (B, n3, n3)
    dzo.pairwise_batch_hvp(pts, dev(n3 * B, 0x1300), N, products=dev(n3 * B, 0x1400))
    dzo.pairwise_batch_hvp(dev(n3, 0x1000), dev(n3 * B, 0x1300), N, products=dev(n3 * B, 0x1400), shared_point=True)
    fp, _ = dzo.structure_fingerprints(pts, N)
    assert fp.shape == (B, 2 * N)
    dzo.lowest_modes(pts, N, seed=-4)
    dzo.modefollow_apply(pts, dev((B, n3), 0x1500), dev((B, n3, n3), 0x1600), N)
    dzo.hybridef_apply(pts, dev(B, 0x1500), dev((B, n3), 0x1600), N)
    head = {name: args[:5] for name, args in fake.calls if "batch" in name}
    for name in ("dzo_pairwise_batch_energy_gradient", "dzo_pairwise_batch_hessian", "dzo_structure_batch_fingerprint",
                 "dzo_pairwise_batch_lowest_mode", "dzo_modefollow_batch_apply", "dzo_hybridef_batch_apply"):
        assert head[name] == (0, N, B, F64, 0x1000), name
    assert [args[:7] for args in fake.named("dzo_pairwise_batch_hvp")] == [(0, N, B, F64, 0x1000, n3, 0x1300), (0, N, B, F64, 0x1000, 0, 0x1300)]
    assert fake.named("dzo_pairwise_batch_energy_gradient")[0][6] == 0x1200
    assert fake.named("dzo_pairwise_batch_lowest_mode")[0][5:10] == (1, 32, 40, 4.3e-15, MASK - 3)
    odd = dev(n3 * B + 1, 0x1000)
    for call in (lambda: dzo.pairwise_batch_energy_gradient(odd, N), lambda: dzo.pairwise_batch_hessian(odd, N),
                 lambda: dzo.pairwise_batch_hvp(pts, odd, N), lambda: dzo.structure_fingerprints(odd, N), lambda: dzo.lowest_modes(odd, N),
                 lambda: dzo.hessian_spectrum(odd, N), lambda: dzo.modefollow_apply(odd, None, None, N),
                 lambda: dzo.hybridef_apply(odd, None, None, N), lambda: dzo.connect_saddles(odd, odd, N, 0.1, 1e-4)):
        with pytest.raises(AssertionError, match="must hold 3 \\* n_particles \\* batch elements"):
            call()
    for call in (lambda: dzo.pairwise_batch_hessian(pts, 0), lambda: dzo.structure_fingerprints(pts, 0), lambda: dzo.lowest_modes(pts, -1),
                 lambda: dzo.hessian_spectrum(pts, 0), lambda: dzo.connect_saddles(pts, pts, 0, 0.1, 1e-4)):
        with pytest.raises(AssertionError, match="must hold 3 \\* n_particles \\* batch elements"):
            call()
    with pytest.raises((AssertionError, ZeroDivisionError)):
        dzo.pairwise_batch_energy_gradient(pts, 0)


# ------------------------------------------------------------------------------ teardown
@pytest.mark.parametrize("make", MAKERS)
def test_close_destroys_once(fake, make):
    obj, keep, _, prefix = make()
    h = obj.h.value
    fake.calls.clear()
    obj.close()
    assert fake.calls == [(prefix + "destroy", (h,))] and not obj.h
    obj.close()
    del obj
    assert fake.calls == [(prefix + "destroy", (h,))]


@pytest.mark.parametrize("make", MAKERS)
def test_del_destroys_once(fake, make):
    obj, keep, _, prefix = make()
    h = obj.h.value
    fake.calls.clear()
    del obj
    assert fake.calls == [(prefix + "destroy", (h,))]


@pytest.mark.parametrize("make", MAKERS)
def test_del_after_the_library_is_gone_does_nothing(fake, make, monkeypatch):
    obj, keep, _, _ = make()
    fake.calls.clear()
    monkeypatch.setattr(dzo, "_lib", None)
    del obj
    assert fake.calls == []
    monkeypatch.setattr(dzo, "_lib", object())                  # ``keep`` goes to the recorder


@pytest.mark.parametrize("make", [m for m in MAKERS if m is not make_comm])
def test_failed_constructor_is_deleted_quietly(fake, make, capsys):
    create = make()[2]
    gc.collect()
    fake.calls.clear()
    fake.rc[create] = 1
    with pytest.raises(dzo.DzoError, match="dzo error 1 \\(invalid argument\\): x") as e:
        make()
    del e
    gc.collect()
    names = [name for name, _ in fake.calls]
    at = names.index(create)
    assert names[at + 1] == "dzo_last_error"
    # nothing is destroyed but the problem that a single-instance optimizer was to be built from
    assert names[at + 2:] == ["dzo_problem_destroy"] * names[:at].count("dzo_problem_create")
    assert capsys.readouterr().err == ""                        # nothing "ignored in __del__"
