"""What ``assign_particles``, ``align_pairs`` and ``connect_minima`` send to the C ABI, call by call (CPU only, no library, no
device): the recorder of tests/test_handles.py stands in for ``dzo.lib``."""
import inspect

import numpy as np
import pytest

from dzo_loader import dzo
from test_handles import Recorder, dev, fake  # noqa: F401  (``fake`` is the fixture)

N, B = 5, 3
A_PTR, B_PTR = 0x1000, 0x2000


def _pair(dtype=np.float64):
    return dev(3 * N * B, A_PTR, dtype), dev((B, 3 * N), B_PTR, dtype)


def _allocations(fake):
    """the made-up addresses dzo_malloc handed out, in order"""
    return [0x5000 + 0x10 * k for k in range(len(fake.named("dzo_malloc")))]


def test_assign_particles_sends_what_the_header_declares(fake):
    a, b = _pair(np.float32)
    perm, cost = dzo.assign_particles(a, b, N)
    (args,) = fake.named("dzo_align_batch_assign")
    perm_ptr, cost_ptr = _allocations(fake)
    assert args == (N, B, dzo.F32, A_PTR, B_PTR, perm_ptr, cost_ptr)
    assert perm.shape == (B, N) and perm.dtype == np.int32 and cost.shape == (B,) and cost.dtype == np.float64
    assert [c[1][2] for c in fake.calls if c[0] == "dzo_memcpy_d2h"] == [4 * N * B, 8 * B]


def test_align_pairs_sends_what_the_header_declares(fake):
    a, b = _pair()
    r = dzo.align_pairs(a, b, N)
    (args,) = fake.named("dzo_align_batch_pairs")
    aligned, perm, rot, dist, best, cycles, status = _allocations(fake)
    assert args == (N, B, dzo.F64, A_PTR, B_PTR, dzo.ALIGN_TRIAL_IDENTITY | dzo.ALIGN_TRIAL_PRINCIPAL, 8, 20, 0, 0, aligned, perm, rot, dist, best,
                    cycles, status, None)                    # NULL for the trial distances unless asked for
    assert len(args) == len(dzo.ABI["dzo_align_batch_pairs"]) == 18
    assert r.trial_distances is None and r.aligned.ptr == aligned and r.aligned.shape == (B, 3 * N) and r.aligned.dtype == np.float64
    assert r.permutations.shape == (B, N) and r.rotations.shape == (B, 3, 3) and r.distances.shape == (B,)
    assert r.best_trials.dtype == r.cycles.dtype == r.status.dtype == np.int32


def test_align_pairs_options_and_the_trial_distances(fake):
    a, b = _pair(np.float32)
    r = dzo.align_pairs(a, b, N, trials=dzo.ALIGN_TRIAL_PRINCIPAL, random_trials=3, max_cycles=7, allow_inversion=True, seed=-1, want_trials=True)
    (args,) = fake.named("dzo_align_batch_pairs")
    ptrs = _allocations(fake)
    assert len(ptrs) == 8
    assert args == (N, B, dzo.F32, A_PTR, B_PTR, 2, 3, 7, 1, (1 << 64) - 1) + tuple(ptrs)
    assert r.trial_distances.shape == (B, 2 * (4 + 3)) and r.aligned.dtype == np.float32
    sig = inspect.signature(dzo.align_pairs).parameters
    assert list(sig) == ["a", "b", "n_particles", "trials", "random_trials", "max_cycles", "allow_inversion", "seed", "want_trials"]
    assert [sig[k].default for k in list(sig)[3:]] == [3, 8, 20, False, 0, False]
    assert list(inspect.signature(dzo.assign_particles).parameters) == ["a", "b", "n_particles"]


def test_mis_sized_arrays_are_refused_with_the_shared_message(fake):
    a, b = _pair()
    short = dev(3 * N * (B - 1), B_PTR)
    message = "must hold 3 \\* n_particles \\* batch elements"
    for call in (lambda: dzo.align_pairs(a, short, N), lambda: dzo.assign_particles(a, short, N), lambda: dzo.align_pairs(a, b, N + 1),
                 lambda: dzo.assign_particles(short, b, N), lambda: dzo.align_pairs(dev(0, A_PTR), dev(0, B_PTR), N)):
        with pytest.raises(AssertionError, match=message):
            call()
    with pytest.raises(AssertionError, match="one element type"):
        dzo.align_pairs(a, dev(3 * N * B, B_PTR, np.float32), N)
    assert fake.named("dzo_align_batch_pairs") == [] and fake.named("dzo_align_batch_assign") == []


# the symbols connect_minima called before it had ``align``, for three bands none of which is ACTIVE (count_active says 0) and all
# of which ended FAILED (nothing to refine), in order, recorded on the commit before; dzo_free comes whenever an array is collected
PLAIN_CALLS = ["dzo_malloc", "dzo_neb_batch_interpolate", "dzo_neb_batch_create", "dzo_neb_batch_count_active", "dzo_neb_batch_read",
               "dzo_neb_batch_read", "dzo_neb_batch_read", "dzo_neb_batch_read", "dzo_neb_batch_read", "dzo_malloc", "dzo_malloc",
               "dzo_neb_batch_destroy"]


def _connect(fake, **options):
    fake.fill["dzo_neb_batch_read", dzo.NEB_STATUS] = np.full(B, dzo.NEB_FAILED, dtype=np.int32)
    a, b = _pair()
    return dzo.connect_minima(a, b, N, 4, 1e-6, **options)


def _names(fake):
    return [name for name, _ in fake.calls if name != "dzo_free"]


def test_connect_minima_without_align_makes_no_new_call(fake):
    c = _connect(fake)
    assert _names(fake) == PLAIN_CALLS
    assert fake.named("dzo_neb_batch_interpolate") == [(N, 4, B, dzo.F64, A_PTR, B_PTR, 0x5000)]
    assert not hasattr(c, "alignment")
    fake.calls.clear()
    _connect(fake, align=False)
    assert _names(fake) == PLAIN_CALLS


def test_connect_minima_with_align_interpolates_to_the_aligned_copy(fake):
    c = _connect(fake, align=True)
    names = _names(fake)
    k = names.index("dzo_align_batch_pairs")
    assert names[:k] == ["dzo_malloc"] * 7 and names[k + 1:k + 7] == ["dzo_memcpy_d2h"] * 6     # every output but the aligned points
    assert names[k + 7:] == PLAIN_CALLS
    aligned = fake.named("dzo_align_batch_pairs")[0][10]
    assert aligned == 0x5000 and c.alignment.aligned.ptr == aligned
    assert fake.named("dzo_neb_batch_interpolate")[0][4:6] == (A_PTR, aligned)
    fake.calls.clear()
    _connect(fake, align=dict(trials=dzo.ALIGN_TRIAL_PRINCIPAL, random_trials=0, max_cycles=5))
    assert fake.named("dzo_align_batch_pairs")[0][5:10] == (2, 0, 5, 0, 0)
