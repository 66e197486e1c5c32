"""What real handles decide, against tests/lbfgs_plan_twin.py, at the smallest shapes at which a decision can go wrong: n below
four vectors (slabs), exactly four, ragged (a tile ring of points only), exactly one wave-row of 62 vectors and one element more,
in both element types; history lengths on either side of every threshold (9: the stream-major default begins; 12 / 13: the fp32
limit of one register set; 20 / 21 and 24 / 25: the limits of the pass).  Every case builds an LBFGSOptimizer through a Problem and
checks ring_layout, tile_arrangement and pass_register_sets; after three steps single_pass_steps, iteration_count and the layout
again; then an option the passes do not serve (a Wolfe search for even m, CHAIN mode for odd m) and one more step: the layout the
ring falls back to -- the slabs for a ragged n.  Only the public Python API is used."""
import numpy as np
import pytest

import lbfgs_plan_twin as tw
from dzo_loader import dzo

gpu = pytest.mark.gpu
NS = {np.float64: [7, 8, 9, 124, 125], np.float32: [15, 16, 17, 248, 249]}
MS = [1, 8, 9, 12, 13, 20, 21, 24, 25]
DECOR = dict(l2=0.01, box_constraint=(-2.0, 2.0))
OBJECTIVES = {  # name -> (kind of the twin, decorated, centre vector aligned)
    "rosen": (tw.ROSENBROCK_CHAIN, False, True), "quad": (tw.QUADRATIC_CHAIN, False, True), "lse": (tw.LSE, False, True),
    "lse-c-off": (tw.LSE, False, False), "rosen-dec": (tw.ROSENBROCK_CHAIN, True, True), "quad-dec": (tw.QUADRATIC_CHAIN, True, True),
    "lse-dec": (tw.LSE, True, True),
}
KIND = {tw.ROSENBROCK_CHAIN: "ROSENBROCK_CHAIN", tw.QUADRATIC_CHAIN: "QUADRATIC_CHAIN", tw.LSE: "LSE"}


@pytest.fixture(scope="module")
def device():
    dzo.init(0)


def start_point(n, dtype):
    i = np.arange(n)
    return (0.5 * np.cos(0.7 * i) - 0.3).astype(dtype)


def make_problem(name, n, dtype):
    kind, decorated, c_aligned = OBJECTIVES[name]
    kw = dict(DECOR) if decorated else {}
    keep = None                                   # (the buffer a misaligned centre vector is a view of)
    if kind == tw.LSE:
        c = (0.25 * np.sin(np.arange(n))).astype(dtype)
        if c_aligned:
            kw.update(c=dzo.DeviceArray.from_host(c), lam=1.0)
        else:
            keep = dzo.DeviceArray.from_host(np.concatenate([c[:1], c]))
            kw.update(c=keep.view(1, n), lam=1.0)       # one element off the allocation: 8 or 4 bytes off a 16-byte boundary
    elif kind == tw.QUADRATIC_CHAIN:
        kw.update(lam=0.5)
    return dzo.Problem(getattr(dzo, KIND[kind]), n, dtype, **kw), keep


def reported(opt):
    return opt.ring_layout, opt.tile_arrangement, opt.pass_register_sets


def predicted(L, m, dtype_code):
    return tw.ring_layout(L["blocked"], L["points"]), tw.tile_arrangement(L), tw.pass_register_sets(L, m, dtype_code)


@gpu
@pytest.mark.parametrize("name", list(OBJECTIVES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_handles_decide_what_the_twin_predicts(device, dtype, name):
    kind, decorated, c_aligned = OBJECTIVES[name]
    code = tw.F64 if dtype == np.float64 else tw.F32
    layouts = set()
    for n in NS[dtype]:
        for m in MS:
            what = (name, np.dtype(dtype).name, n, m)
            prob, keep = make_problem(name, n, dtype)
            x = dzo.DeviceArray.from_host(start_point(n, dtype))
            opt = dzo.LBFGSOptimizer(None, prob, None, x, 0.05, m)
            L = tw.layout(n, code, m, kind, decorated, True, True, c_aligned)
            assert reported(opt) == predicted(L, m, code), what
            for _ in range(3):
                opt.step()
            assert not opt.is_stuck and opt.iteration_count == 3, what
            assert opt.single_pass_steps == (3 if L["points"] else 0), what     # every step of a point ring is one pass per trial
            assert reported(opt) == predicted(L, m, code), what
            chain = m % 2 == 1
            if chain:
                opt.set_two_loop_mode(dzo.TWOLOOP_CHAIN)
            else:
                opt.set_line_search(dzo.LINE_SEARCH_WOLFE)
            opt.step()
            after = tw.layout_after_leaving_points(L, n, code, chain)
            assert opt.ring_layout == after and opt.tile_arrangement == (tw.tile_arrangement(L) if after else 0), what
            assert opt.pass_register_sets == 0 and opt.single_pass_steps == (3 if L["points"] else 0), what     # (no pass since)
            layouts.add((predicted(L, m, code)[0], after))
            del opt, prob, keep
    # the shapes reach what they were chosen for
    want = {"rosen": {(0, 0), (2, 0), (2, 1)}, "quad": {(0, 0), (2, 0), (2, 1)}, "lse": {(0, 0), (2, 0), (2, 1)}, "rosen-dec": {(0, 0), (2, 0), (2, 1)}}
    assert layouts == want.get(name, {(0, 0)}), (name, layouts)


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_create_without_a_problem_and_with_callbacks_is_never_blocked(device, dtype):
    """dzo_lbfgs_create called directly (the full constructor with f0 and g0) and the callback constructor: slabs, whatever the shape."""
    for n in NS[dtype]:
        for m in MS:
            prob = dzo.Problem(dzo.ROSENBROCK_CHAIN, n, dtype)
            x = dzo.DeviceArray.from_host(start_point(n, dtype))
            g0 = prob.gradient_(dzo.DeviceArray.zeros(n, dtype), x)
            direct = dzo.LBFGSOptimizer(None, prob, None, x, prob(x), g0, 0.05, m)
            x2 = dzo.DeviceArray.from_host(start_point(n, dtype))
            callbacks = dzo.LBFGSOptimizer(None, prob.native_callbacks(), None, x2, 0.05, m)
            L = tw.layout(n, tw.F64 if dtype == np.float64 else tw.F32, m)
            assert not L["blocked"]
            for opt in (direct, callbacks):
                assert reported(opt) == (0, 0, 0), (n, m)
                for _ in range(3):
                    opt.step()
                assert reported(opt) == (0, 0, 0) and opt.single_pass_steps == 0 and opt.iteration_count == 3, (n, m)
            del direct, callbacks
