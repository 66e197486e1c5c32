"""csrc/dzo_lbfgs_plan.h on the CPU: tools/lbfgs_plan_table.cpp, built with -Wall -Werror and the address and undefined-behaviour
sanitizers and run as a process of its own, answers a grid of queries; every field is compared with tests/lbfgs_plan_twin.py, which
restates the decisions from the code the header replaced.  The grid holds what no GPU test can allocate: the sizes on either side of
the 2^32 byte-offset limits.  Then the properties of the plans themselves, and the table of DESIGN.md against the program's output."""
import functools
import itertools
import os
import re
import subprocess

import pytest

import lbfgs_plan_twin as tw
from test_tuning_knobs import FOLDED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "lbfgs_plan_table.cpp")
BEGIN, END = "<!-- lbfgs-plan-table:begin -->", "<!-- lbfgs-plan-table:end -->"
DTYPES = [tw.F64, tw.F32]
KINDS = [tw.NO_PROBLEM, tw.ROSENBROCK_CHAIN, tw.QUADRATIC_CHAIN, tw.LSE, tw.QUADRATIC]
MS = list(range(1, 27)) + [64]
LAYOUT_FIELDS = ["stride", "blocked", "points", "ring_obj", "nslots", "ring_rows", "tile_stride", "rowbytes", "ring_bytes", "pair_stride",
                 "slab_bytes", "lin_bytes", "d_bytes", "d_offset", "gram_grid", "point_sets", "scalar_total"]
FACTS = ["points", "single_pass", "blocked", "mode", "line_search", "descent_check", "sd_fallback", "speculate", "fused_post", "callbacks",
         "box_on", "has_problem", "iteration_count", "n", "k", "m", "dtype", "ring_obj", "ring_decorated", "obj_agrees", "dec_agrees",
         "lambda_agrees", "lse_c_agrees", "spec_scalars", "d_al16"]


def last_n_where(cond):
    """The largest n for which the monotone condition holds (bisection)."""
    lo, hi = 1, 1 << 40
    assert cond(lo) and not cond(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if cond(mid) else (lo, mid)
    return lo


def stream_major_fits(n, es, ms):
    """2 ms stream_bytes + 2^20 < 2^32, stream_bytes = the rows' KiB made odd (one KiB per row of 62 vectors of 16 bytes)."""
    vecn = 16 // es
    rows = ((n + vecn - 1) // vecn + 61) // 62
    return 2 * ms * ((rows | 1) * 1024) + (1 << 20) < (1 << 32)


def n_values(dtype):
    es = tw.es_of(dtype)
    ns = [1, 7, 8, 9, 15, 16, 17, 123, 124, 125, 4099, 4100, 10 ** 7, (1 << 32) // es - 1, (1 << 32) // es]
    for m in (9, 24):
        for extra in (0, 1):                      # the centre vector's slot of the log-sum-exp ring
            last = last_n_where(lambda n: stream_major_fits(n, es, m + 2 + extra))
            ns += [last, last + 1]
    return sorted(set(ns))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "lbfgs_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])

    def ask(queries):
        path = exe + ".queries"
        with open(path, "w") as f:
            f.write("\n".join(queries) + "\n")
        out = subprocess.run([exe, path], capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
        lines = out.stdout.splitlines()
        assert len(lines) == len(queries)
        return [[int(v) for v in ln.split()[1:]] for ln in lines]
    ask.exe = exe
    return ask


def layout_cases():
    """(n, dtype, m, kind, (l2, box gradient, box constraint), (x, g, c aligned), knob, value)."""
    cases = []
    aligned = (1, 1, 1)
    for dtype in DTYPES:
        ns = n_values(dtype)
        for n, m, kind in itertools.product(ns, MS, KINDS):
            for dec in itertools.product((0, 1), repeat=3):                       # every decorator on and off
                cases.append((n, dtype, m, kind, dec, aligned, "-", 0))
            for al in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):                          # x, g, c off 16 bytes in turn
                cases.append((n, dtype, m, kind, (0, 0, 0), al, "-", 0))
        for knob, dflt in tw.KNOB_DEFAULTS.items():                               # each construction knob flipped singly
            flips = [0, 1] if dflt is None else [{0: 1, 1: 0}.get(dflt, dflt * 2)]
            for v, n, m, kind in itertools.product(flips, ns, (1, 8, 9, 12, 13, 20, 21, 24, 25, 64), (tw.ROSENBROCK_CHAIN, tw.LSE)):
                cases.append((n, dtype, m, kind, (0, 0, 0), aligned, knob, v))
    return cases


@functools.lru_cache(maxsize=None)
def twin_layout(n, dtype, m, kind, decorated, al, knob, v):
    """(the twin looks at whether ANY decorator is on: one answer serves the eight combinations the driver is asked about)"""
    return tw.layout(n, dtype, m, kind, decorated, *al, cus=256, knobs={} if knob == "-" else {knob: v})


def test_layout_matches_the_twin_over_the_whole_range(driver):
    cases = layout_cases()
    answers = driver(["L %d %d %d %d %g %d %d %d %d %d 256 %s %d" % (n, dtype, m, kind, 0.5 * dec[0], dec[1], dec[2], *al, knob, v)
                      for n, dtype, m, kind, dec, al, knob, v in cases])
    seen = set()
    for case, got in zip(cases, answers):
        n, dtype, m, kind, dec, al, knob, v = case
        L = twin_layout(n, dtype, m, kind, any(dec), al, knob, v)
        want = [int(L[name]) for name in LAYOUT_FIELDS]
        assert got[:len(want)] == want, (case, [(name, g, w) for name, g, w in zip(LAYOUT_FIELDS, got, want) if g != w])
        offsets = got[len(LAYOUT_FIELDS):]
        assert len(offsets) == len(tw.SCALARS) + 1                                # ... and the slack behind them
        # the parent's sub-arrays at the parent's offsets, in the parent's order, disjoint, and summing to the total
        assert offsets[:-1] == [L["scalar_offsets"][s] for s in tw.SCALARS], case
        assert offsets[0] == 0 and all(a < b for a, b in zip(offsets, offsets[1:])), case
        assert offsets[-1] - offsets[-2] == L["link_partials_len"], case
        assert L["scalar_total"] - offsets[-1] == tw.K_MAX_HISTORY, case         # the slack: what the parent allocated and never carved
        seen.add((tw.ring_layout(L["blocked"], L["points"]), tw.tile_arrangement(L)))
        if L["blocked"]:
            # the last tile of the last row of the last stream ends inside the ring, and a stream-major ring fits 32-bit byte offsets
            streams = 2 * (L["nslots"] + (1 if L["ring_obj"] == 2 else 0))
            assert (streams - 1) * L["tile_stride"] + (L["ring_rows"] - 1) * L["rowbytes"] + tw.K_TILE_BYTES <= L["ring_bytes"], case
            assert tw.tile_arrangement(L) == 1 or L["ring_bytes"] + (1 << 20) < (1 << 32), case
    assert seen == {(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)}                       # the grid reaches every layout and arrangement


def test_limits_sit_where_the_grid_says():
    """The grid's boundary sizes really are boundaries (of the twin; the driver agrees with it above)."""
    for dtype in DTYPES:
        es = tw.es_of(dtype)
        below, at = tw.layout((1 << 32) // es - 1, dtype, 5, tw.ROSENBROCK_CHAIN), tw.layout((1 << 32) // es, dtype, 5, tw.ROSENBROCK_CHAIN)
        assert below["blocked"] and not at["blocked"]
        for m in (9, 24):
            if m > tw.point_max_k(dtype):
                continue
            last = last_n_where(lambda n: stream_major_fits(n, es, m + 2))
            a, b = tw.layout(last, dtype, m, tw.ROSENBROCK_CHAIN), tw.layout(last + 1, dtype, m, tw.ROSENBROCK_CHAIN)
            assert (tw.tile_arrangement(a), tw.tile_arrangement(b)) == (2, 1), (dtype, m, last)


def test_kernel_variants_hold_m_pairs_and_are_the_smallest_offered(driver):
    cases = [(m, dtype, sets, dec, obj, first) for m in MS for dtype in DTYPES for sets in (1, 2) for dec in (0, 1) for obj in (0, 1)
             for first in (0, 1)]
    for case, got in zip(cases, driver(["V %d %d %d %d %d %d" % c for c in cases])):
        m, dtype, sets, dec, obj, first = case
        K, SETS, DEC, OBJ, FIRST = tw.point_pass_variant(m, dtype, sets, dec, obj, first)
        assert got == [int(tw.point_one_set(m, dtype, sets)), K, SETS, int(DEC), OBJ, int(FIRST), tw.pair_pass_k(m), tw.lse_dots_k(m, dtype)], case
        if m <= tw.point_max_k(dtype) and not first:
            offered = tw.POINT_PASS_OFFERED[dtype][(SETS, DEC, OBJ)]
            assert K >= m and K == min(k for k in offered if k >= m), (case, K)
            assert SETS == 2 or K <= (20 if dtype == tw.F64 else 12)               # one register set: where it fits 256 registers
        if m <= tw.K_PAIR_MAX_K:
            assert got[6] >= m and got[6] == min(k for k in (8, 16, 20) if k >= m)
        if m <= tw.point_max_k(dtype):
            assert got[7] >= m and got[7] == min(k for k in ((8, 12, 20, 24) if dtype == tw.F64 else (8, 12, 20)) if k >= m)


def test_launch_shape_respects_the_lds_budget(driver):
    grids = ((256, 2048), (512, 2048), (1 << 20, 2048), (512, 3), (0, 1))          # (resident blocks, gram_grid): the grid bound alone
    cases = [(n, dtype, m, k, sets, regrad, rows, prio, mb, nrows) + grids[i % len(grids)]
             for i, ((n, nrows), dtype, m, sets, regrad, rows, prio, mb) in enumerate(itertools.product(
                 ((124, 1), (10 ** 7, 80646), (3 * 10 ** 8, 2419355)), DTYPES, (1, 8, 12, 13, 20, 21, 24), (1, 2), (0, 1),
                 (-3, 0, 1, 9, 16, 18, 36, 1000), (0, 1), (0, 200)))
             for k in (0, 1, m)]
    for case, got in zip(cases, driver(["P %d %d %d %d %d %d %d %d %d %d %d %d" % c for c in cases])):
        n, dtype, m, k, sets, regrad, rows, prio, mb, nrows, res, gg = case
        P = tw.point_launch(n, dtype, m, k, sets, regrad, rows, prio, mb)
        assert got[:9] == [int(P["one_set"]), P["stage_tiles"], P["stage_max"], P["stage_rows"], P["stage_bytes"], P["nt_tiles"], P["prio"],
                           P["small_rows"], P["small_bytes"]], case
        assert got[9:] == [tw.pass_grid(nrows, res, gg, 1024), tw.pass_grid(nrows, res, gg, 2048)], case
        # the budget the shape was derived from: of the 160 KiB of LDS of a CU, 144 KiB staged by the one resident block with two
        # register sets per wave, 72 KiB by each of the two with one (the rest: the kernel's static arrays, 8 KiB a block at the
        # most); without the attribute, the default 64 KiB
        blocks_per_cu = 2 if got[0] else 1
        assert 1 <= got[3] and got[4] <= (72 if got[0] else 144) * 1024 and blocks_per_cu * (got[4] + 8 * 1024) <= 160 * 1024, case
        assert got[8] + 8 * 1024 <= 64 * 1024, case
        assert 1 <= got[9] <= 1024 and got[9] <= got[10] <= 2048, case


def test_step_path_matches_the_twin(driver):
    base = dict(points=1, single_pass=1, blocked=1, mode=1, line_search=0, descent_check=0, sd_fallback=0, speculate=1, fused_post=1, callbacks=0,
                box_on=0, has_problem=1, iteration_count=3, n=4100, k=3, m=5, dtype=tw.F64, ring_obj=0, ring_decorated=0, obj_agrees=1,
                dec_agrees=1, lambda_agrees=1, lse_c_agrees=1, spec_scalars=1, d_al16=1)
    cases = []
    for dtype, obj, dec in itertools.product(DTYPES, (0, 1, 2), (0, 1)):
        start = dict(base, dtype=dtype, ring_obj=obj, ring_decorated=dec)
        cases.append(start)
        for name in FACTS:                                                        # every fact moved singly ...
            if name in ("n", "k", "m", "dtype", "iteration_count", "ring_obj", "ring_decorated"):
                continue
            cases.append(dict(start, **{name: 1 - start[name]}))
        for k, m in itertools.product((0, 1, 19, 20, 21, 24, 25), (1, 20, 21, 24, 25, 64)):      # ... and the sizes
            for it, spec in ((0, 0), (0, 1), (7, 0), (7, 1)):
                cases.append(dict(start, k=k, m=m, iteration_count=it, spec_scalars=spec))
        es = tw.es_of(dtype)
        for n in (1, 4 * (16 // es) - 1, 4 * (16 // es), (1 << 32) // es - 1, (1 << 32) // es):
            cases.append(dict(start, n=n))
            cases.append(dict(start, n=n, points=0))
    answers = driver(["S " + " ".join(str(int(c[name])) for name in FACTS) for c in cases])
    seen = set()
    for c, got in zip(cases, answers):
        assert got == [int(tw.points_ok(c)), int(tw.single_pass_ok(c))], c
        seen.add(tuple(got))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_constants(driver):
    assert driver(["C"])[0] == [tw.K_WAVES, tw.K_MAX_HISTORY, tw.K_MAX_PARTIAL_BLOCKS, tw.K_GRAM_VALUES, tw.K_ROW_OWN, tw.K_ROW_LEAD,
                                tw.K_TILE_BYTES, tw.K_PAIR_MAX_K, tw.K_FUSED_MAX_K, tw.point_max_k(tw.F64), tw.point_max_k(tw.F32)]


def test_design_holds_the_programs_table(driver):
    table = subprocess.run([driver.exe], capture_output=True, text=True, check=True).stdout
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.count(BEGIN) == 1 and design.count(END) == 1
    section = design[design.index(BEGIN) + len(BEGIN):design.index(END)]
    assert section.strip() == table.strip(), "DESIGN.md: regenerate the table between the markers with tools/lbfgs_plan_table.cpp"


def test_reading_test_of_the_translation_unit():
    """The decisions left the translation unit: no thread-local hand-over, no ALLOC macro, the construction-time knobs read in
    one function, every instantiation of the point pass named once, and the plan header free of HIP."""
    src = open(os.path.join(ROOT, "dzoptimization.jl_amd", "csrc", "dzo_lbfgs.hip")).read()
    assert "thread_local" not in src and "#define ALLOC" not in src
    knobs = [k for k in tw.KNOB_DEFAULTS]
    reader = src[src.index("static LbfgsKnobs lbfgs_read_knobs()"):]
    reader = reader[:reader.index("\n}\n")]
    for k in knobs:
        name = '"DZO_TUNE_%s"' % k
        assert src.count(name) == reader.count(name) >= 1, k
    # the knobs folded into their defaults (tests/test_tuning_knobs.py keeps the list), and the state only they reached
    gone = [k for k in FOLDED if not k.startswith("ADGD_")]
    assert len(gone) >= 18 and not [k for k in gone if re.search(r"DZO_TUNE_%s(?![A-Z0-9_])" % k, src)]
    assert not [word for word in ("gram_variant", "interleaved", "lazy_d", "combine_nts") if word in src]
    code ="\n".join(line.split("//")[0] for line in src.splitlines())           # (comments may speak of an instantiation)
    assert code.count("lbfgs_point_pass_kernel<") == 1
    plan = open(os.path.join(ROOT, "dzoptimization.jl_amd", "csrc", "dzo_lbfgs_plan.h")).read()
    assert "#include <hip" not in plan and "__device__" not in plan and "__global__" not in plan


def test_point_pass_table_is_the_set_of_variants():
    """point_pass_kernel_of names each instantiation once, and its list for an element type is exactly what point_pass_variant can
    ask for there (m up to point_max_k; both values of DZO_TUNE_POINT_SETS): no variant without a kernel, no kernel without a use."""
    src = open(os.path.join(ROOT, "dzoptimization.jl_amd", "csrc", "dzo_lbfgs.hip")).read()
    body = src[src.index("static void (*point_pass_kernel_of(PassVariant v))"):]
    body = body[:body.index("#undef DZO_PP")]
    lists = dict(zip((tw.F64, tw.F32), body[body.index("if constexpr (sizeof(T) == 8)"):].split("} else {")))
    assert len(lists) == 2
    for dtype, text in lists.items():
        named = [(int(K), int(SETS), DEC == "true", int(OBJ), FIRST == "true")
                 for K, FIRST, SETS, DEC, OBJ in re.findall(r"DZO_PP\((\d+), (true|false), (\d+), (true|false), (\d+)\)", text)]
        assert len(named) == text.count("DZO_PP(") and len(set(named)) == len(named), dtype
        asked = {tw.point_pass_variant(m, dtype, sets, dec, obj, first) for m in range(1, tw.point_max_k(dtype) + 1) for sets in (1, 2)
                 for dec in (False, True) for obj in (0, 1) for first in (False, True)}
        assert set(named) == asked, (dtype, sorted(set(named) ^ asked))
