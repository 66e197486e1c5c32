"""CPU-side checks of the batched hybrid eigenvector-following unit (the method of tests/test_lowmode_build.py): the library
exports its entry points, the Python table and the Julia module bind them with the header's arity, the constants match the
header, the header block sits where its neighbours are and states the rule, the kernels exist for gfx950 in both launch shapes
and both element types without scratch memory or spills, the source takes its energies, gradients and sums from dzo_cluster.h and its modes from the
asynchronous path of the lowest-mode unit, and the plain-C example compiles and links against the library alone.  No compute
here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_hybridef_batch_" + s for s in ("apply", "create", "destroy", "set_directions", "step", "count_active", "get_ptr", "read")]
WHATS = ["POINTS", "GRADIENTS", "ENERGIES", "GRMS", "STATUS", "EIGENVALUES", "MODES", "MODE_RESIDUALS", "PROJECTIONS", "UPHILL_STEPS",
         "TANGENT_STEPS", "ITERATION_COUNTS", "PRODUCTS", "EVALUATIONS"]
BANNED_TITLES = ("Batched LBFGSOptimizer", "Batched AdGDOptimizer", "Batched basin hopping", "Batched Hessian-vector products and dense Hessians",
                 "Batched symmetric eigensolver", "Batched eigenvector following", "Batched lowest Hessian mode")


def _header_arity(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
    return params.count(",") + 1


def test_library_exports_the_entry_points_and_both_hosts_bind_them():
    lib = ctypes.CDLL(dzo.build())
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if not hasattr(lib, n)] == []
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    for name in SYMBOLS:
        arity = _header_arity(header, name)
        assert len(dzo.ABI[name]) == arity, name
        calls = list(re.finditer(r"ccall\(\(:%s, libdzo\), Cint,\s*\(" % name, julia))
        assert calls, name
        for m in calls:                                      # the argument-type tuple of every literal ccall
            depth, i = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(julia[i], 0)
                i += 1
            types = [t for t in re.sub(r"\{[^}]*\}", "", julia[m.end():i - 1]).split(",") if t.strip()]
            assert len(types) == arity, (name, types)
    assert len(dzo.ABI["dzo_hybridef_batch_apply"]) == 21 and len(dzo.ABI["dzo_hybridef_batch_create"]) == 18
    assert dzo.ABI["dzo_hybridef_batch_create"][16] is ctypes.c_uint64
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    for name in ("HybridModeFollowing", "hybridef_apply!", "find_saddles_hybrid", "HYBRIDEF_CONVERGED"):
        assert name in exports, name
    for name in ("HybridModeFollowing", "hybridef_apply!", "find_saddles_hybrid"):
        assert re.search(r"^function %s\(" % re.escape(name), julia, flags=re.M), name


def test_python_constants_and_signatures_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    assert dzo.HYBRIDEF_MAX_PARTICLES == value("DZO_HYBRIDEF_MAX_PARTICLES") == 1024 == dzo.LOWMODE_MAX_PARTICLES
    for k, name in enumerate(WHATS):
        assert value("DZO_HYBRIDEF_" + name) == k == getattr(dzo, "HYBRIDEF_" + name), name
    for k, name in enumerate(("ACTIVE", "CONVERGED", "FAILED")):
        assert value("DZO_HYBRIDEF_" + name) == k == getattr(dzo, "HYBRIDEF_" + name), name
    assert value("DZO_VERSION") == 100
    assert issubclass(dzo.HybridModeFollowing, dzo._HandleArrays)
    for method in ("step", "run", "count_active", "set_directions", "close"):
        assert callable(getattr(dzo.HybridModeFollowing, method)), method
    sig = inspect.signature(dzo.HybridModeFollowing.__init__).parameters
    assert list(sig)[1:4] == ["points", "n_particles", "directions"]
    defaults = dict(max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05, tangent_first=0.01, krylov=8, mode_cycles=1,
                    mode_tol=1e-3, zero_tol=1e-4, grad_tol=1e-10)
    assert {k: sig[k].default for k in defaults} == defaults and sig["directions"].default is None
    assert list(inspect.signature(dzo.find_saddles_hybrid).parameters)[:3] == ["minima", "n_particles", "kick"]
    assert inspect.signature(dzo.find_saddles_hybrid).parameters["kick"].default == 0.05
    assert list(inspect.signature(dzo.hybridef_apply).parameters)[:4] == ["points", "eigenvalues", "modes", "n_particles"]
    a = dzo.HybridModeFollowing.__new__(dzo.HybridModeFollowing)
    a.batch, a.n_particles, a.dtype = 3, 5, "float32"
    assert [a._shape(w)[0] for w in (dzo.HYBRIDEF_POINTS, dzo.HYBRIDEF_MODES, dzo.HYBRIDEF_EIGENVALUES)] == [(3, 15), (3, 15), (3,)]
    assert a._shape(dzo.HYBRIDEF_PRODUCTS)[1] is __import__("numpy").int64
    a.h = None


def test_header_block_is_in_place_and_states_the_rule():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched hybrid eigenvector following")
    end = header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("Batched lowest Hessian mode") < header.index("int32_t dzo_pairwise_batch_lowest_mode(") < start < end
    block = header[start:end]
    for banned in BANNED_TITLES:
        assert banned not in block, banned
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("Munro & Wales 1999", "DZO_HYBRIDEF_MAX_PARTICLES = 1024", "THE ORDER OF THE SUMS",
                   "with the bits of dzo_pairwise_batch_energy_gradient", "grms = sqrt((g.g)/n) in fp64",                    # 1
                   "the mode's status FAILED", "grms <= grad_tol", "the point is not moved", "frozen for all later steps",     # 2
                   "F = T(u.g)", "a = |lam|", "If a <= zero_tol, h = 0", "q = (F + F) / a", "h = q / (1 + sqrt(1 + q*q))",      # 3
                   "invariant to the sign of u", "If |h| > max_step", "h = +-T(max_step)", "x_e = fma(h, u_e, x_e)",
                   "tangent_steps iterations when lam < -zero_tol, otherwise tangent_steps_convex", "c = u.g'",                # 4
                   "p_e = T(g'_e - c u_e)", "pp = p.p", "sqrt(pp / n) <= grad_tol", "alpha = tangent_first at t = 0",
                   "s = x - x_prev", "y = p - p_prev", "alpha = (s.s) / (s.y) in fp64 if s.y > 0, else tangent_first", "Barzilai-Borwein",
                   "dn = alpha sqrt(pp)", "if dn > tangent_cap, alpha = alpha (tangent_cap / dn)", "x_e = fma(-T(alpha), p_e, x_e)",
                   "all of the point BEFORE the move", "products += the mode's products", "evaluations += 1", "iteration count += 1",   # 5
                   "No floating-point atomics", "one writer per element", "nothing loops without a bound",
                   "alone or anywhere in any batch", "one call of k steps or k calls of one",
                   "CONVERGED says only that the point is stationary", "saddle of higher index", "ALIASES points_dev",
                   "project_rigid = 1", "mode_cycles + 1 cycles", "UNFINISHED is normal", "No host wait between the two launches",
                   "Frozen instances still pass through the mode launch", "rigid projection needs 3 particles",
                   "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "DZO_ERR_NOMEM"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_hybridef_kernels_exist_for_gfx950_without_scratch():
    """Two launch shapes, two element types: no private segment, no VGPR or SGPR spill."""
    check_unit("hybridef", lj_count=4)


def test_the_source_takes_its_pieces_from_the_shared_headers():
    src = open(os.path.join(PKG, "csrc", "dzo_hybridef.hip")).read()
    for include in ('#include "dzo_chain.h"', '#include "dzo_cluster.h"'):
        assert include in src, include
    for word in ("cl_wave_eval<", "cl_block_eval<", "cl_dot3(", "cl_block_sum(", "wave_sum_all(", "cl_step(", "cl_count(", "cl_get_ptr(", "cl_read(",
                 "lm_prepare(", "lm_enqueue(", "ClCore core", 'DZO_TIMED("hybridef_mode"', 'DZO_TIMED("hybridef_step"'):
        assert word in src, word
    for word in ("atomic", "printf(", "pw_pair<", "F::"):
        assert word not in src, word
    # nothing waits between the two launches of a step or between steps
    step = src[src.index("int32_t dzo_hybridef_batch_step("):src.index("int32_t dzo_hybridef_batch_count_active(")]
    assert "Synchronize" not in step and "cl_step(" in step and step.index("lm_enqueue(") < step.index("he_launch<T, F>(")
    assert step.count("he_launch<") == 1
    chain = open(os.path.join(PKG, "csrc", "dzo_chain.h")).read()
    assert "int32_t lm_prepare(" in chain and "int32_t lm_enqueue(hipStream_t s" in chain
    lowmode = open(os.path.join(PKG, "csrc", "dzo_lowmode.hip")).read()
    assert "int32_t lm_enqueue(hipStream_t s" in lowmode and '#include "dzo_chain.h"' in lowmode
    enqueue = lowmode[lowmode.index("int32_t lm_enqueue("):lowmode.index("}  // namespace dzo", lowmode.index("int32_t lm_enqueue("))]
    assert "Synchronize" not in enqueue and "hipMalloc" not in enqueue
    assert "csrc/dzo_hybridef.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_saddle_large_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_saddle_large")
    assert {"dzo_hybridef_batch_create", "dzo_hybridef_batch_step", "dzo_hybridef_batch_read", "dzo_hybridef_batch_destroy",
            "dzo_pairwise_batch_lowest_mode", "dzo_tempering_run", "dzo_lbfgs_batch_step", "dzo_axpy"} <= wanted and wanted <= have, wanted - have
    src = open(os.path.join(ROOT, "examples", "lj_saddle_large.c")).read()
    assert int(re.search(r"atoi\(argv\[1\]\) : (\d+)", src).group(1)) > dzo.MODEFOLLOW_MAX_PARTICLES
