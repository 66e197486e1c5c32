"""CPU-side checks of the batched nudged elastic band (the method of tests/test_hybridef_build.py): the library exports its
entry points, the Python table and the Julia module bind them with the header's arity, the constants match the header, the
header block sits where its neighbours are and states the rule, the kernels exist for gfx950 in both launch shapes and both
element types without scratch memory or spills, the source takes its energies, gradients and sums from dzo_cluster.h, the residency plan is pinned at its
edges, and the plain-C example compiles and links against the library alone.  No compute here."""
import ctypes
import inspect
import os
import re

import numpy as np

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_neb_plan"] + ["dzo_neb_batch_" + s for s in ("interpolate", "apply", "create", "destroy", "step", "count_active", "get_ptr", "read")]
WHATS = ["BAND", "VELOCITIES", "FORCES", "TANGENTS", "ENERGIES", "FORCE_RMS", "RESIDUALS", "CLIMBING_IMAGES", "HIGHEST_IMAGES", "STATUS",
         "ITERATION_COUNTS"]
BANNED_TITLES = ("Batched LBFGSOptimizer", "Batched AdGDOptimizer", "Batched basin hopping", "Batched Hessian-vector products and dense Hessians",
                 "Batched symmetric eigensolver", "Batched eigenvector following", "Batched lowest Hessian mode",
                 "Batched hybrid eigenvector following", "Structure fingerprints and their classification")
LDS_MAX = 160 * 1024 - 1024                                  # the dynamic LDS the cluster units allow a launch
SMALL = 768                                                  # reduction cells, F.F and E of 32 images, the kernel's copy of its arguments


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
    assert len(dzo.ABI["dzo_neb_batch_apply"]) == 21 and len(dzo.ABI["dzo_neb_batch_create"]) == 13 and len(dzo.ABI["dzo_neb_batch_interpolate"]) == 7
    assert dzo.ABI["dzo_neb_batch_create"][11] is ctypes.c_int64
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    for name in ("ElasticBand", "interpolate_band!", "connect_minima", "neb_plan", "NEB_CONVERGED"):
        assert name in exports, name
    for name in ("ElasticBand", "interpolate_band!", "connect_minima", "neb_plan"):
        assert re.search(r"^function %s\(" % re.escape(name), julia, flags=re.M), name


def test_python_constants_and_signatures_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    assert dzo.NEB_MAX_PARTICLES == value("DZO_NEB_MAX_PARTICLES") == 1024 == dzo.HYBRIDEF_MAX_PARTICLES
    assert dzo.NEB_MAX_IMAGES == value("DZO_NEB_MAX_IMAGES") == 32
    for k, name in enumerate(WHATS):
        assert value("DZO_NEB_" + name) == k == getattr(dzo, "NEB_" + name), name
    for names in (("ACTIVE", "CONVERGED", "FAILED"), ("SHAPE_WAVE", "SHAPE_BLOCK"), ("STORAGE_LDS", "STORAGE_MEMORY")):
        for k, name in enumerate(names):
            assert value("DZO_NEB_" + name) == k == getattr(dzo, "NEB_" + name), name
    defines = set(re.findall(r"^#define[ \t]+DZO_(NEB_\w+)", header, flags=re.M))
    assert defines == {k for k in vars(dzo) if k.startswith("NEB_")} and len(defines) == 20
    assert value("DZO_VERSION") == 100
    assert issubclass(dzo.ElasticBand, dzo._HandleArrays)
    for method in ("step", "run", "count_active", "close", "read", "ptr"):
        assert callable(getattr(dzo.ElasticBand, method)), method
    sig = inspect.signature(dzo.ElasticBand.__init__).parameters
    assert list(sig)[1:4] == ["band", "n_particles", "n_images"]
    defaults = dict(spring=1.0, dt=0.02, max_move=0.1, climb=True, climb_after=50)
    assert {k: sig[k].default for k in defaults} == defaults and sig["force_tol"].default is inspect.Parameter.empty
    assert list(inspect.signature(dzo.connect_minima).parameters)[:5] == ["a", "b", "n_particles", "n_images", "force_tol"]
    assert inspect.signature(dzo.connect_minima).parameters["force_tol"].default is inspect.Parameter.empty
    assert list(inspect.signature(dzo.interpolate_band).parameters)[:4] == ["a", "b", "n_particles", "n_images"]
    assert list(inspect.signature(dzo.neb_apply).parameters)[:4] == ["band", "velocities", "n_particles", "n_images"]
    a = dzo.ElasticBand.__new__(dzo.ElasticBand)
    a.batch, a.n_particles, a.n_images, a.dtype = 3, 5, 4, "float32"
    assert [a._shape(w)[0] for w in (dzo.NEB_BAND, dzo.NEB_TANGENTS, dzo.NEB_ENERGIES, dzo.NEB_RESIDUALS)] == [(3, 4, 15), (3, 4, 15), (3, 4), (3,)]
    assert a._shape(dzo.NEB_FORCE_RMS) == ((3, 4), np.float64) and a._shape(dzo.NEB_ITERATION_COUNTS)[1] is np.int64
    assert a._shape(dzo.NEB_CLIMBING_IMAGES)[1] is np.int32
    a.h = None
    for name in ("ElasticBand", "BandConnections", "connect_minima", "interpolate_band", "neb_apply", "neb_plan"):
        assert name in dzo.__all__, name


def test_header_block_is_in_place_and_states_the_rule():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched nudged elastic band")
    end = header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("Structure fingerprints and their classification") < header.index("int32_t dzo_structure_batch_classify(") < start < end
    block = header[start:end]
    for banned in BANNED_TITLES:
        assert banned not in block, banned
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("Henkelman & Jonsson 2000", "DZO_NEB_MAX_IMAGES = 32", "DZO_NEB_MAX_PARTICLES = 1024", "THE ORDER OF THE SUMS",
                   "image m of band b sits at element 3N (M b + m)", "Images 0 and M-1 are the fixed ends",
                   "with the bits of dzo_pairwise_batch_energy_gradient", "evaluated once, at create",                                # 1
                   "d+ = x_{m+1} - x_m and d- = x_m - x_{m-1}", "If E_{m+1} > E_m > E_{m-1}: t = d+", "If E_{m+1} < E_m < E_{m-1}: t = d-",   # 2
                   "a = max(|E_{m+1} - E_m|, |E_{m-1} - E_m|)", "t_e = fma(a, d+_e, b d-_e) if E_{m+1} > E_{m-1}", "t_e = fma(b, d+_e, a d-_e)",
                   "tau_e = T(t_e / sqrt(t.t))", "c = g_m.tau (fp64)", "w = spring (sqrt(d+.d+) - sqrt(d-.d-))",                               # 3
                   "F_e = T(-(g_e - c tau_e) + w tau_e)", "F_e = T(-g_e + (c + c) tau_e)", "iteration count is >= climb_after",
                   "the first one in index order", "frms_m = sqrt((F_m.F_m) / n) in fp64", "residual = max_m frms_m",                          # 4
                   "status FAILED", "residual <= force_tol: status CONVERGED", "nothing moves", "frozen for all later iterations",
                   "p = v.F (fp64)", "If p > 0, v_e = T((p / F.F) F_e)", "else v_e = 0", "v_e = fma(T(dt), F_e, v_e)", "s_e = T(dt) v_e",       # 5
                   "If sqrt(s.s) > max_move", "s_e = T((max_move / sqrt(s.s)) s_e)", "x_e = x_e + s_e", "Iteration count += 1",
                   "as it stood at the start of that iteration",                                                                              # 6
                   "BEFORE the move", "-1 while none climbs", "No floating-point atomics", "one writer per element", "every loop is bounded",
                   "alone or anywhere in any batch", "one call of k steps or k calls of one",
                   "One 256-thread block per band", "workgroup barriers only", "no grid-wide synchronisation", "no host wait inside or between launches",
                   "dealt round-robin to the four waves", "lane i holds particle i", "staged in LDS", "DZO_NEB_STORAGE_LDS", "DZO_NEB_STORAGE_MEMORY",
                   "768 bytes", "159 KiB", "Both storages compute the same bits", "x_m = fma(T(m / (M-1)), b - a, a)", "copies of a and b",
                   "ALIASES band_dev", "ONE launch", "Out of scope: alignment of arbitrary end pairs, the doubly-nudged spring term, L-BFGS on the band",
                   "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "DZO_ERR_NOMEM"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_neb_kernels_exist_for_gfx950_without_scratch():
    """Two launch shapes and the interpolation, two element types: no private segment, no VGPR or SGPR spill."""
    check_unit("neb", lj_count=6)


def test_the_source_takes_its_pieces_from_the_shared_headers():
    src = open(os.path.join(PKG, "csrc", "dzo_neb.hip")).read()
    for include in ('#include "dzo_cluster.h"', '#include "dzo_neb_plan.h"'):
        assert include in src, include
    for word in ("cl_wave_eval<", "cl_block_eval<", "cl_dot3(", "cl_block_sum(", "wave_sum_all(", "cl_step(", "cl_count(", "cl_get_ptr(", "cl_read(",
                 "cl_alloc(", "cl_finish_create(", "cl_check_args(", "ClCore core", 'DZO_TIMED("neb_step"', "neb_plan(", "kClLdsMax"):
        assert word in src, word
    for word in ("atomic", "printf(", "pw_pair<", "F::", "asm"):
        assert word not in src, word
    # one launch per step call, nothing waits inside it or after it
    step = src[src.index("int32_t dzo_neb_batch_step("):src.index("int32_t dzo_neb_batch_count_active(")]
    assert "Synchronize" not in step and "cl_step(" in step and step.count("neb_launch<T, F>(") == 1 and step.count("neb_launch<") == 1 and "for (" not in step
    cluster = open(os.path.join(PKG, "csrc", "dzo_cluster.h")).read()
    assert "__global__" not in cluster
    plan = open(os.path.join(PKG, "csrc", "dzo_neb_plan.h")).read()
    assert "hip" not in plan.replace("dzo_neb.hip", "").lower().replace("no hip here", "")     # a plain C++ header
    assert "csrc/dzo_neb.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_the_residency_plan_at_its_edges():
    """LDS storage exactly when 768 bytes, the stage of the BLOCK shape and 3 arrays of 3N M elements fit 159 KiB."""
    for dtype, es in ((np.float64, 8), (np.float32, 4)):
        # the WAVE shape always fits, the largest band included
        for n, m in ((1, 3), (3, 3), (38, 9), (64, 32)):
            assert dzo.neb_plan(n, m, dtype) == (dzo.NEB_SHAPE_WAVE, dzo.NEB_STORAGE_LDS, SMALL + 9 * n * m * es), (n, m)
        assert dzo.neb_plan(64, 32, dtype)[2] <= LDS_MAX
        assert dzo.neb_plan(65, 3, dtype) == (dzo.NEB_SHAPE_BLOCK, dzo.NEB_STORAGE_LDS, SMALL + 3 * 65 * es + 9 * 65 * 3 * es)
        # the BLOCK shape: for every image count the largest N that still fits, and the one above it
        for m in (3, 5, 9, 32):
            fits = lambda n: SMALL + 3 * n * es + 9 * n * m * es <= LDS_MAX
            edge = max(n for n in range(65, 1025) if fits(n)) if fits(65) else None
            if edge is not None:
                assert dzo.neb_plan(edge, m, dtype) == (dzo.NEB_SHAPE_BLOCK, dzo.NEB_STORAGE_LDS, SMALL + 3 * edge * es + 9 * edge * m * es), (m, edge)
            above = 65 if edge is None else edge + 1
            if above <= 1024:
                assert dzo.neb_plan(above, m, dtype) == (dzo.NEB_SHAPE_BLOCK, dzo.NEB_STORAGE_MEMORY, SMALL + 3 * above * es), (m, above)
    assert dzo.neb_plan(1024, 3, np.float64)[1] == dzo.NEB_STORAGE_MEMORY and dzo.neb_plan(1024, 3, np.float32)[1] == dzo.NEB_STORAGE_LDS
    assert dzo.neb_plan(130, 5, np.float64)[1] == dzo.NEB_STORAGE_LDS
    L = dzo.lib()
    assert L.dzo_neb_plan(10, 2, dzo.F64, None, None, None) == 1 and L.dzo_neb_plan(10, 33, dzo.F64, None, None, None) == 1
    assert L.dzo_neb_plan(0, 3, dzo.F64, None, None, None) == 1 and L.dzo_neb_plan(10, 3, 9, None, None, None) == 1
    assert L.dzo_neb_plan(1025, 3, dzo.F64, None, None, None) == 5 and L.dzo_neb_plan(1024, 32, dzo.F64, None, None, None) == 0


def test_lj_band_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_band")
    assert {"dzo_neb_batch_interpolate", "dzo_neb_batch_create", "dzo_neb_batch_step", "dzo_neb_batch_read", "dzo_neb_batch_destroy",
            "dzo_hybridef_batch_create", "dzo_tempering_run", "dzo_lbfgs_batch_step", "dzo_axpy"} <= wanted and wanted <= have, wanted - have
    src = open(os.path.join(ROOT, "examples", "lj_band.c")).read()
    assert "dzo_neb_batch_apply" not in src and "barrier" in src
