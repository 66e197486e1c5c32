"""CPU-side checks of the batched eigenvector-following unit (the method of tests/test_symeig_build.py): the library exports its
entry points, the Python table and the Julia module bind them, the constants match the header, the header states the
arithmetic of the step, the kernels exist for gfx950 in both element types without scratch memory or spills, and the plain-C example
compiles and links against the library alone.  No compute here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_modefollow_batch_" + s for s in ("apply", "create", "destroy", "set_start_mode", "set_directions", "step", "count_active",
                                                 "get_ptr", "read")]
WHATS = ["POINTS", "GRADIENTS", "ENERGIES", "GRMS", "STATUS", "INDEX", "ZEROS", "FOLLOWED_MODE", "STEP_LENGTHS", "ITERATION_COUNTS",
         "EIGENVALUES", "EIGENVECTORS", "SWEEPS", "FOLLOW"]


def test_library_exports_the_mode_following_entry_points():
    lib = ctypes.CDLL(dzo.build())
    assert [n for n in SYMBOLS if not hasattr(lib, n)] == []
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert len(dzo.ABI["dzo_modefollow_batch_apply"]) == 23 and len(dzo.ABI["dzo_modefollow_batch_create"]) == 10
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if "(:%s, libdzo)" % n not in julia] == []
    for name in ("ModeFollowing", "modefollow_apply!", "set_start_mode!", "set_directions!", "polish_minima", "find_saddles", "read_array"):
        assert name in julia[julia.index("export "):julia.index("const libdzo")], name
    for name in ("ModeFollowing", "modefollow_apply!", "polish_minima", "find_saddles", "read_array"):
        assert re.search(r"^function %s\(" % re.escape(name), julia, flags=re.M), name


def test_python_constants_and_functions_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    m = re.search(r"#define\s+DZO_MODEFOLLOW_MAX_PARTICLES\s+(\d+)\b", header)
    assert m and dzo.MODEFOLLOW_MAX_PARTICLES == int(m.group(1)) == 128 and 3 * 128 == dzo.SYMEIG_MAX_N
    for k, name in enumerate(WHATS):
        assert re.search(r"#define\s+DZO_MODEFOLLOW_%s\s+%d\b" % (name, k), header), name
        assert getattr(dzo, "MODEFOLLOW_" + name) == k
    for k, name in enumerate(("ACTIVE", "CONVERGED", "FAILED")):
        assert re.search(r"#define\s+DZO_MODEFOLLOW_%s\s+%d\b" % (name, k), header) and getattr(dzo, "MODEFOLLOW_" + name) == k
    assert issubclass(dzo.ModeFollowing, dzo._HandleArrays)
    assert list(inspect.signature(dzo.ModeFollowing.__init__).parameters)[1:7] == ["points", "n_particles", "target_index", "max_step",
                                                                                  "zero_tol", "grad_tol"]
    assert list(inspect.signature(dzo.polish_minima).parameters)[:4] == ["points", "n_particles", "grad_tol", "max_steps"]
    assert list(inspect.signature(dzo.find_saddles).parameters)[:4] == ["minima", "n_particles", "start_mode", "kick"]
    assert list(inspect.signature(dzo.modefollow_apply).parameters)[:4] == ["points", "eigenvalues", "eigenvectors", "n_particles"]


def test_header_states_the_arithmetic_of_the_step():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched eigenvector following")
    assert header.index("int32_t dzo_symeig_plan(") < start
    block = header[start:header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")]
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("with the bits of dzo_pairwise_batch_energy_gradient", "grms = sqrt((g.g)/n)", "offsets 32, 16, 8, 4, 2, 1",
                   "|lam[i]| <= zero_tol", "index = #{lam[i] < -zero_tol}", "sweeps = -1", "grms <= grad_tol", "the point is not moved",
                   "F[i] = V[:,i].g in fp64", "rounded once to T", "start_mode-th non-zero mode", "largest |V[:,i].w|", "ties go to the lowest i",
                   "w = V[:,i*] as stored, sign included", "a = |lam[i]|", "q = (F[i] + F[i]) / a", "h[i] = s * q / (1 + sqrt(1 + q*q))",
                   "h[i] = 0 for zero modes", "2F / (a (1 + sqrt(1 + 4F^2/a^2)))", "bounded by 1", "An overflowing q*q gives h = 0 by itself",
                   "hn = sqrt(sum h[i]^2)", "If hn > max_step", "T(max_step / hn)", "sum_i V[r,i] h[i]", "FUSED multiply-add",
                   "No floating-point atomics", "alone or anywhere in any batch", "ALIASES points_dev", "no host wait",
                   "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_modefollow_kernels_exist_for_gfx950_without_scratch():
    """One step kernel per element type: no private segment, no VGPR or SGPR spill."""
    check_unit("modefollow", lj_count=2)
    src = open(os.path.join(PKG, "csrc", "dzo_modefollow.hip")).read()
    body = src.split("namespace dzo {", 1)[1]
    assert "atomic" not in body and "cl_wave_eval<" in body and "cl_block_eval<" in body and "cl_block_sum(" in body
    assert "hb_enqueue_hessian(" in body and "se_enqueue(" in body and 'DZO_TIMED("modefollow_step"' in body
    # nothing waits between the three launches of a step: the only waits of the file are apply's and destroy's
    step = body[body.index("int32_t dzo_modefollow_batch_step("):body.index("int32_t dzo_modefollow_batch_count_active(")]
    assert "Synchronize" not in step and "cl_step(" in step
    assert "csrc/dzo_modefollow.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_saddle_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_saddle")
    assert {"dzo_modefollow_batch_create", "dzo_modefollow_batch_step", "dzo_modefollow_batch_set_directions", "dzo_modefollow_batch_read",
            "dzo_tempering_run", "dzo_lbfgs_batch_step"} <= wanted and wanted <= have, wanted - have
