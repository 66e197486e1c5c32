"""CPU-side checks of the batched AdGD entry points (the method of tests/test_quench_build.py): the library exports them, the
Python table binds them, the constants match the header, the header states the arithmetic with the reference's lines, the step
kernels exist for gfx950 in both launch shapes and element types without scratch memory or spills, and the plain-C example
compiles and links against the library alone.  No compute here."""
import ctypes
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_adgd_batch_create", "dzo_adgd_batch_destroy", "dzo_adgd_batch_set_max_halvings", "dzo_adgd_batch_step",
           "dzo_adgd_batch_count_active", "dzo_adgd_batch_get_ptr", "dzo_adgd_batch_read"]
WHAT = ["POINTS", "GRADIENTS", "DELTA_POINTS", "DELTA_GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES", "IS_STUCK", "ITERATION_COUNTS",
        "CURRENT_STEP_SIZES", "PREVIOUS_STEP_SIZES", "LAST_HALVINGS"]


def test_library_exports_the_batched_adgd_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if "(:%s, libdzo)" % n not in julia] == []


def test_python_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    values = []
    for name in WHAT + ["MAX_PARTICLES"]:
        m = re.search(r"#define\s+DZO_ADGD_BATCH_%s\s+(\d+)\b" % name, header)
        assert m, name
        assert getattr(dzo, "ADGD_BATCH_" + name) == int(m.group(1)), name
        values.append(int(m.group(1)))
    assert sorted(values[:len(WHAT)]) == list(range(11))
    assert dzo.ADGD_BATCH_MAX_PARTICLES == 1024
    assert callable(dzo.BatchedAdGD)
    for f in ("step", "count_active", "read", "ptr", "set_max_halvings", "close"):
        assert callable(getattr(dzo.BatchedAdGD, f)), f
    for p in ("current_points", "current_gradients", "delta_points", "delta_gradients", "current_objective_values",
              "delta_objective_values", "is_stuck", "iteration_counts", "current_step_sizes", "previous_step_sizes", "last_halvings"):
        assert isinstance(getattr(dzo.BatchedAdGD, p), property), p


def test_header_states_the_arithmetic_with_the_reference_lines():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    block = header[header.index("Batched AdGDOptimizer"):header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")]
    for needle in (":274-312", ":107-154", ":229-241", ":298-299", "max_halvings", ":245-271", ":216-217", ":229)", "sqrt(1 + theta)",
                   "fused multiply-add", "No floating-point atomics"):
        assert needle in block, needle


def test_adgd_batch_kernels_exist_for_gfx950_without_scratch():
    """Both launch shapes of the step kernel and the constructor's kernel, two element types each: no private segment, no VGPR
    or SGPR spill."""
    check_unit("adgd_batch", lj_count=6)


def _csrc():
    """(dzo_cluster.h, {name: text of every .hip})"""
    csrc = os.path.join(PKG, "csrc")
    return open(os.path.join(csrc, "dzo_cluster.h")).read(), {f: open(os.path.join(csrc, f)).read()
                                                              for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}


def test_the_evaluation_has_one_definition():
    """The trial's energy and gradient, the block sums and the dots are the routines of dzo_cluster.h, defined once there and in
    no .hip; the step-size rule is the only arithmetic dzo_adgd_batch.hip adds."""
    header, hips = _csrc()
    for routine in ("void cl_wave_eval(", "void cl_block_eval(", "double cl_block_sum(", "void cl_block_sum2(", "double cl_dot3(",
                    "#define CL_FOR_OWN(", "int32_t cl_check_args("):
        assert header.count(routine) == 1, routine
        assert [f for f, text in hips.items() if routine in text] == [], routine
    assert "__global__" not in header
    assert [f for f, text in hips.items() if "void quench_count_active_kernel(" in text] == ["dzo_lbfgs_batch.hip"]
    assert hips["dzo_lbfgs_batch.hip"].count("void quench_count_active_kernel(") == 1
    assert "#undef" not in header and [f for f, text in hips.items() if "CL_FOR_OWN" in text and "#define" in text] == []
    for name in ("q_wave_eval", "q_block_eval", "q_block_sum_all", "q_dot3", "DZO_Q_OWN", "hb_dot3", "hb_block_sum2", "block_sum2_all"):
        assert [f for f, text in hips.items() if name in text] == [] and name not in header, name
    section = hips["dzo_adgd_batch.hip"]
    for call in ("cl_wave_eval<T, F>(", "cl_block_eval<T, F>(", "cl_block_sum(", "cl_dot3(", "cl_step(", "cl_count(", "cl_launch_eval<T>("):
        assert call in section, call
    assert "dzo_lbfgs_batch_s" not in section                # the evaluation needs no handle of the other optimizer
    assert "pw_pair" not in section and "F::" not in section
    assert 'DZO_TIMED("adgd_batch_init"' in section and 'DZO_TIMED("adgd_batch_step"' in section
    assert header.count("hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClLdsMax") == 1
    # ... which dzo_adgd_batch_create raises for the block step kernel of the handle's radial and element type
    assert "DZO_DISPATCH_RADIAL(radial, dtype, k = (const void *)adgd_batch_block_step_kernel<T, F>)" in section
    assert "cl_finish_create(&c, k, " in section
    assert "csrc/dzo_adgd_batch.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_adgd_quench_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_adgd_quench")
    assert {"dzo_adgd_batch_create", "dzo_adgd_batch_step", "dzo_adgd_batch_read", "dzo_adgd_batch_count_active",
            "dzo_tempering_run"} <= wanted and wanted <= have, wanted - have
