"""CPU-side checks of the batched Hessian entry points (the method of tests/test_adgd_batch_build.py): the library exports them,
the Python table and the Julia module bind them, the constant matches the header, the header states the arithmetic with the
reference's lines, the kernels exist for gfx950 in both launch shapes, both entries and both element types without scratch
memory or spills, the source takes its pair term from dzo_pairwise.h, and the plain-C example compiles and links against the
library alone.  No compute here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_pairwise_batch_hvp", "dzo_pairwise_batch_hessian"]


def test_library_exports_the_batched_hessian_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert len(dzo.ABI["dzo_pairwise_batch_hvp"]) == 9 and len(dzo.ABI["dzo_pairwise_batch_hessian"]) == 6
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if "(:%s, libdzo)" % n not in julia] == []


def test_python_constant_and_functions_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    m = re.search(r"#define\s+DZO_HESSIAN_BATCH_MAX_PARTICLES\s+(\d+)\b", header)
    assert m and dzo.HESSIAN_BATCH_MAX_PARTICLES == int(m.group(1)) == 1024
    for f in ("pairwise_batch_hvp", "pairwise_batch_hessian", "hessian_eigenvalues", "morse_index"):
        assert callable(getattr(dzo, f)), f
    hvp = inspect.signature(dzo.pairwise_batch_hvp).parameters
    assert list(hvp)[:6] == ["points", "directions", "n_particles", "products", "curvatures", "shared_point"]
    assert hvp["products"].default is None and hvp["curvatures"].default is False and hvp["shared_point"].default is False
    assert list(inspect.signature(dzo.pairwise_batch_hessian).parameters)[:3] == ["points", "n_particles", "out"]
    tol = inspect.signature(dzo.morse_index).parameters["zero_tol"]
    assert tol.default is inspect.Parameter.empty            # no invented default


def test_header_states_the_arithmetic_with_the_reference_lines():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched Hessian-vector products and dense Hessians")
    assert header.index("Batched AdGDOptimizer") < start
    block = header[start:header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")]
    for banned in ("Batched LBFGSOptimizer", "Batched AdGDOptimizer"):
        assert banned not in block
    for needle in (":367-468", ":50-72", "column-major", "No floating-point atomics", "point_stride",
                   "column c of hessians[b] has the same values as\n * dzo_pairwise_batch_hvp of points[b] with the unit direction e_c",
                   "du = -e_b", "sequentially in T from +0", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "r + 3N (c + 3N b)"):
        assert needle in block, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_hessian_batch_kernels_exist_for_gfx950_without_scratch():
    """Both launch shapes of both entries, two element types each: no private segment, no VGPR or SGPR spill."""
    check_unit("hessian_batch", lj_count=8)


def test_the_pair_term_has_one_definition():
    """The per-pair arithmetic is pw_pair of dzo_pairwise.h: the file calls no radial function itself and adds up nothing in
    memory; its fp64 dots and its block sum are those of dzo_cluster.h, on wave_sum_all."""
    src = open(os.path.join(PKG, "csrc", "dzo_hessian_batch.hip")).read()
    assert '#include "dzo_pairwise.h"' in src
    assert "pw_pair<T, F, kPwHvp>(" in src
    assert "F::" not in src and "atomic" not in src
    assert "wave_sum_all(" in src
    assert '#include "dzo_cluster.h"' in src and "cl_dot3(" in src and "cl_block_sum2(" in src
    for own in ("hb_dot3", "hb_block_sum2", "hb_check_common", "__builtin_fma", "__syncthreads();\n    double r"):
        assert own not in src, own                           # no dot or block sum of its own
    assert 'DZO_TIMED("hess_batch_hvp"' in src and 'DZO_TIMED("hess_batch_hessian"' in src
    makefile = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/dzo_hessian_batch.hip" in makefile


def test_lj_hessian_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_hessian")
    assert {"dzo_pairwise_batch_hessian", "dzo_pairwise_batch_hvp", "dzo_lbfgs_batch_create", "dzo_lbfgs_batch_step",
            "dzo_pairwise_batch_energy_gradient"} <= wanted and wanted <= have, wanted - have
