"""CPU-side checks of the batched lowest Hessian mode (the method of tests/test_hessian_batch_build.py): the library exports the
entry point, the Python table and the Julia module bind it, the constants match the header, the header block sits where its
neighbours are and states what a caller relies on, the kernels exist for gfx950 in both launch shapes and both element types
without scratch memory or spills, the source takes its pair
term from dzo_pairwise.h and its dots from dzo_cluster.h, and the plain-C example compiles and links against the library alone.
No compute here."""
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
SYMBOL = "dzo_pairwise_batch_lowest_mode"


def test_library_exports_the_entry_point_and_both_hosts_bind_it():
    lib = ctypes.CDLL(dzo.build())
    assert hasattr(lib, SYMBOL)
    assert SYMBOL in dzo.ABI and len(dzo.ABI[SYMBOL]) == 15
    assert dzo.ABI[SYMBOL][9] is ctypes.c_uint64 and dzo.ABI[SYMBOL][8] is ctypes.c_double
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert "(:%s, libdzo)" % SYMBOL in julia
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    assert "lowest_modes" in exports and "function lowest_modes(" in julia


def test_python_constants_and_signature_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    assert dzo.LOWMODE_MAX_PARTICLES == value("DZO_LOWMODE_MAX_PARTICLES") == 1024
    assert dzo.LOWMODE_MAX_KRYLOV == value("DZO_LOWMODE_MAX_KRYLOV") == 32
    assert [dzo.LOWMODE_CONVERGED, dzo.LOWMODE_UNFINISHED, dzo.LOWMODE_FAILED] == [value("DZO_LOWMODE_" + s) for s in ("CONVERGED", "UNFINISHED", "FAILED")]
    assert len({dzo.LOWMODE_CONVERGED, dzo.LOWMODE_UNFINISHED, dzo.LOWMODE_FAILED}) == 3
    assert value("DZO_VERSION") == 100
    sig = inspect.signature(dzo.lowest_modes).parameters
    assert list(sig)[:9] == ["points", "n_particles", "project_rigid", "krylov", "max_cycles", "res_tol", "start", "seed", "radial"]
    assert sig["project_rigid"].default is True and sig["krylov"].default == 32 and sig["res_tol"].default is None and sig["start"].default is None
    assert sig["seed"].default == 0
    tol = dzo.LOWMODE_DEFAULT_RES_TOL
    assert set(tol) == {np.dtype(np.float64), np.dtype(np.float32)} and 0 < tol[np.dtype(np.float64)] < tol[np.dtype(np.float32)] < 1e-3


def test_header_block_is_in_place_and_states_the_contract():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched lowest Hessian mode")
    assert header.index("Batched eigenvector following") < start < header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("int32_t dzo_modefollow_batch_read(") < start
    block = header[start:header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")]
    for needle in (":427-468", "An instance computes the same bits alone or anywhere in any batch", "No floating-point atomics",
                   "every output element is written once", "CLASSICAL Gram-Schmidt", "det > 2^-36", "collinear", "0x14057B7EF767814F + base_seed + b",
                   "at most four passes", "s > 0.7", "items 3-5", "off2 <= 2^-104", "at most max_cycles K", "DZO_ERR_NOMEM", "DZO_ERR_UNSUPPORTED",
                   "DZO_ERR_ASSERT", "status at\n * 3 b, cycles at 3 b + 1, products at 3 b + 2", "the same bits"):
        assert needle in block, needle
    assert "int32_t %s(" % SYMBOL in block


def test_lowmode_kernels_exist_for_gfx950_without_scratch():
    """Two launch shapes, two element types: no private segment, no VGPR or SGPR spill."""
    check_unit("lowmode", lj_count=4)


def test_the_product_and_the_dots_have_one_definition():
    """The per-pair arithmetic is pw_pair of dzo_pairwise.h, called as dzo_hessian_batch.hip calls it; the dots are cl_dot3 on
    wave_sum_all; the draws are those of dzo_pcg.h; nothing is added up in memory."""
    src = open(os.path.join(PKG, "csrc", "dzo_lowmode.hip")).read()
    for include in ('#include "dzo_pairwise.h"', '#include "dzo_cluster.h"', '#include "dzo_pcg.h"'):
        assert include in src, include
    assert src.count("pw_pair<T, F, kPwHvp>(") == 2          # one call per launch shape
    assert "F::" not in src and "atomic" not in src
    assert "cl_dot3(" in src and "wave_sum_all(" in src and "pcg_normals<T>(" in src and "pcg_advance(kPcgInc + " in src
    assert "lowmode_wave_kernel" in src and "lowmode_block_kernel" in src and 'DZO_TIMED("lowmode"' in src
    for word in ("__builtin_fma", "printf("):
        assert word not in src, word
    assert "csrc/dzo_lowmode.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_lowest_mode_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_lowest_mode")
    assert {SYMBOL, "dzo_tempering_create", "dzo_tempering_run", "dzo_lbfgs_batch_create", "dzo_lbfgs_batch_step", "dzo_pairwise_batch_hessian",
            "dzo_symmetric_batch_eigen"} <= wanted and wanted <= have, wanted - have
