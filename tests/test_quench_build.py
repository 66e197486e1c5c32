"""CPU-side checks of the batched L-BFGS entry points: the library exports them, the Python table binds them, the constants
match the header, the kernels exist for gfx950 without scratch memory or spills (the method of
tests/test_tempering_build.py), and the plain-C example compiles and links against the library alone.  No compute here."""
import ctypes
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_lbfgs_batch_create", "dzo_lbfgs_batch_destroy", "dzo_lbfgs_batch_set_max_halvings", "dzo_lbfgs_batch_step",
           "dzo_lbfgs_batch_count_active", "dzo_lbfgs_batch_get_ptr", "dzo_lbfgs_batch_read", "dzo_pairwise_batch_energy_gradient"]
WHAT = ["POINTS", "GRADIENTS", "DIRECTIONS", "DELTA_POINTS", "DELTA_GRADIENTS", "OBJECTIVES", "DELTA_OBJECTIVES", "IS_STUCK",
        "ITERATION_COUNTS", "HISTORY_COUNTS", "S", "Y", "RHO", "LAST_HALVINGS"]


def test_library_exports_the_batched_lbfgs_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []


def test_python_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    values = []
    for name in WHAT + ["MAX_PARTICLES", "MAX_HISTORY"]:
        m = re.search(r"#define\s+DZO_LBFGS_BATCH_%s\s+(\d+)\b" % name, header)
        assert m, name
        assert getattr(dzo, "LBFGS_BATCH_" + name) == int(m.group(1)), name
        values.append(int(m.group(1)))
    assert sorted(values[:len(WHAT)]) == list(range(len(WHAT)))
    assert dzo.LBFGS_BATCH_MAX_PARTICLES == 1024 and dzo.LBFGS_BATCH_MAX_HISTORY == 32
    assert callable(dzo.BatchedLBFGS) and callable(dzo.pairwise_batch_energy_gradient) and callable(dzo.ParallelTempering.quench)
    for f in ("step", "count_active", "read", "set_max_halvings"):
        assert callable(getattr(dzo.BatchedLBFGS, f))
    for p in ("current_points", "current_gradients", "current_objective_values", "is_stuck", "iteration_counts"):
        assert isinstance(getattr(dzo.BatchedLBFGS, p), property), p


def test_header_cites_the_reference_for_every_entry():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    block = header[header.index("Batched LBFGSOptimizer"):]
    for needle in (":454-509", ":107-154", ":430-451", ":381-387", ":393", "max_halvings", "newest first"):
        assert needle in block, needle


def test_quench_kernels_exist_for_gfx950_without_scratch():
    """Both launch shapes of the step kernel (the BLOCK shape with the history in LDS and in device memory) and of the
    evaluation kernel, two element types each: no private segment, no VGPR or SGPR spill."""
    check_unit("lbfgs_batch", lj_count=11)                    # ... and the one count kernel


def test_source_uses_the_shared_pair_arithmetic():
    """The quench, the batched AdGD and the header both are built on (dzo_cluster.h, which holds their pair loops)."""
    src, adgd, header = (open(os.path.join(PKG, "csrc", f)).read() for f in ("dzo_lbfgs_batch.hip", "dzo_adgd_batch.hip", "dzo_cluster.h"))
    assert '#include "dzo_cluster.h"' in src and '#include "dzo_cluster.h"' in adgd and '#include "dzo_pairwise.h"' in header
    for text in (src, adgd):
        assert "cl_wave_eval<T, F>(" in text and "cl_block_eval<T, F>(" in text
    assert "qc_wave_run<T, F>(" in src and "qc_block_run<T, F>(" in src and "pw_pair<" in header
    for text in (src, adgd, header):
        assert "F::energy(" not in text and "F::first(" not in text
    # the one integer count; no floating-point atomic
    assert "atomicAdd(&total" in src and src.count("atomic") + adgd.count("atomic") + header.count("atomic") <= 4
    makefile = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/dzo_lbfgs_batch.hip" in makefile and "csrc/dzo_adgd_batch.hip" in makefile


def test_lj_quench_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_quench")
    assert {"dzo_lbfgs_batch_create", "dzo_lbfgs_batch_step", "dzo_lbfgs_batch_read", "dzo_tempering_run"} <= wanted and wanted <= have, wanted - have
