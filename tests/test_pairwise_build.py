"""CPU-side checks of the pairwise radial (Lennard-Jones) objective: the library exports its entry points, the Python
table binds them, its kernels exist for gfx950 without scratch memory or spills, and the plain-C example compiles and
links against the library alone.  No compute here."""
import ctypes
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dzo_pairwise_energy", "dzo_pairwise_gradient", "dzo_pairwise_hvp", "dzo_pairwise_energy_delta", "dzo_calibrate_fma_rate"]


def test_library_exports_the_pairwise_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert lib.dzo_version() == 100


def test_python_constants_and_functions():
    assert dzo.PAIRWISE_LJ == 5 and dzo.RADIAL_LENNARD_JONES == 0
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    assert re.search(r"#define\s+DZO_PROBLEM_PAIRWISE_LJ\s+5\b", header)
    assert re.search(r"#define\s+DZO_RADIAL_LENNARD_JONES\s+0\b", header)
    for f in ("pairwise_radial_energy", "pairwise_radial_gradient_", "pairwise_radial_hvp_", "pairwise_radial_energy_delta",
              "calibrate_fma_rate"):
        assert callable(getattr(dzo, f))


def test_pairwise_kernels_exist_for_gfx950_without_scratch():
    """The tile and wave kernels in their three modes, the energy difference and the two finishing kernels, two element types:
    every one of them, under every radial, keeps its accumulators in registers: no private segment, no VGPR or SGPR spill."""
    check_unit("pairwise", lj_count=17, morse_sgpr_clean=True)


def test_lj_cluster_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_cluster")
    assert {"dzo_pairwise_energy", "dzo_problem_create", "dzo_lbfgs_step"} <= wanted and wanted <= have, wanted - have
