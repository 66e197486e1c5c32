"""CPU-side checks of the parallel-tempering entry points: the library exports them, the Python table binds them, the
kernels exist for gfx950 without scratch memory or spills (the method of tests/test_pairwise_build.py), and the plain-C
example compiles and links against the library alone.  No compute here."""
import ctypes
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_tempering_create", "dzo_tempering_destroy", "dzo_tempering_temper", "dzo_tempering_swap", "dzo_tempering_run",
           "dzo_tempering_analyze", "dzo_tempering_set_record", "dzo_tempering_get_ptr", "dzo_tempering_read", "dzo_tempering_set"]


def test_library_exports_the_tempering_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert lib.dzo_version() == 100


def test_python_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    names = ["REPLICAS", "RADII", "INV_TEMPS", "NUM_ACCEPT", "NUM_REJECT", "RNG_STATES", "REC_INDEX", "REC_NORMALS", "REC_UNIFORM",
             "REC_CODE", "REC_SWAP", "REC_SWAP_LOGP", "MAX_PARTICLES"]
    for name in names:
        m = re.search(r"#define\s+DZO_TEMPERING_%s\s+(\d+)\b" % name, header)
        assert m, name
        assert getattr(dzo, "TEMPERING_" + name) == int(m.group(1)), name
    assert callable(dzo.ParallelTempering)
    for f in ("temper", "swap", "run", "analyze", "set_record", "read"):
        assert callable(getattr(dzo.ParallelTempering, f))


def test_header_states_the_random_number_rule():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    for needle in ("0x5851F42D4C957F2D", "0x14057B7EF767814F", "SIX draws", "(d0 * N) >> 32", "Box-Muller", "scripts/MonteCarlo.jl"):
        assert needle in header, needle


def test_tempering_kernels_exist_for_gfx950_without_scratch():
    """Both launch shapes of the temper kernel, the swap and the analyze kernel, two element types each; every one keeps its
    state in registers: no private segment, no VGPR or SGPR spill."""
    check_unit("tempering", lj_count=8)


def test_source_uses_the_shared_pair_arithmetic():
    src = open(os.path.join(PKG, "csrc", "dzo_tempering.hip")).read()
    assert '#include "dzo_pairwise.h"' in src and "pw_pair_energy<" in src
    assert "F::energy(" not in src


def test_lj_tempering_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_tempering")
    assert {"dzo_tempering_create", "dzo_tempering_run", "dzo_tempering_analyze"} <= wanted and wanted <= have, wanted - have
