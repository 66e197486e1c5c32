"""CPU-side checks of the structure unit (the method of tests/test_lowmode_build.py): the library exports the two entry points,
the Python table and the Julia module bind them with the header's arity, the constants match the header, the header block sits
behind the hybrid eigenvector-following block and states its contract, the kernels exist for gfx950 in both launch shapes and
both element types without scratch memory or spills, the source takes its pair term from dzo_pairwise.h and its sums from dzo_cluster.h, and the plain-C
example compiles and links against the library alone.  No compute here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_structure_batch_fingerprint", "dzo_structure_batch_classify"]


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
        assert arity == 7 and len(dzo.ABI[name]) == arity, name
        calls = list(re.finditer(r"ccall\(\(:%s, libdzo\), Cint,\s*\(" % name, julia))
        assert calls, name
        for m in calls:                                      # the argument-type tuple of every literal ccall
            depth, i = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(julia[i], 0)
                i += 1
            types = [t for t in re.sub(r"\{[^}]*\}", "", julia[m.end():i - 1]).split(",") if t.strip()]
            assert len(types) == arity, (name, types)
    assert dzo.ABI["dzo_structure_batch_classify"][4] is ctypes.c_double
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    for name in ("structure_fingerprints", "classify_structures", "connect_saddles"):
        assert name in exports and re.search(r"^function %s\(" % name, julia, flags=re.M), name


def test_python_constants_and_signatures_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    assert dzo.STRUCTURE_MAX_PARTICLES == value("DZO_STRUCTURE_MAX_PARTICLES") == 1024 == dzo.LBFGS_BATCH_MAX_PARTICLES
    assert dzo.STRUCTURE_MAX_BATCH == value("DZO_STRUCTURE_MAX_BATCH") == 16384
    assert value("DZO_VERSION") == 100
    assert list(inspect.signature(dzo.structure_fingerprints).parameters) == ["points", "n_particles", "radial"]
    assert list(inspect.signature(dzo.classify_structures).parameters) == ["fingerprints", "tol"]
    assert list(inspect.signature(dzo.unique_structures).parameters)[:3] == ["points", "n_particles", "tol"]
    sig = inspect.signature(dzo.connect_saddles).parameters
    assert list(sig)[:10] == ["saddles", "modes", "n_particles", "displacement", "tol", "known_minima", "history_length", "initial_step_length",
                              "steps_per_launch", "max_steps"]
    # the two values that depend on the element type and the system have no default
    assert sig["displacement"].default is inspect.Parameter.empty and sig["tol"].default is inspect.Parameter.empty
    assert inspect.signature(dzo.classify_structures).parameters["tol"].default is inspect.Parameter.empty
    assert inspect.signature(dzo.unique_structures).parameters["tol"].default is inspect.Parameter.empty
    assert (sig["known_minima"].default, sig["history_length"].default, sig["initial_step_length"].default, sig["steps_per_launch"].default,
            sig["max_steps"].default) == (None, 10, 0.01, 50, 2000)
    assert "structure-readme" in dzo.connect_saddles.__doc__


def test_header_block_is_in_place_and_states_the_contract():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Structure fingerprints and their classification")
    end = header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("Batched hybrid eigenvector following") < header.index("int32_t dzo_hybridef_batch_read(") < start < end
    block = header[start:end]
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("DZO_STRUCTURE_MAX_PARTICLES = 1024", "DZO_STRUCTURE_MAX_BATCH = 16384", "with j ascending", "dropped by a select",
                   "E has the bits of dzo_pairwise_batch_energy_gradient", "one division in fp64, one rounding to T",
                   "[e sorted ascending (N) | d sorted ascending (N)]", "bitonic sort", "padded with +inf to a power of two",
                   "Values that are not numbers sort last", "No floating-point atomics", "every output element is written once",
                   "the same bits alone or anywhere in any batch", "there is no device-memory fallback",
                   "it does not tell a structure from its mirror image", "two different structures could in principle share it",
                   "GMIN-style", "|a_i - b_i| <= tol * max(1, |a_i|, |b_i|)", "evaluated in fp64", "gets label -1",
                   "greedy leader labels in index order", "first REPRESENTATIVE", "deliberately not \"the smallest matching index\"",
                   "matching is not transitive", "length is free", "match against a database", "leaves at the first failing element",
                   "does not depend on grid size or scheduling", "batch^2 / 8 bytes", "The call blocks",
                   "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "DZO_ERR_NOMEM"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_structure_kernels_exist_for_gfx950_without_scratch():
    """Two launch shapes and two element types of the fingerprint, the comparison in both element types, one label kernel: no
    private segment, no VGPR or SGPR spill."""
    check_unit("structure", lj_count=7)


def test_the_source_takes_its_pieces_from_the_shared_headers():
    src = open(os.path.join(PKG, "csrc", "dzo_structure.hip")).read()
    for include in ('#include "dzo_pairwise.h"', '#include "dzo_cluster.h"'):
        assert include in src, include
    assert src.count("pw_pair<T, F, kPwEnergy>(") == 2       # one call per launch shape
    for word in ("pw_r2(", "wave_sum_all(", "cl_block_sum(", "CL_FOR_OWN(", "pw_check_args(", "device_alloc(", "copy_blocking(",
                 'DZO_TIMED("structure_fingerprint"', 'DZO_TIMED("structure_compare"', 'DZO_TIMED("structure_label"'):
        assert word in src, word
    for word in ("F::", "atomic", "printf(", "cl_wave_eval", "cl_block_eval", "__builtin_fma"):
        assert word not in src, word
    cluster = open(os.path.join(PKG, "csrc", "dzo_cluster.h")).read()
    assert "__global__" not in cluster
    assert "csrc/dzo_structure.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_pathways_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_pathways")
    assert {"dzo_structure_batch_fingerprint", "dzo_structure_batch_classify", "dzo_tempering_run", "dzo_lbfgs_batch_step",
            "dzo_pairwise_batch_lowest_mode", "dzo_hybridef_batch_step", "dzo_hybridef_batch_get_ptr", "dzo_pairwise_batch_energy_gradient",
            "dzo_axpy", "dzo_fill"} <= wanted and wanted <= have, wanted - have
