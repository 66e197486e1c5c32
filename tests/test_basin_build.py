"""CPU-side checks of the batched basin-hopping unit (the method of tests/test_modefollow_build.py): the library exports its
entry points, the Python table and the Julia module bind them, the constants match the header, the header states the rule of a
hop, the kernels exist for gfx950 in both element types and both launch shapes without scratch memory or spills, the quench loop is defined
once (csrc/dzo_quench_core.h) and called by both units, and the plain-C example compiles and links against the library alone.
No compute here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_basin_hopping_" + s for s in ("create", "destroy", "set_max_halvings", "hop", "set_record", "get_ptr", "read", "set")]
WHATS = ["POINTS", "ENERGIES", "BEST_POINTS", "BEST_ENERGIES", "RADII", "INV_TEMPS", "NUM_ACCEPT", "NUM_REJECT", "RNG_STATES", "HOP_COUNTS",
         "QUENCH_ITERATIONS", "QUENCH_UNFINISHED", "REC_NORMALS", "REC_UNIFORM", "REC_TRIAL_ENERGY", "REC_QUENCH_ITERATIONS", "REC_CODE"]


def _csrc(name):
    return open(os.path.join(PKG, "csrc", name)).read()


def test_library_exports_the_basin_hopping_entry_points():
    lib = ctypes.CDLL(dzo.build())
    assert [n for n in SYMBOLS if not hasattr(lib, n)] == []
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert len(dzo.ABI["dzo_basin_hopping_create"]) == 13 and len(dzo.ABI["dzo_basin_hopping_hop"]) == 3
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if "(:%s, libdzo)" % n not in julia] == []
    for name in ("BasinHopping", "hop!", "read_array"):
        assert name in julia[julia.index("export "):julia.index("const libdzo")], name
    for name in ("BasinHopping", "hop!"):
        assert re.search(r"^function %s\(" % re.escape(name), julia, flags=re.M), name
    assert re.search(r"^function read_array\(bh::BasinHopping", julia, flags=re.M)


def test_python_constants_and_class_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    m = re.search(r"#define\s+DZO_BASIN_HOPPING_MAX_PARTICLES\s+(\d+)\b", header)
    assert m and dzo.BASIN_HOPPING_MAX_PARTICLES == int(m.group(1)) == 1024
    for k, name in enumerate(WHATS):
        assert re.search(r"#define\s+DZO_BASIN_HOPPING_%s\s+%d\b" % (name, k), header), name
        assert getattr(dzo, "BASIN_HOPPING_" + name) == k
    assert len(re.findall(r"#define\s+DZO_BASIN_HOPPING_[A-Z_]+\s+\d+", header)) == len(WHATS) + 1
    assert issubclass(dzo.BasinHopping, dzo._HandleArrays)
    sig = inspect.signature(dzo.BasinHopping.__init__).parameters
    assert list(sig)[1:11] == ["points", "n_particles", "inverse_temperatures", "perturbation_radii", "constraining_radius",
                               "initial_step_length", "history_length", "quench_steps", "base_seed", "radial"]
    assert (sig["initial_step_length"].default, sig["history_length"].default, sig["quench_steps"].default, sig["base_seed"].default) == (0.01, 10, 400, 0)
    hop = inspect.signature(dzo.BasinHopping.hop).parameters
    assert list(hop)[1:] == ["num_hops", "adapt", "hops_per_launch", "wait"]
    assert (hop["adapt"].default, hop["hops_per_launch"].default, hop["wait"].default) == (True, 8, True)
    for f in ("set_record", "read", "ptr", "set_max_halvings", "close"):
        assert callable(getattr(dzo.BasinHopping, f)), f
    for p in ("current_points", "energies", "best_points", "best_energies", "perturbation_radii", "inverse_temperatures", "rng_states", "num_accept",
              "num_reject", "hop_counts", "quench_iterations", "quench_unfinished"):
        assert isinstance(getattr(dzo.BasinHopping, p), property), p
    assert dzo.BasinHopping.perturbation_radii.fset and dzo.BasinHopping.rng_states.fset


def test_header_states_the_rule_of_a_hop():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched basin hopping")
    assert header.index("int32_t dzo_pairwise_batch_energy_gradient(") < start
    block = header[start:header.index("Batched AdGDOptimizer")]
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("Wales & Doye 1997", "scripts/MonteCarlo.jl:49-55", "scripts/MonteCarlo.jl:63-70", "src/DZOptimization.jl:321-509",
                   "ALIASES it", "current minima", "(2 history_length + 6) 3N elements", "advance(0x14057B7EF767814F + base_seed + b)",
                   "consumes no draws, is always kept", "exactly 4N + 1 draws", "pcg_jump(s, 4N + 1)", "s' = A_k s + C_k", "draws 4i .. 4i+3",
                   "fourth normal unused", "Draw 4N is the acceptance uniform", "u = d 2^-32", "old + radius * n", "a product and a sum in T",
                   "x^2 + y^2 + z^2 < R^2", "keeps its old position", "exactly dzo_lbfgs_batch_create on the trial",
                   "dzo_lbfgs_batch_step(quench_steps)", "have the bits of those calls", "delta = E_q - E in T",
                   "E_q is finite and (delta <= 0 || u <= exp(-beta * delta))", "E_q < BEST_ENERGY, accepted or not", "two coincident particles",
                   "scripts/MonteCarlo.jl:77-81", "the same cap of 1", "When adapt == 0 the radii stay", "No floating-point atomics",
                   "alone or anywhere in any batch", "hop(a) followed by hop(b) equals hop(a + b) when adapt == 0", "DZO_ERR_INVALID",
                   "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "do not block", "A launch lasts num_hops quenches", "keep num_hops small"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_basin_hopping_kernels_exist_for_gfx950_without_scratch():
    """One wave kernel and two block kernels (ring in LDS / in the slab) per element type: no private segment, no VGPR or SGPR
    spill.  (tests/test_kernel_inventory.py: no kernel belongs to two units, and every unit's count is what it was.)"""
    check_unit("basin_hopping", lj_count=6)


def test_the_quench_loop_has_one_definition():
    """csrc/dzo_quench_core.h defines the step loop of either shape and the constructor's first direction once; the step and
    evaluation kernels of dzo_lbfgs_batch.hip and the basin-hopping kernels call them; the generator is dzo_pcg.h's in both
    Monte Carlo units."""
    core, quench, basin, temper, pcg = (_csrc(f) for f in ("dzo_quench_core.h", "dzo_lbfgs_batch.hip", "dzo_basin_hopping.hip", "dzo_tempering.hip",
                                                          "dzo_pcg.h"))
    assert "__global__" not in core and "__shared__" not in core and "atomic" not in core
    for routine in ("bool qc_wave_run(", "bool qc_block_run(", "bool qc_wave_first_direction(", "T qc_block_first_scale("):
        assert core.count(routine) == 1, routine
        assert routine not in quench and routine not in basin, routine
    for call in ("qc_wave_run<T, F>(", "qc_block_run<T, F>(", "qc_wave_first_direction<T>(", "qc_block_first_scale<T>("):
        assert call in quench and call in basin, call
    # the loop's landmarks are in the header and in neither unit
    for landmark in ("// take_backtracking_step!, :107-154", "// compute_lbfgs_step_direction!, :430-451", "// pushfirst!, :482-496", "t *= T(0.5);",
                     "if (Et < E)"):
        assert landmark in core and landmark not in quench and landmark not in basin, landmark
    assert '#include "dzo_quench_core.h"' in quench and '#include "dzo_quench_core.h"' in basin
    assert "atomic" not in basin.split("namespace dzo {", 1)[1]
    assert "cl_wave_eval<T, F>(" in basin and "cl_block_eval<T, F>(" in basin and "pw_pin_ptr(" in basin
    assert "F::energy(" not in basin and "F::first(" not in basin
    for text in (basin, temper):
        assert '#include "dzo_pcg.h"' in text and "pcg_normals<T>(" in text and "0x5851F42D4C957F2D" not in text
    assert "mc_adapted_radius<T>(" in basin and "mc_adapted_radius<T>(" in temper and "mc_exp<T>(" in basin and "mc_exp<T>(" in temper
    for routine in ("uint64_t pcg_advance(", "uint32_t pcg_extract(", "uint32_t pcg_draw(", "uint64_t pcg_jump(", "PcgMap pcg_jump_map(",
                    "T mc_adapted_radius(", "void pcg_normals("):
        assert pcg.count(routine) == 1, routine
    assert 'DZO_TIMED("basin_hopping_hop"' in basin and 'DZO_TIMED("basin_hopping_init"' in basin
    # hop and create enqueue only
    hop = basin[basin.index("int32_t dzo_basin_hopping_hop("):basin.index("int32_t dzo_basin_hopping_set_record(")]
    assert "Synchronize" not in hop
    assert "csrc/dzo_basin_hopping.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_basin_hopping_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_basin_hopping")
    assert {"dzo_basin_hopping_create", "dzo_basin_hopping_hop", "dzo_basin_hopping_read", "dzo_basin_hopping_destroy"} <= wanted
    assert wanted <= have, wanted - have
