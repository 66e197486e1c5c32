"""CPU-side checks of the alignment unit (the method of tests/test_structure_build.py): the library exports the two entry
points, the Python table and the Julia module bind them with the header's arity, the constants match the header, the header
block sits behind the nudged-elastic-band block and states its rule, the kernels exist for gfx950 in the three column-per-lane
instantiations and both element types without scratch memory or spills, and the plain-C example compiles and links against the library alone.  No
compute here."""
import ctypes
import inspect
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = {"dzo_align_batch_assign": 7, "dzo_align_batch_pairs": 18}
CONSTANTS = dict(ALIGN_MAX_PARTICLES=1024, ALIGN_MAX_RANDOM_TRIALS=64, ALIGN_MAX_CYCLES=64, ALIGN_TRIAL_IDENTITY=1, ALIGN_TRIAL_PRINCIPAL=2,
                 ALIGN_CONVERGED=0, ALIGN_CYCLE_LIMIT=1, ALIGN_FAILED=2)
BANNED_TITLES = ("Batched LBFGSOptimizer", "Batched AdGDOptimizer", "Batched basin hopping", "Batched Hessian-vector products and dense Hessians",
                 "Batched symmetric eigensolver", "Batched eigenvector following", "Batched lowest Hessian mode",
                 "Batched hybrid eigenvector following", "Structure fingerprints and their classification", "Batched nudged elastic band")


def _header():
    return open(os.path.join(ROOT, "include", "dzo.h")).read()


def _header_arity(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
    return params.count(",") + 1


def test_library_exports_the_entry_points_and_both_hosts_bind_them():
    lib = ctypes.CDLL(dzo.build())
    header = _header()
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if not hasattr(lib, n)] == []
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    for name, expected in SYMBOLS.items():
        arity = _header_arity(header, name)
        assert arity == expected and len(dzo.ABI[name]) == arity, name
        calls = list(re.finditer(r"ccall\(\(:%s, libdzo\), Cint,\s*\(" % name, julia))
        assert calls, name
        for m in calls:                                      # the argument-type tuple of every literal ccall
            depth, i = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(julia[i], 0)
                i += 1
            types = [t for t in re.sub(r"\{[^}]*\}", "", julia[m.end():i - 1]).split(",") if t.strip()]
            assert len(types) == arity, (name, types)
    assert dzo.ABI["dzo_align_batch_pairs"][9] is ctypes.c_uint64                 # the seed
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    for name in ("assign_particles", "align_pairs", "ALIGN_TRIAL_PRINCIPAL", "ALIGN_FAILED"):
        assert name in exports, name
    for name in ("assign_particles", "align_pairs"):
        assert re.search(r"^function %s\(" % name, julia, flags=re.M), name
    connect = julia[julia.index("function connect_minima("):]
    assert "align=false" in connect[:connect.index(") where")] and "align_pairs(a, b, n_particles" in connect
    for name, value in CONSTANTS.items():
        assert re.search(r"\b%s\b" % name, julia), name


def test_python_constants_and_signatures_match_the_header():
    header = _header()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    for name, expected in CONSTANTS.items():
        assert getattr(dzo, name) == value("DZO_" + name) == expected and type(getattr(dzo, name)) is int, name
    defines = set(re.findall(r"^#define[ \t]+DZO_(ALIGN_\w+)", header, flags=re.M))
    assert defines == set(CONSTANTS) == {k for k in vars(dzo) if k.startswith("ALIGN_")}
    assert value("DZO_VERSION") == 100
    for name in ("assign_particles", "align_pairs", "Alignment"):
        assert name in dzo.__all__, name
    sig = inspect.signature(dzo.connect_minima).parameters
    assert list(sig)[:5] == ["a", "b", "n_particles", "n_images", "force_tol"] and sig["force_tol"].default is inspect.Parameter.empty
    assert sig["align"].default is False and list(sig)[-1] == "band_options"
    assert inspect.signature(dzo.align_pairs).parameters["trials"].default == dzo.ALIGN_TRIAL_IDENTITY | dzo.ALIGN_TRIAL_PRINCIPAL
    assert "align_pairs" in dzo.connect_minima.__doc__ and "include/dzo.h" in dzo.align_pairs.__doc__


def test_header_block_is_in_place_and_states_the_rule():
    header = _header()
    start = header.index("Batched rigid and permutational alignment")
    end = header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("Batched nudged elastic band") < header.index("int32_t dzo_neb_batch_read(") < start < end
    assert header.count("Batched rigid and permutational alignment") == 1
    block = header[start:end]
    for banned in BANNED_TITLES:
        assert banned not in block, banned
    # the band block keeps its own sentence; this block says that it supplies what that sentence excludes
    assert "Out of scope: alignment of arbitrary end pairs" in header[header.index("Batched nudged elastic band"):start]
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("minpermdist", "\"alignment of arbitrary end pairs\" out of scope: this block supplies it", "this block is the specification",
                   "there is no `radial`", "DZO_ALIGN_MAX_PARTICLES = 1024", "DZO_ALIGN_MAX_RANDOM_TRIALS = 64", "DZO_ALIGN_MAX_CYCLES = 64",
                   "All arithmetic below is fp64", "do not depend on the element type beyond the input values",
                   "THE ORDER OF EVERY SUM", "lane j mod 64", "offsets 32, 16, 8, 4, 2, 1",
                   "c(i, j) = fma(dz, dz, fma(dy, dy, dx dx))", "No N x N matrix is stored", "shortest augmenting path",
                   "Rows are taken in index order", "at most N + 1 times", "cur = (c(i0, j) - u[i0]) - v[j]", "the lowest column that has it",
                   "stop when j1 has no row", "cost_dev = sum_i c(i, p(i))",
                   "the identity, if trials has DZO_ALIGN_TRIAL_IDENTITY", "the four principal ones, if it has DZO_ALIGN_TRIAL_PRINCIPAL",
                   "n_starts = (allow_inversion ? 2 : 1) n_orient", "eigenvalue ascending, equal ones by index",
                   "the third is negated if the determinant is negative", "(+,+,+), (+,-,-), (-,+,-), (-,-,+)",
                   "PCG32 XSH-RR", "state = A (C + seed) + C", "jumped ahead by 4 r draws for random trial r",
                   "a pair draws the same numbers alone or anywhere in a batch", "u_m = (d_m + 1/2) 2^-32", "four standard normals",
                   "Horn's rotation", "S_uv = sum b_p(i).u a_i.v", "H00 = (Sxx + Syy) + Szz", "H23 = Syz + Szy",
                   "the largest eigenvalue (the first among equals)", "DZO_ALIGN_CONVERGED when a cycle's permutation is the previous cycle's",
                   "DZO_ALIGN_CYCLE_LIMIT after max_cycles cycles", "at most 12 sweeps", "theta = (M_qq - M_pp) / (M_pq + M_pq)",
                   "N = 1 and N = 2 give rank-deficient matrices and finite answers",
                   "the smallest distance, the first in index order among equals", "rounded once to T", "det = +-1", "may be NULL",
                   "detected before any loop runs", "status DZO_ALIGN_FAILED, the identity permutation, aligned = b",
                   "one wave per (pair, start)", "1, 4 and 16 columns per lane", "38 N + 8 bytes", "38 920 at N = 1024",
                   "four waves per compute unit of 160 KiB", "waits for no other wave", "No floating-point atomics",
                   "every output element is written once", "every loop is bounded by a count known at entry", "no NaN can keep one alive",
                   "the same bits alone or anywhere in any batch", "Both calls block",
                   "Out of scope: several atom species", "point-group symmetry detection", "a guarantee of the global minimum",
                   "a multi-start local one", "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT", "DZO_ERR_NOMEM"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_align_kernels_exist_for_gfx950_without_scratch():
    """Three column-per-lane instantiations and the finish kernel in both element types, one finish kernel of the assignment:
    no private segment, no VGPR or SGPR spill, no more than 512 vector registers."""
    check_unit("align", lj_count=9, vgpr_limit=512)


def test_the_source_keeps_to_its_rules():
    src = open(os.path.join(PKG, "csrc", "dzo_align.hip")).read()
    for include in ('#include "dzo_common.h"', '#include "dzo_pcg.h"'):
        assert include in src, include
    for word in ("wave_sum_all(", "lane_xor1(", "lane_xor8(", "permlane16_swap", "permlane32_swap", "pcg_jump(", "pcg_draw(", "device_alloc(",
                 "require_same_backend(", 'DZO_TIMED("align_starts"', 'DZO_TIMED("align_finish"', 'DZO_TIMED("align_assign"', "__launch_bounds__(64)"):
        assert word in src, word
    for word in ("atomic", "printf(", "asm", "__shfl", "while ("):
        assert word not in src, word
    # every loop of the kernels counts up to a bound: no loop condition reads a floating-point value
    for loop in re.findall(r"for \(([^)]*)\)", src[:src.index("host side")]):
        assert re.match(r"(int|int64_t) \w+ = ", loop), loop
    assert "csrc/dzo_align.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_lj_align_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_align")
    assert {"dzo_align_batch_pairs", "dzo_neb_batch_interpolate", "dzo_neb_batch_create", "dzo_neb_batch_step", "dzo_neb_batch_read",
            "dzo_tempering_run", "dzo_lbfgs_batch_step"} <= wanted and wanted <= have, wanted - have
    src = open(os.path.join(ROOT, "examples", "lj_align.c")).read()
    assert "raw centred distance" in src and "aligned distance" in src and "barrier" in src
