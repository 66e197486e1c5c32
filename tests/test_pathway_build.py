"""CPU-side checks of the candidate unit (the method of tests/test_align_build.py): the library exports the entry point, the
Python table and the Julia module bind it with the header's arity, the constants match the header, the header block sits behind
the alignment block and states its rule, the kernels exist for gfx950 in both launch shapes and both element types without
scratch memory or spills, the source takes its sums from the shared headers, and the plain-C example compiles and links against the library alone.  No
compute here."""
import ctypes
import os
import re

from build_checks import link_example
from kernel_inventory import check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = {"dzo_pathway_batch_candidates": 14}
CONSTANTS = dict(PATHWAY_MAX_PARTICLES=1024, PATHWAY_MAX_IMAGES=32, PATHWAY_MAX_BATCH=1048576, PATHWAY_OVERFLOW=7)
BANNED_TITLES = ("Batched LBFGSOptimizer", "Batched AdGDOptimizer", "Batched basin hopping", "Batched Hessian-vector products and dense Hessians",
                 "Batched symmetric eigensolver", "Batched eigenvector following", "Batched lowest Hessian mode",
                 "Batched hybrid eigenvector following", "Structure fingerprints and their classification", "Batched nudged elastic band",
                 "Batched rigid and permutational alignment")


def _header():
    return open(os.path.join(ROOT, "include", "dzo.h")).read()


def _header_arity(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
    return params.count(",") + 1


def test_library_exports_the_entry_point_and_both_hosts_bind_it():
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
    abi = dzo.ABI["dzo_pathway_batch_candidates"]
    assert abi[0] is ctypes.c_int64 and abi[1] is ctypes.c_int32 and abi[6] is ctypes.c_int64      # n_particles, n_images, capacity
    assert abi[13] is ctypes.POINTER(ctypes.c_int64)                                              # the count, on the host
    exports = julia[julia.index("export "):julia.index("const libdzo")]
    for name in ("band_candidates", "PATHWAY_MAX_BATCH", "PATHWAY_OVERFLOW"):
        assert name in exports, name
    assert re.search(r"^function band_candidates\(", julia, flags=re.M)
    for name, value in CONSTANTS.items():
        assert re.search(r"\b%s\b" % name, julia) and str(value) in julia, name
    assert "connect_pathways" not in exports                 # the cycle is Python only


def test_python_constants_match_the_header():
    header = _header()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, header).group(1))
    for name, expected in CONSTANTS.items():
        assert getattr(dzo, name) == value("DZO_" + name) == expected and type(getattr(dzo, name)) is int, name
    defines = set(re.findall(r"^#define[ \t]+DZO_(PATHWAY_\w+)", header, flags=re.M))
    assert defines == set(CONSTANTS) == {k for k in vars(dzo) if k.startswith("PATHWAY_")}
    assert value("DZO_VERSION") == 100
    assert dzo.PATHWAY_MAX_PARTICLES == dzo.NEB_MAX_PARTICLES and dzo.PATHWAY_MAX_IMAGES == dzo.NEB_MAX_IMAGES
    assert dzo.PATHWAY_OVERFLOW in dzo._ERR and dzo.PATHWAY_OVERFLOW not in (0, 1, 2, 3, 4, 5, 6)
    assert dzo.PATHWAY_MAX_BATCH * ((dzo.PATHWAY_MAX_IMAGES - 1) // 2) < 2 ** 31     # the offsets are int32
    assert "include/dzo.h" in dzo.band_candidates.__doc__


def test_header_block_is_in_place_and_states_the_rule():
    header = _header()
    start = header.index("Transition-state candidates of many bands")
    end = header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")
    assert header.index("Batched rigid and permutational alignment") < header.index("int32_t dzo_align_batch_pairs(") < start < end
    assert header.count("Transition-state candidates of many bands") == 1
    block = header[start:end]
    for banned in BANNED_TITLES:
        assert banned not in block, banned
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("Carr, Trygubenko & Wales 2005", "this block is the specification", "there is no `radial`",
                   "image m of band b sits at element 3N (M b + m)", "energies_dev is (M, batch) in T", "Neither is changed",
                   "DZO_PATHWAY_MAX_PARTICLES = 1024", "DZO_PATHWAY_MAX_IMAGES = 32", "DZO_PATHWAY_MAX_BATCH = 1048576",
                   "a candidate iff E_m > E_{m-1} and E_m >= E_{m+1}", "plain comparisons in T", "yields its first image only",
                   "E_m == E_{m-1} is no candidate", "a NaN on either side of a comparison yields nothing", "the ends are never candidates",
                   "at most (M - 1) / 2 candidates", "band-major, the image index ascending inside a band",
                   "offsets_dev[batch] the count", "points_dev row c = x_m, copied", "candidate_energies_dev[c] = E_m, copied",
                   "d+ = x_{m+1} - x_m and d- = x_m - x_{m-1}", "If E_{m+1} > E_m > E_{m-1}: t = d+", "If E_{m+1} < E_m < E_{m-1}: t = d-",
                   "a = max(|E_{m+1} - E_m|, |E_{m-1} - E_m|)", "t_e = fma(a, d+_e, b d-_e) if E_{m+1} > E_{m-1}", "t_e = fma(b, d+_e, a d-_e)",
                   "tau_e = T(t_e / sqrt(t.t))", "a product and two fused multiply-adds", "the wave tree", "the four waves in wave order",
                   "bit for bit the tangent dzo_neb_batch_apply records", "gives the same NaN row",
                   "are not written", "offsets_dev and *count are complete all the same", "returns DZO_PATHWAY_OVERFLOW = 7",
                   "With capacity == 0 the five arrays may be NULL", "three on one stream and one host wait at the end",
                   "One thread per band counts", "ONE 256-thread block", "per = ceil(batch / 256)", "any batch up to the bound is one pass",
                   "One 256-thread block per band", "candidate k goes to wave k mod 4", "lane i holds particle i", "t, t + 256",
                   "No read-modify-write on memory", "one writer per element", "every loop is bounded by an argument",
                   "the same bits alone or anywhere in any batch", "The call blocks", "Out of scope: evaluating the band",
                   "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_candidate_kernels_exist_for_gfx950_without_scratch():
    """The count, the two shapes of the writing kernel in both element types and the one scan: no private segment, no VGPR or
    SGPR spill, no more than 512 vector registers."""
    check_unit("pathway", lj_count=7, vgpr_limit=512)


def test_the_source_keeps_to_its_rules():
    src = open(os.path.join(PKG, "csrc", "dzo_pathway.hip")).read()
    assert '#include "dzo_cluster.h"' in src and '#include "dzo_neb' not in src
    for word in ("cl_dot3(", "cl_block_sum(", "wave_sum_all(", "cl_check_args(", "cl_abs(", "dfma<T>(", "require_same_backend(",
                 'DZO_TIMED("pathway_candidates"', "DZO_PATHWAY_MAX_BATCH", "DZO_PATHWAY_OVERFLOW", "__launch_bounds__(kBlock)"):
        assert word in src, word
    for word in ("atomic", "printf(", "asm", "__shfl", "while (", "radial,", "device_alloc(", "hipMalloc"):
        assert word not in src, word
    # every loop of the kernels counts up to a bound: no loop condition reads a floating-point value
    for loop in re.findall(r"for \(([^)]*)\)", src[:src.index('extern "C"')]):
        assert re.match(r"(int|int64_t) \w+ = ", loop), loop
    # three launches and one host wait
    entry = src[src.index("int32_t dzo_pathway_batch_candidates("):]
    assert entry.count("hipLaunchKernelGGL(") == 4 and entry.count("pathcand_count_kernel") == 1 and entry.count("pathcand_scan_kernel") == 1
    assert entry.count("Synchronize") == 1 and "dim3(1), dim3(kBlock)" in entry
    assert "csrc/dzo_pathway.hip" in open(os.path.join(PKG, "Makefile")).read()
    # the band unit is what it was: the tangent is restated here, not moved
    neb = open(os.path.join(PKG, "csrc", "dzo_neb.hip")).read()
    assert "pathcand" not in neb and "dzo_pathway" not in neb


def test_lj_connect_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_connect")
    assert {"dzo_pathway_batch_candidates", "dzo_neb_batch_interpolate", "dzo_neb_batch_create", "dzo_neb_batch_step", "dzo_neb_batch_get_ptr",
            "dzo_hybridef_batch_create", "dzo_hybridef_batch_step", "dzo_lbfgs_batch_step"} <= wanted and wanted <= have, wanted - have
    src = open(os.path.join(ROOT, "examples", "lj_connect.c")).read()
    assert "candidate" in src and "band" in src and "image" in src
