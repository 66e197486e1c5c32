"""CPU-side checks of the Thomson unit (csrc/dzo_sphere.hip): the library exports its entry points, the Python table binds
them, the header cites the reference, its kernels -- exactly the expected set, every name starting with sphere_ -- exist for
gfx950 without scratch memory or spills, the Riesz functor stays inside them, and the plain-C example compiles and links against
the library alone.  No compute here.  (The units table of tests/kernel_inventory.py is about the radial units and stays as it
is; this file reads the code object through it.)"""
import ctypes
import itertools
import os
import re

import kernel_inventory as inv
from build_checks import link_example
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
HANDLE = ["create", "destroy", "set_max_halvings", "step", "count_active", "get_ptr", "read"]
SYMBOLS = ["dzo_sphere_batch_project", "dzo_sphere_batch_energy_gradient"] + ["dzo_sphere_lbfgs_batch_" + f for f in HANDLE]
# template name -> the integer axes behind the element type
KERNELS = {"sphere_project_kernel": (), "sphere_wave_eval_kernel": (), "sphere_block_eval_kernel": (), "sphere_wave_quench_kernel": (),
           "sphere_block_quench_kernel": ((0, 1),)}
GUARDED_STEMS = ("batch_step_kernel", "combine_kernel", "gram_pass_lanes_kernel", "lbfgs_single_pass_kernel", "lbfgs_point_pass_kernel")


def test_library_exports_the_sphere_entry_points():
    lib = ctypes.CDLL(dzo.build())
    assert [n for n in SYMBOLS if not hasattr(lib, n)] == []
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert dzo.ABI["dzo_sphere_lbfgs_batch_create"] == dzo.ABI["dzo_lbfgs_batch_create"]     # _ClusterHandle._create serves both


def test_python_binds_the_unit():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    m = re.search(r"#define\s+DZO_SPHERE_ENERGY_RIESZ1\s+(\d+)\b", header)
    assert m and dzo.SPHERE_ENERGY_RIESZ1 == int(m.group(1)) == 0
    assert len(re.findall(r"#define\s+DZO_SPHERE_", header)) == 1               # the what constants and limits are DZO_LBFGS_BATCH_*
    for name in ("sphere_project_", "sphere_energy_gradient", "SphereLBFGS"):
        assert callable(getattr(dzo, name)) and name in dzo.__all__, name
    assert issubclass(dzo.SphereLBFGS, dzo._BatchedOptimizer) and dzo.SphereLBFGS._prefix == "dzo_sphere_lbfgs_batch_"
    assert dzo.SphereLBFGS._what is dzo.BatchedLBFGS._what and dzo.SphereLBFGS._shape is dzo.BatchedLBFGS._shape      # shared
    for f in ("step", "count_active", "read", "set_max_halvings"):
        assert callable(getattr(dzo.SphereLBFGS, f))
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    for name in SYMBOLS:
        assert "ccall((:%s, libdzo)" % name in julia, name
    for name in ("sphere_project!", "sphere_energy_gradient", "SphereLBFGS"):
        assert name in julia, name


def test_header_cites_the_reference_for_every_entry():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    block = header[header.index("The Thomson problem"):header.index("dzo_sphere_lbfgs_batch_read(")]
    for needle in ("legacy/ExampleFunctions.jl", ":30-45", ":47-83", ":361-374", ":133-135", ":412-414", ":454-509", ":381-387", ":62",
                   "inv_dist_cubed", "(3, N)", "x / r, y / r, z / r", "overlap = x gx + y gy + z gz", "unfused",
                   "ships the gradient constraint but NOT the", "normalisation is ours", "DZO_LBFGS_BATCH_MAX_PARTICLES"):
        assert needle in block, needle
    for name in SYMBOLS:
        assert re.search(r"int32_t %s\(" % name, header), name


def _sphere_kernels():
    meta, decoded = inv.code_object()
    return meta, {n: inst for n, inst in decoded.items() if inst[0].startswith("sphere_")}


def test_sphere_kernels_are_exactly_the_expected_set_without_scratch_or_spills():
    meta, found = _sphere_kernels()
    expected = set()
    for kernel, axes in KERNELS.items():
        for t, *values in itertools.product(inv.ELEMENT_TYPES, *axes):
            expected.add((kernel, t, None, tuple(values)))
    assert set(found.values()) == expected, sorted(set(found.values()) ^ expected, key=str)
    assert len(found) == len(expected) == 12
    for n, inst in sorted(found.items()):
        print(n, meta[n])
        assert meta[n].get("private_segment_fixed_size", 0) == 0, (n, meta[n])
        assert meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
        assert meta[n].get("sgpr_spill_count", 0) == 0, (n, meta[n])


def test_names_keep_clear_of_the_guarded_stems_and_the_functor_stays_inside():
    _, decoded = inv.code_object()
    for n, inst in decoded.items():
        if inst[0].startswith("sphere_"):
            assert not any(stem in n for stem in GUARDED_STEMS) and not inst[0].startswith("rad_"), n
        else:
            assert "RieszRadial" not in n, n                    # ... and no kernel of another unit is instantiated for it
    # the table of the radial units does not know the unit, and none of its kernels is a sphere kernel
    assert not any(k.startswith("sphere_") for kernels in inv.UNITS.values() for k in kernels)
    # in the sources: the functor is named by the unit alone, never by the dispatch table
    for f in os.listdir(os.path.join(PKG, "csrc")):
        text = open(os.path.join(PKG, "csrc", f)).read()
        if f not in ("dzo_sphere.hip", "dzo_pairwise.h"):
            assert "RieszRadial" not in text, f
    pairwise = open(os.path.join(PKG, "csrc", "dzo_pairwise.h")).read()
    table = pairwise[pairwise.index("#define DZO_RADIAL_CASES_"):pairwise.index("#define DZO_DISPATCH_RADIAL")]
    assert "Riesz" not in table and table.count("else if") == 2


def test_source_is_built_on_the_shared_pieces():
    src, quench, core, args = (open(os.path.join(PKG, "csrc", f)).read() for f in ("dzo_sphere.hip", "dzo_lbfgs_batch.hip", "dzo_quench_core.h",
                                                                              "dzo_quench_args.h"))
    assert "qc_wave_run<T, RieszRadial<T>, QcUnitSphere>(" in src and "qc_block_run<T, RieszRadial<T>, QcUnitSphere>(" in src
    assert "typename C = QcFree" in core and core.count("struct QcUnitSphere") == 1 and core.count("struct QcFree") == 1
    for piece in ("QuenchArgs<T>", "qa_args<T>(", "qa_alloc(", "qa_array", "qa_free("):
        assert piece in src and piece in quench, piece          # one copy of the arguments, of the handle, its layout and its table
    assert "struct QuenchArgs" in args and "struct QuenchArgs" not in src + quench and "struct QaHandle" in args
    for piece in ("qa_wave_load<T>(", "qa_wave_store<T>(", "qa_block_load<T>(", "qa_block_store<T>("):
        assert piece in src and args.count(piece.replace("<T>(", "(")) == 1, piece    # the unit's kernels are load -> run -> store
    assert "__global__" not in args and "__shared__" not in args
    for text in (src, args):                                    # behind the opening comment: no atomic of any kind
        assert "atomic" not in text.split("namespace dzo {", 1)[1]
    assert "F::energy(" not in src and "F::first(" not in src and "cl_count" in src
    assert "csrc/dzo_sphere.hip" in open(os.path.join(PKG, "Makefile")).read()


def test_thomson_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "thomson_quench")
    assert {"dzo_sphere_batch_project", "dzo_sphere_lbfgs_batch_create", "dzo_sphere_lbfgs_batch_step", "dzo_sphere_lbfgs_batch_read"} <= wanted
    assert wanted <= have, wanted - have
