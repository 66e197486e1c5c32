"""CPU-side checks of the Morse radials: the header, the Python package and the Julia module agree on the selectors, 7 stays
unknown (and 1), every unit that dispatches on the radial carries gfx950 kernels for both Morse ranges and both element types (none of
them with scratch memory), and the plain-C example compiles and links against the library alone.  No compute here."""
import os
import re

import kernel_inventory as inv
from build_checks import link_example
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECTORS = {"LENNARD_JONES": 0, "MORSE_RHO6": 2, "MORSE_RHO14": 3}
UNITS = inv.RADIAL_UNITS                                     # every unit (csrc/dzo_<unit>.hip) with a kernel that takes a radial


def test_header_python_and_julia_agree_on_the_selectors():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    julia = open(os.path.join(ROOT, "dzoptimization.jl_amd", "julia", "DZOptimizationAMD.jl")).read()
    for name, value in SELECTORS.items():
        assert re.search(r"#define\s+DZO_RADIAL_%s\s+%d\b" % (name, value), header), name
        assert re.search(r"const DZO_RADIAL_%s = Cint\(%d\)" % (name, value), julia), name
        assert getattr(dzo, "RADIAL_" + name) == value


def test_one_and_seven_are_not_selectors():
    """The error-code tests of the units pass 7 and (tests/test_gpu_structure.py) 1 as unknown radials."""
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    values = [int(v) for v in re.findall(r"#define\s+DZO_RADIAL_\w+\s+(\d+)", header)]
    assert sorted(values) == [0, 2, 3], values
    assert sorted(v for k, v in vars(dzo).items() if k.startswith("RADIAL_")) == [0, 2, 3]


def test_julia_passes_no_radial_literal():
    """Every ccall takes the function's `radial` keyword; the Lennard-Jones constant appears only as its default."""
    julia = open(os.path.join(ROOT, "dzoptimization.jl_amd", "julia", "DZOptimizationAMD.jl")).read()
    assert not re.search(r"DZO_RADIAL_LENNARD_JONES, [a-z]", julia)                  # (the export list names the constant, too)
    assert len(re.findall(r"radial::Integer=DZO_RADIAL_LENNARD_JONES", julia)) == len(re.findall(r"^\s+Cint\(radial\),", julia, re.M)) >= 19


def test_every_radial_unit_has_morse_kernels_without_scratch():
    """Every kernel that takes a radial exists for both Morse ranges and both element types, as many of them as there are
    Lennard-Jones twins, with no private segment (scratch) and no VGPR spill.  (The fp64 Morse kernels keep the constants of
    exp in scalar registers and move some of those to VGPR lanes; that costs no memory traffic and is reported, not refused.)"""
    meta, moved = inv.code_object()[0], {}
    for unit in UNITS:
        found = inv.present(unit)
        for kernel, axes in inv.UNITS[unit].items():
            for t in inv.ELEMENT_TYPES if axes and inv.R in axes else ():
                twins = [i for i in found if i[:3] == (kernel, t, "LJ")]
                assert len(twins) >= 1, (unit, kernel, t)
                for rho in (6, 14):
                    hits = [i for i in found if i[:3] == (kernel, t, "Morse%d" % rho)]
                    assert sorted(i[3] for i in hits) == sorted(i[3] for i in twins), (unit, kernel, t, rho, hits, twins)
                    for n in (found[i] for i in hits):
                        assert meta[n].get("private_segment_fixed_size", 0) == 0 and meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
                        if meta[n].get("sgpr_spill_count", 0):
                            moved[n] = meta[n]["sgpr_spill_count"]
    print("scalar registers kept in VGPR lanes:", {k.split("NS_")[0][7:]: v for k, v in sorted(moved.items())})


def test_one_table_of_radials():
    """The one table of (radial, dtype) -> (T, F) is in dzo_pairwise.h; no .hip names MorseRadial, and every unit that launches
    with a radial goes through the table."""
    csrc = os.path.join(ROOT, "dzoptimization.jl_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            assert "MorseRadial" not in open(os.path.join(csrc, f)).read(), f
    header = open(os.path.join(csrc, "dzo_pairwise.h")).read()
    assert header.count("#define DZO_RADIAL_CASES_(") == 1 and header.count("MorseRadial<T, 6>") == 1 and header.count("MorseRadial<T, 14>") == 1
    for unit in UNITS:
        text = open(os.path.join(csrc, "dzo_%s.hip" % unit)).read()
        assert "DZO_DISPATCH_RADIAL" in text or "DZO_RADIAL_CASES_" in text, unit


def test_morse_quench_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "morse_quench")
    assert {"dzo_lbfgs_batch_create", "dzo_pairwise_batch_hessian", "dzo_symmetric_batch_eigen"} <= wanted and wanted <= have, wanted - have
