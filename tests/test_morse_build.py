"""CPU-side checks of the Morse radials: the header, the Python package and the Julia module agree on the selectors, 7 stays
unknown (and 1), every unit that dispatches on the radial carries gfx950 kernels for both Morse ranges and both element types (none of
them with scratch memory), and the plain-C example compiles and links against the library alone.  No compute here."""
import os
import re

from build_checks import kernel_metadata, link_example
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECTORS = {"LENNARD_JONES": 0, "MORSE_RHO6": 2, "MORSE_RHO14": 3}
# Per unit (csrc/dzo_<unit>.hip): the Lennard-Jones entry points and the entry points of the same bodies for the other radials.
UNITS = {"pairwise": {"pairwise_tile_kernel": "pairwise_tile_kernel", "pairwise_wave_kernel": "pairwise_wave_kernel",
                      "pairwise_energy_delta_kernel": "pairwise_energy_delta_kernel"},
         "tempering": {"temper_wave_kernel": "rad_temper_wave", "temper_block_kernel": "rad_temper_block", "swap_kernel": "rad_swap"},
         "lbfgs_batch": {"quench_wave_eval_kernel": "rad_quench_wave_eval", "quench_block_eval_kernel": "rad_quench_block_eval",
                         "quench_wave_step_kernel": "rad_quench_wave_step", "quench_block_step_kernel": "rad_quench_block_step"},
         "adgd_batch": {"adgd_batch_wave_step_kernel": "rad_adgdb_wave_step", "adgd_batch_block_step_kernel": "rad_adgdb_block_step"},
         "hessian_batch": {"hess_batch_wave_hvp_kernel": "rad_hessb_wave_hvp", "hess_batch_block_hvp_kernel": "rad_hessb_block_hvp",
                           "hess_batch_wave_hessian_kernel": "rad_hessb_wave_hessian", "hess_batch_block_hessian_kernel": "rad_hessb_block_hessian"},
         "lowmode": {"lowmode_wave_kernel": "rad_lowm_wave", "lowmode_block_kernel": "rad_lowm_block"},
         "structure": {"structfp_wave_kernel": "rad_sfp_wave", "structfp_block_kernel": "rad_sfp_block"},
         "basin_hopping": {"basin_hop_wave_kernel": "rad_bhop_wave", "basin_hop_block_kernel": "rad_bhop_block"},
         "modefollow": {"modefollow_step_kernel": "rad_mfollow_step"},
         "hybridef": {"hybridef_wave_step_kernel": "rad_hybef_wave_step", "hybridef_block_step_kernel": "rad_hybef_block_step"},
         "neb": {"neb_wave_kernel": "rad_band_wave", "neb_block_kernel": "rad_band_block"}}


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
    Lennard-Jones twins, with no private segment (scratch) and no VGPR spill.  The Lennard-Jones entry points are instantiated
    for Lennard-Jones only.  (The fp64 Morse kernels keep the constants of exp in scalar registers and move some of those to
    VGPR lanes; that costs no memory traffic and is reported, not refused.)"""
    meta = kernel_metadata()
    moved = {}
    for unit, kernels in UNITS.items():
        for lj, rad in kernels.items():
            for t in ("f", "d"):
                # (the Lennard-Jones kernels of three units are templates of the element type alone)
                twins = [n for n in meta if lj in n and ("8LJRadialI%sE" % t in n or "%sI%sE" % (lj, t) in n)]
                assert len(twins) >= 1, (unit, lj, t)
                for rho in (6, 14):
                    tag = "11MorseRadialI%sLi%dEE" % (t, rho)
                    hits = [n for n in meta if rad in n and tag in n]
                    assert len(hits) == len(twins), (unit, rad, t, rho, hits, twins)
                    if rad != lj:
                        assert [n for n in meta if lj in n and tag in n] == [], (unit, lj)
                        assert [n for n in meta if rad in n and "LJRadial" in n] == [], (unit, rad)
                    for n in hits:
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
