"""The whole-library statements about the device kernels of the units in tests/kernel_inventory.py: every unit has exactly its
kernels, no kernel belongs to two units, every radial kernel exists for all three radials in equal numbers, and no entry point
is a second name for a body another entry point runs.  The units' own build tests check their kernels' cleanliness."""
import re

import kernel_inventory as inv


def test_every_unit_has_exactly_its_kernels():
    """(how many that is per unit is pinned once, in the unit's own build test)"""
    for unit in inv.UNITS:
        assert set(inv.present(unit)) == inv.expected(unit), (unit, sorted(set(inv.present(unit)) ^ inv.expected(unit), key=str))


def test_no_kernel_belongs_to_two_units():
    names = [k for kernels in inv.UNITS.values() for k in kernels]
    assert len(names) == len(set(names))
    # ... nor ends like a streaming kernel that tests/test_abi.py guards by the tail of its name
    assert [k for k in names if re.search(r"(lbfgs_single_pass|lbfgs_point_pass|gram_pass_lanes|combine|batch_step)_kernel$", k)] == []
    owners = {}
    for unit in inv.UNITS:
        for mangled in inv.present(unit).values():
            assert owners.setdefault(mangled, unit) == unit, (mangled, owners[mangled], unit)
    assert len(owners) == sum(len(inv.expected(u)) for u in inv.UNITS)


def test_no_kernel_carries_a_rad_stem():
    """One entry point per kernel: the radials are template arguments of the kernel's one name."""
    templates = {inst[0] for inst in inv.code_object()[1].values()}
    assert [t for t in templates if t.startswith("rad_")] == [] and "swap_kernel" in templates


def test_every_radial_kernel_exists_for_all_three_radials_in_equal_numbers():
    assert len(inv.RADIAL_UNITS) == 11 and "symeig" not in inv.RADIAL_UNITS
    for unit in inv.RADIAL_UNITS:
        found = inv.present(unit)
        for kernel, axes in inv.UNITS[unit].items():
            for t in inv.ELEMENT_TYPES:
                per_radial = [sorted(i[3] for i in found if i[:3] == (kernel, t, radial)) for radial in inv.RADIALS]
                if axes and inv.R in axes:
                    assert per_radial[0] and per_radial[0] == per_radial[1] == per_radial[2], (unit, kernel, t, per_radial)
                else:
                    assert per_radial == [[], [], []], (unit, kernel, t, per_radial)


def test_names_are_matched_whole():
    """The decoder on spellings a substring would confuse: a type name in the argument list, a longer kernel name."""
    assert inv.decode("_ZN3dzo15neb_wave_kernelIdNS_8LJRadialIdEEEEvNS_7NebArgsIT_EE") == ("neb_wave_kernel", "d", "LJ", ())
    assert inv.decode("_ZN3dzo24quench_block_step_kernelIfNS_11MorseRadialIfLi14EEELb1EEEvNS_10QuenchArgsIT_EE") == \
        ("quench_block_step_kernel", "f", "Morse14", (1,))
    assert inv.decode("_ZN3dzo17align_wave_kernelIdLi16EEEvNS_9AlignArgsE") == ("align_wave_kernel", "d", None, (16,))
    assert inv.decode("_ZN3dzo26quench_count_active_kernelElPKiPl") == ("quench_count_active_kernel", None, None, ())
    assert inv.decode("_ZN3dzo11swap_kernelIdNS_8LJRadialIfEEEEviliPT_PKS3_PmPaS4_")[1:] == (None, None, None)   # a radial of another type
    assert inv.decode("_ZN3dzo11cast_kernelIdfEEvlPKT_PT0_")[1:] == (None, None, None)
    assert inv.template_of_demangled("void dzo::swap_kernel<float, dzo::LJRadial<float>>(int, long, int, float*)") == "swap_kernel"
    assert inv.template_of_demangled("dzo::structlabel_kernel(int, int, unsigned long long const*, int*, int*)") == "structlabel_kernel"
    assert inv.template_of_demangled("int dzo::(anonymous namespace)::k<float>(int)") is None      # left to the mangled name
