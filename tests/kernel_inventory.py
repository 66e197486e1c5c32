"""The one table of the device kernels of the units built on dzo_pairwise.h and dzo_cluster.h, and what the build tests ask
of them in the gfx950 code object: every unit has exactly its kernels, in exactly its instantiations, and they are clean.  A
helper module like build_checks.py (no fixtures; imported by name).

A kernel is matched by its template name, never by a substring: the name llvm-cxxfilt of the ROCm llvm directory prints, or,
where that tool is not installed, the length-prefixed component of the mangled name (24quench_wave_step_kernel).  The template
arguments are read from the mangled name; the kernels here take an element type, at most one radial, and integers."""
import functools
import itertools
import os
import re
import subprocess

from build_checks import LLVM, kernel_metadata

ELEMENT_TYPES = ("f", "d")
RADIALS = ("LJ", "Morse6", "Morse14")                        # LJRadial<T>, MorseRadial<T, 6>, MorseRadial<T, 14>
R = "radial"
# unit (csrc/dzo_<unit>.hip) -> {kernel: the axes it is instantiated over behind the element type}: R for the radial, a tuple of
# values for an integer or bool parameter (HL, the mode of the pairwise kernels, the columns per lane of the alignment, the
# eigensolver's storage).  None: not a template.
UNITS = {
    "pairwise": {"pairwise_tile_kernel": (R, (0, 1, 2)), "pairwise_wave_kernel": (R, (0, 1, 2)), "pairwise_energy_delta_kernel": (R,),
                 "pairwise_finish_rows_kernel": (), "pairwise_finish_energy_kernel": None},
    "tempering": {"temper_wave_kernel": (R,), "temper_block_kernel": (R,), "swap_kernel": (R,), "analyze_kernel": ()},
    "lbfgs_batch": {"quench_wave_eval_kernel": (R,), "quench_block_eval_kernel": (R,), "quench_wave_step_kernel": (R,),
                    "quench_block_step_kernel": (R, (0, 1)), "quench_count_active_kernel": None},
    "adgd_batch": {"adgd_batch_wave_step_kernel": (R,), "adgd_batch_block_step_kernel": (R,), "adgd_batch_init_kernel": ()},
    "hessian_batch": {"hess_batch_wave_hvp_kernel": (R,), "hess_batch_block_hvp_kernel": (R,), "hess_batch_wave_hessian_kernel": (R,),
                      "hess_batch_block_hessian_kernel": (R,)},
    "basin_hopping": {"basin_hop_wave_kernel": (R,), "basin_hop_block_kernel": (R, (0, 1))},
    "lowmode": {"lowmode_wave_kernel": (R,), "lowmode_block_kernel": (R,)},
    "hybridef": {"hybridef_wave_step_kernel": (R,), "hybridef_block_step_kernel": (R,)},
    "modefollow": {"modefollow_step_kernel": (R,)},
    "neb": {"neb_wave_kernel": (R,), "neb_block_kernel": (R,), "neb_interp_kernel": ()},
    "structure": {"structfp_wave_kernel": (R,), "structfp_block_kernel": (R,), "structcmp_kernel": (), "structlabel_kernel": None},
    "symeig": {"symeig_jacobi_kernel": ((0, 1),)},
    "align": {"align_wave_kernel": ((1, 4, 16),), "align_finish_kernel": (), "align_assign_finish_kernel": None},
    "pathway": {"pathcand_count_kernel": (), "pathcand_wave_kernel": (), "pathcand_block_kernel": (), "pathcand_scan_kernel": None},
}
RADIAL_UNITS = [u for u, kernels in UNITS.items() if any(axes and R in axes for axes in kernels.values())]

_ARG = re.compile(r"NS_8LJRadialI([fd])EE|NS_11MorseRadialI([fd])Li(\d+)EEE|L[bi](\d+)E|([fd])")


def template_of_demangled(text):
    """`void dzo::swap_kernel<float, dzo::LJRadial<float>>(int, ...)` -> swap_kernel; None for a spelling this does not read
    (another return type, an anonymous namespace), which leaves the name to its mangled form"""
    m = re.match(r"(?:void )?(?:\w+::)*(\w+)[<(]", text)
    return m.group(1) if m else None


def decode(mangled, template=None):
    """(kernel, element type, radial, integers) of a mangled kernel name; the last three are None where the name is no template
    or takes arguments of another kind.  `template` is the demangled template name where a demangler gave one."""
    m = re.match(r"_ZN3dzo(\d+)", mangled)
    if not m:
        return (template or mangled, None, None, None)
    name = mangled[m.end():m.end() + int(m.group(1))]
    assert template in (None, name), (mangled, template)
    rest, pos, args = mangled[m.end() + len(name):], 1, []
    if not rest.startswith("I"):
        return (name, None, None, ())
    while rest[pos] != "E":
        a = _ARG.match(rest, pos)
        if not a:
            return (name, None, None, None)
        lj, morse, rho, integer, plain = a.groups()
        args.append(("LJ", lj) if lj else ("Morse" + rho, morse) if morse else int(integer) if integer else plain)
        pos = a.end()
    element, radial, integers = args[0], None, args[1:]
    if integers and isinstance(integers[0], tuple):          # the radial, of the kernel's element type
        radial, integers = integers[0][0] if integers[0][1] == element else "?", integers[1:]
    if element not in ELEMENT_TYPES or radial == "?" or not all(isinstance(a, int) for a in integers):
        return (name, None, None, None)
    return (name, element, radial, tuple(integers))


@functools.lru_cache(maxsize=None)
def code_object():
    """(metadata, {mangled name: decode(name)}) of every kernel of the built library"""
    meta = kernel_metadata()
    names, templates = sorted(meta), {}
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    if os.path.exists(tool):
        out = subprocess.run([tool], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
        templates = {n: template_of_demangled(d) for n, d in zip(names, out)}
    return meta, {n: decode(n, templates.get(n)) for n in names}


def expected(unit, radials=RADIALS):
    """the instantiations the table asks of `unit`, the radial kernels for `radials`"""
    out = set()
    for kernel, axes in UNITS[unit].items():
        if axes is None:
            out.add((kernel, None, None, ()))
            continue
        integers = [a for a in axes if a != R]
        for t, radial, *values in itertools.product(ELEMENT_TYPES, radials if R in axes else (None,), *integers):
            out.add((kernel, t, radial, tuple(values)))
    return out


def present(unit):
    """{instantiation: mangled name} of the kernels of the code object that carry a template name of `unit`"""
    return {inst: n for n, inst in code_object()[1].items() if inst[0] in UNITS[unit]}


def check_unit(unit, lj_count, vgpr_limit=None, morse_sgpr_clean=False):
    """`unit` has exactly its kernels: `lj_count` of them without the Morse radials, as many again for either Morse range.  None
    uses scratch memory or spills a vector register; none but a Morse instantiation keeps a scalar register in VGPR lanes (the
    fp64 Morse kernels of the cluster units hold the constants of exp in scalar registers: no memory traffic; reported, not
    refused), and with `morse_sgpr_clean` no Morse instantiation either."""
    meta, found = code_object()[0], present(unit)
    assert set(found) == expected(unit), sorted(set(found) ^ expected(unit), key=str)
    assert len(expected(unit, ("LJ",))) == lj_count, (unit, len(expected(unit, ("LJ",))))
    for inst, n in sorted(found.items(), key=str):
        print(n, meta[n])
        assert meta[n].get("private_segment_fixed_size", 0) == 0, (n, meta[n])
        assert meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
        if inst[2] in (None, "LJ") or morse_sgpr_clean:
            assert meta[n].get("sgpr_spill_count", 0) == 0, (n, meta[n])
        elif meta[n].get("sgpr_spill_count", 0):
            print("scalar registers kept in VGPR lanes:", inst, meta[n]["sgpr_spill_count"])
        if vgpr_limit is not None:
            assert meta[n].get("vgpr_count", 0) <= vgpr_limit, (n, meta[n])
