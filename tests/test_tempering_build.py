"""CPU-side checks of the parallel-tempering entry points: the library exports them, the Python table binds them, the
kernels exist for gfx950 without scratch memory or spills (the method of tests/test_pairwise_build.py), and the plain-C
example compiles and links against the library alone.  No compute here."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

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
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm llvm tools")
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(dzo.build(), os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        meta = {}
        for f in os.listdir(tmp):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", f], cwd=tmp, check=True,
                                   capture_output=True, text=True).stdout
            name = None
            for line in notes.splitlines():
                m = re.match(r"\s+\.name:\s+(\S+)", line)
                if m:
                    name = m.group(1)
                m = re.match(r"\s+\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", line)
                if m and name:
                    meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kernels = sorted(n for n in meta if re.search(r"temper_wave_kernel|temper_block_kernel|swap_kernel|analyze_kernel", n))
    assert len(kernels) >= 8, kernels
    for shape in ("temper_wave_kernel", "temper_block_kernel", "swap_kernel", "analyze_kernel"):
        for t in ("If", "Id"):
            assert any(shape + t in n for n in kernels), (shape, t, kernels)
    for n in kernels:
        assert meta[n].get("private_segment_fixed_size", 0) == 0, (n, meta[n])
        assert meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
        assert meta[n].get("sgpr_spill_count", 0) == 0, (n, meta[n])


def test_lj_tempering_example_compiles_and_links(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_tempering")
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_tempering.c"),
           "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    wanted = {l.split()[-1].split("@")[0] for l in out.splitlines() if " dzo_" in l}
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libdzo_hip.so")], check=True, capture_output=True,
                              text=True).stdout
    have = {l.split()[-1] for l in exported.splitlines()}
    assert {"dzo_tempering_create", "dzo_tempering_run", "dzo_tempering_analyze"} <= wanted and wanted <= have, wanted - have
