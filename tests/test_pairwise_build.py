"""CPU-side checks of the pairwise radial (Lennard-Jones) objective: the library exports its entry points, the Python
table binds them, its kernels exist for gfx950 without scratch memory or spills, and the plain-C example compiles and
links against the library alone.  No compute here."""
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
SYMBOLS = ["dzo_pairwise_energy", "dzo_pairwise_gradient", "dzo_pairwise_hvp", "dzo_pairwise_energy_delta", "dzo_calibrate_fma_rate"]


def test_library_exports_the_pairwise_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert lib.dzo_version() == 100


def test_python_constants_and_functions():
    assert dzo.PAIRWISE_LJ == 5 and dzo.RADIAL_LENNARD_JONES == 0
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    assert re.search(r"#define\s+DZO_PROBLEM_PAIRWISE_LJ\s+5\b", header)
    assert re.search(r"#define\s+DZO_RADIAL_LENNARD_JONES\s+0\b", header)
    for f in ("pairwise_radial_energy", "pairwise_radial_gradient_", "pairwise_radial_hvp_", "pairwise_radial_energy_delta",
              "calibrate_fma_rate"):
        assert callable(getattr(dzo, f))


def test_pairwise_kernels_exist_for_gfx950_without_scratch():
    """Four entries x two element types is the fewest there can be; every one of them keeps its accumulators in registers:
    no private segment, no VGPR or SGPR spill."""
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
    kernels = sorted(n for n in meta if "pairwise" in n)
    assert len(kernels) >= 8, kernels
    for shape in ("pairwise_tile_kernel", "pairwise_wave_kernel", "pairwise_energy_delta_kernel"):
        for t in ("If", "Id"):
            assert any(shape + t in n for n in kernels), (shape, t, kernels)
    for n in kernels:
        assert meta[n].get("private_segment_fixed_size", 0) == 0, (n, meta[n])
        assert meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
        assert meta[n].get("sgpr_spill_count", 0) == 0, (n, meta[n])


def test_lj_cluster_example_compiles_and_links(tmp_path):
    dzo.build()
    exe = str(tmp_path / "lj_cluster")
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lj_cluster.c"),
           "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    wanted = {l.split()[-1].split("@")[0] for l in out.splitlines() if " dzo_" in l}
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libdzo_hip.so")], check=True, capture_output=True,
                              text=True).stdout
    have = {l.split()[-1] for l in exported.splitlines()}
    assert {"dzo_pairwise_energy", "dzo_problem_create", "dzo_lbfgs_step"} <= wanted and wanted <= have, wanted - have
