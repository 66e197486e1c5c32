"""What the CPU-side build tests ask of the built library: the metadata of its gfx950 kernels, and a plain-C example linked
against it with gcc alone.  A helper module like the *_twin.py files (no fixtures; imported by name)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = "vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count|sgpr_count"


def kernel_metadata():
    """{kernel name: {vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size, vgpr_count, sgpr_count}} of the gfx950
    code object of the built library (a field the notes do not carry is absent).  Skips without the ROCm llvm tools."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no ROCm llvm tools")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(dzo.build(), os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in os.listdir(tmp):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=tmp, check=True,
                                   capture_output=True, text=True).stdout
            name = None
            for line in notes.splitlines():
                m = re.match(r"\s+\.name:\s+(\S+)", line)
                if m:
                    name = m.group(1)
                m = re.match(r"\s+\.(%s):\s+(\d+)" % FIELDS, line)
                if m and name:
                    meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return meta


def link_example(tmp_path, name):
    """Compiles examples/<name>.c with gcc against the built library.  Returns (exe, wanted, have): the program, the dzo_*
    symbols it leaves undefined, and the symbols the library defines."""
    dzo.build()
    exe = str(tmp_path / name)
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", name + ".c"),
           "-L" + PKG, "-ldzo_hip", "-Wl,-rpath," + PKG, "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run(["nm", "-u", exe], check=True, capture_output=True, text=True).stdout
    wanted = {l.split()[-1].split("@")[0] for l in out.splitlines() if " dzo_" in l}
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libdzo_hip.so")], check=True, capture_output=True,
                              text=True).stdout
    have = {l.split()[-1] for l in exported.splitlines()}
    return exe, wanted, have
