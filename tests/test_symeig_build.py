"""CPU-side checks of the batched symmetric eigensolver (the method of tests/test_hessian_batch_build.py): the library exports
its entry points, the Python table and the Julia module bind them, the constant matches the header, the header states the
arithmetic, the kernels exist for gfx950 in both storages and both element types without scratch memory or spills, the kernel
storage plan is a sound pure function, and the plain-C example compiles and
links against the library alone.  No compute here."""
import ctypes
import inspect
import os
import re

import numpy as np

import symeig_twin as st
from build_checks import link_example
from kernel_inventory import UNITS, check_unit
from dzo_loader import dzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dzoptimization.jl_amd")
SYMBOLS = ["dzo_symmetric_batch_eigen", "dzo_symeig_plan"]
LDS_LIMIT = 160 * 1024


def test_library_exports_the_eigensolver_entry_points():
    lib = ctypes.CDLL(dzo.build())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert [n for n in SYMBOLS if n not in dzo.ABI] == []
    assert len(dzo.ABI["dzo_symmetric_batch_eigen"]) == 8 and len(dzo.ABI["dzo_symeig_plan"]) == 5
    julia = open(os.path.join(PKG, "julia", "DZOptimizationAMD.jl")).read()
    assert [n for n in SYMBOLS if "(:%s, libdzo)" % n not in julia] == []
    for name in ("symmetric_batch_eigen!", "symeig_plan", "hessian_spectrum"):
        assert re.search(r"^function %s\(" % re.escape(name), julia, flags=re.M), name
        assert name in julia[julia.index("export "):julia.index("const libdzo")], name


def test_python_constant_and_functions_match_the_header():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    m = re.search(r"#define\s+DZO_SYMEIG_MAX_N\s+(\d+)\b", header)
    assert m and dzo.SYMEIG_MAX_N == int(m.group(1)) == 384
    assert re.search(r"#define\s+DZO_SYMEIG_DEFAULT_SWEEPS\s+30\b", header) and st.DEFAULT_SWEEPS == 30
    for name, value in (("LDS", dzo.SYMEIG_STORAGE_LDS), ("MEMORY", dzo.SYMEIG_STORAGE_MEMORY)):
        assert re.search(r"#define\s+DZO_SYMEIG_STORAGE_%s\s+%d\b" % (name, value), header), name
    eig = inspect.signature(dzo.symmetric_batch_eigen).parameters
    assert list(eig) == ["matrices", "n", "vectors", "max_sweeps"]
    assert eig["vectors"].default is False and eig["max_sweeps"].default == 0
    spec = inspect.signature(dzo.hessian_spectrum).parameters
    assert list(spec)[:3] == ["points", "n_particles", "vectors"] and spec["vectors"].default is False
    # the existing path stays what it was
    assert list(inspect.signature(dzo.hessian_eigenvalues).parameters) == ["points", "n_particles", "radial"]
    assert "eigvalsh" in inspect.getsource(dzo.hessian_eigenvalues)


def test_header_states_the_arithmetic():
    header = open(os.path.join(ROOT, "include", "dzo.h")).read()
    start = header.index("Batched symmetric eigensolver")
    assert header.index("Batched Hessian-vector products and dense Hessians") < start
    assert header.index("int32_t dzo_pairwise_batch_hessian(") < start
    block = header[start:header.index("LBFGSOptimizer  (src/DZOptimization.jl:321-509)")]
    flat = " ".join(block.replace("\n *", " ").split())
    for needle in ("a[r,c] = T(0.5) * (A[r,c] + A[c,r])", "off <= eps_T * fro", "never as a difference of two sums",
                   "m - 1 rounds", "idx[k] with idx[m-1-k]", "idx = [idx[0], idx[m-1], idx[1], ..., idx[m-2]]", "The list is reset",
                   "p = min, q = max", "tau = (a_qq - a_pp) / (a_pq + a_pq)", "t = copysign(1, tau) / (|tau| + sqrt(1 + tau*tau))",
                   "c = 1 / sqrt(1 + t*t)", "s = t * c", "If a_pq == 0: c = 1, s = 0", "45 degree",
                   "(a[r,p], a[r,q]) = (c*a[r,p] - s*a[r,q], s*a[r,p] + c*a[r,q])",
                   "(a[p,k], a[q,k]) = (c*a[p,k] - s*a[q,k], s*a[p,k] + c*a[q,k])", "a[p,q] = a[q,p] = 0 exactly",
                   "#{j : d_j < d_k} + #{j < k : d_j == d_k}", "no atomics", "offsets 32, 16, 8, 4, 2, 1", "column-major",
                   "sweeps = -1", "with or without eigenvectors", "DZO_ERR_INVALID", "DZO_ERR_UNSUPPORTED", "DZO_ERR_ASSERT",
                   "matrices_dev is not modified", "max_sweeps <= 0: the default, 30"):
        assert needle in flat, needle
    for proto in SYMBOLS:
        assert "int32_t %s(" % proto in block, proto


def test_symeig_kernels_exist_for_gfx950_without_scratch():
    """One kernel body, two storages, two element types: no private segment, no VGPR or SGPR spill."""
    assert UNITS["symeig"] == {"symeig_jacobi_kernel": ((dzo.SYMEIG_STORAGE_LDS, dzo.SYMEIG_STORAGE_MEMORY),)}
    check_unit("symeig", lj_count=4)
    src = open(os.path.join(PKG, "csrc", "dzo_symeig.hip")).read()
    assert 'DZO_TIMED("symeig"' in src and "atomic" not in src.split("namespace dzo {", 1)[1]
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src and '#include "dzo_symeig_plan.h"' in src
    assert "csrc/dzo_symeig.hip" in open(os.path.join(PKG, "Makefile")).read()
    plan = open(os.path.join(PKG, "csrc", "dzo_symeig_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan       # a plain C++ header


def test_plan_is_a_sound_pure_function():
    """dzo_symeig_plan over the whole range, without a device: LDS bytes within 160 KiB, ld >= n and never a multiple of 32
    elements on LDS storage, storage monotone in n, matrix plus angles accounted for, the workload (fp64, n = 114) on LDS, and
    LDS storage used WHENEVER it fits."""
    for dtype, es in ((np.float64, 8), (np.float32, 4)):
        seen_memory = False
        for n in range(1, dzo.SYMEIG_MAX_N + 1):
            storage, ld, lds = dzo.symeig_plan(n, dtype)
            assert (storage, ld, lds) == dzo.symeig_plan(n, dtype)
            m = n + (n & 1)
            assert 0 < lds <= LDS_LIMIT and ld >= n
            fits = 64 + 2 * m * es + n * (n | 1) * es <= LDS_LIMIT
            assert (storage == dzo.SYMEIG_STORAGE_LDS) == fits, (n, storage)
            if storage == dzo.SYMEIG_STORAGE_LDS:
                assert not seen_memory, n                       # monotone
                assert ld % 2 == 1 and ld - n <= 1 and ld % 32 != 0
                assert lds >= (n * ld + m) * es                 # the matrix and the angles (c, s per pair)
            else:
                seen_memory = True
                assert ld == n and lds >= m * es
        assert seen_memory
        last, first = st.lds_edge(np.dtype(dtype), dzo.symeig_plan)
        assert last == st.LDS_LAST[np.dtype(dtype)] and first == last + 1
    assert dzo.symeig_plan(114, np.float64) == (dzo.SYMEIG_STORAGE_LDS, 115, 64 + 2 * 114 * 8 + 114 * 115 * 8)
    L = dzo.lib()
    assert L.dzo_symeig_plan(114, dzo.F64, None, None, None) == 0             # outputs are optional
    assert L.dzo_symeig_plan(0, dzo.F64, None, None, None) == 1 and L.dzo_symeig_plan(8, 9, None, None, None) == 1
    assert L.dzo_symeig_plan(385, dzo.F64, None, None, None) == 5


def test_lj_spectrum_example_compiles_and_links(tmp_path):
    _, wanted, have = link_example(tmp_path, "lj_spectrum")
    assert {"dzo_symmetric_batch_eigen", "dzo_symeig_plan", "dzo_pairwise_batch_hessian", "dzo_lbfgs_batch_create",
            "dzo_lbfgs_batch_step"} <= wanted and wanted <= have, wanted - have
