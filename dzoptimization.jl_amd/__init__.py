"""dzoptimization.jl_amd -- MI355X-native BFGS / L-BFGS ``step!()`` (host-side mirror).

This package is the Python twin of the Julia host module in ``julia/DZOptimizationAMD.jl``:
both are thin bindings over the C ABI of ``include/dzo.h`` (``libdzo_hip.so``, hand-written
HIP for gfx950).  It mirrors the reference's optimizer interface -- constructor argument
order, public state fields, ``step!`` -> :func:`step_` / ``opt.step()``, and the termination
flag under all three historical names (``is_stuck`` ≡ ``has_terminated`` ≡ ``has_converged``;
SURVEY.md 1.2) -- so that the parity tests read like the reference's own usage
(README.md:33-41, src/DZOptimization.jl:347-427).

The directory name contains a dot, so it cannot be imported by name; use the loader::

    from dzo_loader import dzo        # repo root
    opt = dzo.LBFGSOptimizer(None, problem, None, x0, 1.0, 20)

There is NO CPU fallback: importing works anywhere (so ABI/symbol tests can run without a
GPU), but every compute entry point raises :class:`DzoError` unless ``libdzo_hip.so`` is
built and a HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DZO_LIB_PATH") or os.path.join(_HERE, "libdzo_hip.so")   # (override: A/B of two builds)
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

F32, F64 = 0, 1
ROSENBROCK2D, ROSENBROCK_CHAIN, QUADRATIC, LSE, QUADRATIC_CHAIN = 0, 1, 2, 3, 4
PAIRWISE_LJ = 5                 # n = 3N, point = [x | y | z] (src/ExampleFunctions.jl)
RADIAL_LENNARD_JONES = 0        # lj_energy / lj_first_derivative / lj_second_derivative (:16-72)
RADIAL_MORSE_RHO6, RADIAL_MORSE_RHO14 = 2, 3   # E(r) = t^2 - 2 t, t = exp(rho (1 - r)): pair minimum at r = 1, depth 1 (include/dzo.h)
TWOLOOP_CHAIN, TWOLOOP_GRAM = 0, 1
LINE_SEARCH_BACKTRACKING, LINE_SEARCH_WOLFE = 0, 1
STEP_NULL, STEP_GRADIENT_DESCENT, STEP_BFGS = 0, 1, 2

_ERR = {1: "invalid argument", 2: "HIP runtime error", 3: "reference @assert", 4: "out of memory",
        5: "unsupported", 6: "bad call sequence", 7: "more candidates than the capacity"}


class DzoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dzo error {code} ({_ERR.get(code, '?')}): {msg}")
        self.code = code


class AssertionFailed(DzoError, AssertionError):
    """A reference ``@assert`` would have fired (Julia raises AssertionError)."""


def build(force: bool = False) -> str:
    """Compile ``libdzo_hip.so`` for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(INCLUDE_DIR, "dzo.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        jobs = str(min(8, os.cpu_count() or 1))
        subprocess.check_call(["make", "-C", _HERE, "-j", jobs] + (["-B"] if force else []))
    return LIB_PATH


_lib = None
_inited = False


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same
    SONAME as /opt/rocm's); if libdzo_hip.so bound to the system copy and torch later loaded
    its own, the second runtime finds no device.  Bind to torch's copy whenever torch is
    installed -- without importing torch -- so the load order never matters."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib() -> C.CDLL:
    """Load the C-ABI library (no device needed for loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DzoError(2, f"{LIB_PATH} is not built; run __graft_entry__.build() "
                              "(there is no CPU fallback)")
        _preload_hip_runtime()
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().dzo_last_error().decode(errors="replace")
        raise (AssertionFailed if rc == 3 else DzoError)(rc, msg)


def init(device: int = 0) -> None:
    """Select the HIP device.  Fails loudly when there is none."""
    global _inited
    _check(lib().dzo_init(device))
    _inited = True


def _need_init():
    if not _inited:
        init(int(os.environ.get("LOCAL_RANK", "0")) if "DZO_DEVICE" not in os.environ
             else int(os.environ["DZO_DEVICE"]))


def device_info():
    _need_init()
    name = C.create_string_buffer(128)
    cus, hbm = C.c_int32(), C.c_int64()
    _check(lib().dzo_device_info(name, 128, C.byref(cus), C.byref(hbm)))
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}


def device_count() -> int:
    """HIP devices visible to the process (no ``init`` needed, no context created)."""
    v = C.c_int32()
    _check(lib().dzo_device_count(C.byref(v)))
    return v.value


def synchronize():
    _check(lib().dzo_synchronize())


def calibrate_read_bandwidth(nbytes, repeats=20):
    """GB/s of a plain streaming read over ``nbytes`` (Infinity-Cache resident up to ~200 MiB, HBM beyond)."""
    _need_init()
    r = C.c_double()
    _check(lib().dzo_calibrate_read_bandwidth(int(nbytes), int(repeats), C.byref(r)))
    return r.value


def selftest_fast_div(seed, pairs, mode):
    """(checked, mismatches, first) of ``dzo_selftest_fast_div``: the recurrence's division-free quotient against ``a / b``."""
    _need_init()
    chk, bad = C.c_int64(), C.c_int64()
    first = (C.c_double * 4)()
    _check(lib().dzo_selftest_fast_div(int(seed), int(pairs), int(mode), C.byref(chk), C.byref(bad), first))
    return chk.value, bad.value, list(first)


def calibrate_read_bandwidth_of(array, repeats=20):
    """GB/s of the same streaming read over the bytes of a DeviceArray, whatever it holds."""
    _need_init()
    r = C.c_double()
    _check(lib().dzo_calibrate_read_bandwidth_of(array.ptr, int(array.size * array.dtype.itemsize), int(repeats), C.byref(r)))
    return r.value


# ------------------------------------------------------------------------------ ABI table
_vp, _i32, _i64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
CONSTRAINT_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p)
OBJECTIVE_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p)
GRADIENT_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)
_P = C.POINTER

# name -> argtypes; every function returns int32 except dzo_last_error / dzo_version
ABI = {
    "dzo_init": [_i32], "dzo_shutdown": [], "dzo_device_info": [C.c_char_p, _i32, _P(_i32), _P(_i64)],
    "dzo_device_count": [_P(_i32)],
    "dzo_synchronize": [],
    "dzo_profile_enable": [_i32], "dzo_profile_reset": [], "dzo_unsealed_first_reads": [_P(_i64)], "dzo_profile_count": [_P(_i32)],
    "dzo_profile_get": [_i32, C.c_char_p, _i32, _P(_i64), _P(_dbl)],
    "dzo_calibrate_read_bandwidth": [_i64, _i32, _P(_dbl)],
    "dzo_selftest_fast_div": [C.c_uint64, _i64, _i32, _P(_i64), _P(_i64), _P(_dbl)],
    "dzo_calibrate_read_bandwidth_of": [_vp, _i64, _i32, _P(_dbl)],
    "dzo_calibrate_fma_rate": [_i32, _i64, _P(_dbl)],
    "dzo_pairwise_energy": [_i32, _i64, _i32, _vp, _vp, _vp, _P(_dbl)],
    "dzo_pairwise_gradient": [_i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dzo_pairwise_hvp": [_i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dzo_pairwise_energy_delta": [_i32, _i64, _i32, _vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, _P(_dbl)],
    "dzo_tempering_create": [_i32, _i64, _i64, _i32, _vp, _P(_dbl), _P(_dbl), _dbl, C.c_uint64, _P(_vp)],
    "dzo_tempering_destroy": [_vp], "dzo_tempering_temper": [_vp, _i64, _vp, _i64], "dzo_tempering_swap": [_vp, _i32],
    "dzo_tempering_run": [_vp, _i64, _i64, _vp, _i64],
    "dzo_tempering_analyze": [_vp, _i64, _vp, _i64, _P(_dbl), _P(_dbl), _P(_dbl)], "dzo_tempering_set_record": [_vp, _i64],
    "dzo_tempering_get_ptr": [_vp, _i32, _P(_vp)], "dzo_tempering_read": [_vp, _i32, _vp], "dzo_tempering_set": [_vp, _i32, _vp],
    "dzo_lbfgs_batch_create": [_i32, _i64, _i64, _i32, _vp, _dbl, _i32, _P(_vp)], "dzo_lbfgs_batch_destroy": [_vp],
    "dzo_lbfgs_batch_set_max_halvings": [_vp, _i64], "dzo_lbfgs_batch_step": [_vp, _i32, _P(_i32)],
    "dzo_lbfgs_batch_count_active": [_vp, _P(_i64)], "dzo_lbfgs_batch_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_lbfgs_batch_read": [_vp, _i32, _vp], "dzo_pairwise_batch_energy_gradient": [_i32, _i64, _i64, _i32, _vp, _vp, _vp],
    "dzo_sphere_batch_project": [_i64, _i64, _i32, _vp],
    "dzo_sphere_batch_energy_gradient": [_i32, _i64, _i64, _i32, _vp, _vp, _vp, _i32],
    "dzo_sphere_lbfgs_batch_create": [_i32, _i64, _i64, _i32, _vp, _dbl, _i32, _P(_vp)], "dzo_sphere_lbfgs_batch_destroy": [_vp],
    "dzo_sphere_lbfgs_batch_set_max_halvings": [_vp, _i64], "dzo_sphere_lbfgs_batch_step": [_vp, _i32, _P(_i32)],
    "dzo_sphere_lbfgs_batch_count_active": [_vp, _P(_i64)], "dzo_sphere_lbfgs_batch_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_sphere_lbfgs_batch_read": [_vp, _i32, _vp],
    "dzo_basin_hopping_create": [_i32, _i64, _i64, _i32, _vp, _P(_dbl), _P(_dbl), _dbl, _dbl, _i32, _i32, C.c_uint64, _P(_vp)],
    "dzo_basin_hopping_destroy": [_vp], "dzo_basin_hopping_set_max_halvings": [_vp, _i64], "dzo_basin_hopping_hop": [_vp, _i64, _i32],
    "dzo_basin_hopping_set_record": [_vp, _i64], "dzo_basin_hopping_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_basin_hopping_read": [_vp, _i32, _vp], "dzo_basin_hopping_set": [_vp, _i32, _vp],
    "dzo_adgd_batch_create": [_i32, _i64, _i64, _i32, _vp, _dbl, _P(_vp)], "dzo_adgd_batch_destroy": [_vp],
    "dzo_adgd_batch_set_max_halvings": [_vp, _i64], "dzo_adgd_batch_step": [_vp, _i32, _P(_i32)],
    "dzo_adgd_batch_count_active": [_vp, _P(_i64)], "dzo_adgd_batch_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_adgd_batch_read": [_vp, _i32, _vp],
    "dzo_pairwise_batch_hvp": [_i32, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp],
    "dzo_pairwise_batch_hessian": [_i32, _i64, _i64, _i32, _vp, _vp],
    "dzo_symmetric_batch_eigen": [_i64, _i64, _i32, _vp, _vp, _vp, _vp, _i32],
    "dzo_symeig_plan": [_i64, _i32, _P(_i32), _P(_i64), _P(_i64)],
    "dzo_pairwise_batch_lowest_mode": [_i32, _i64, _i64, _i32, _vp, _i32, _i32, _i32, _dbl, C.c_uint64, _vp, _vp, _vp, _vp, _vp],
    "dzo_modefollow_batch_apply": [_i32, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp],
    "dzo_modefollow_batch_create": [_i32, _i64, _i64, _i32, _vp, _i32, _dbl, _dbl, _dbl, _P(_vp)], "dzo_modefollow_batch_destroy": [_vp],
    "dzo_modefollow_batch_set_start_mode": [_vp, _i32], "dzo_modefollow_batch_set_directions": [_vp, _vp],
    "dzo_modefollow_batch_step": [_vp, _i32, _P(_i32)], "dzo_modefollow_batch_count_active": [_vp, _P(_i64)],
    "dzo_modefollow_batch_get_ptr": [_vp, _i32, _P(_vp)], "dzo_modefollow_batch_read": [_vp, _i32, _vp],
    "dzo_hybridef_batch_apply": [_i32, _i64, _i64, _i32, _vp, _vp, _vp, _dbl, _i32, _i32, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp],
    "dzo_hybridef_batch_create": [_i32, _i64, _i64, _i32, _vp, _vp, _dbl, _i32, _i32, _dbl, _dbl, _i32, _i32, _dbl, _dbl, _dbl, C.c_uint64,
                                  _P(_vp)],
    "dzo_hybridef_batch_destroy": [_vp], "dzo_hybridef_batch_set_directions": [_vp, _vp],
    "dzo_hybridef_batch_step": [_vp, _i32, _P(_i32)], "dzo_hybridef_batch_count_active": [_vp, _P(_i64)],
    "dzo_hybridef_batch_get_ptr": [_vp, _i32, _P(_vp)], "dzo_hybridef_batch_read": [_vp, _i32, _vp],
    "dzo_neb_plan": [_i64, _i32, _i32, _P(_i32), _P(_i32), _P(_i64)],
    "dzo_neb_batch_interpolate": [_i64, _i32, _i64, _i32, _vp, _vp, _vp],
    "dzo_neb_batch_apply": [_i32, _i64, _i32, _i64, _i32, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dzo_neb_batch_create": [_i32, _i64, _i32, _i64, _i32, _vp, _dbl, _dbl, _dbl, _dbl, _i32, _i64, _P(_vp)],
    "dzo_neb_batch_destroy": [_vp], "dzo_neb_batch_step": [_vp, _i32, _P(_i32)], "dzo_neb_batch_count_active": [_vp, _P(_i64)],
    "dzo_neb_batch_get_ptr": [_vp, _i32, _P(_vp)], "dzo_neb_batch_read": [_vp, _i32, _vp],
    "dzo_align_batch_assign": [_i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "dzo_align_batch_pairs": [_i64, _i64, _i32, _vp, _vp, _i32, _i32, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dzo_pathway_batch_candidates": [_i64, _i32, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _P(_i64)],
    "dzo_structure_batch_fingerprint": [_i32, _i64, _i64, _i32, _vp, _vp, _vp],
    "dzo_structure_batch_classify": [_i64, _i64, _i32, _vp, _dbl, _vp, _P(_i32)],
    "dzo_malloc": [_P(_vp), _i64], "dzo_free": [_vp], "dzo_memcpy_h2d": [_vp, _vp, _i64],
    "dzo_memcpy_d2h": [_vp, _vp, _i64], "dzo_memcpy_d2d": [_vp, _vp, _i64],
    "dzo_axpy": [_i64, _i32, _dbl, _vp, _vp], "dzo_axpby": [_i64, _i32, _dbl, _vp, _dbl, _vp],
    "dzo_scal": [_i64, _i32, _dbl, _vp], "dzo_copy": [_i64, _i32, _vp, _vp],
    "dzo_fill": [_i64, _i32, _dbl, _vp], "dzo_dot": [_i64, _i32, _vp, _vp, _P(_dbl)],
    "dzo_nrm2": [_i64, _i32, _vp, _P(_dbl)], "dzo_isequal": [_i64, _i32, _vp, _vp, _P(_i32)],
    "dzo_trial_point": [_i64, _i32, _vp, _dbl, _vp, _vp],
    "dzo_norm2": [_i64, _i32, _vp, _P(_dbl)], "dzo_inv_norm": [_i64, _i32, _vp, _P(_dbl)],
    "dzo_negate": [_i64, _i32, _vp], "dzo_scal_oop": [_i64, _i32, _vp, _dbl, _vp],
    "dzo_problem_create": [_i32, _i64, _i32, _vp, _vp, _dbl, _P(_vp)], "dzo_problem_destroy": [_vp],
    "dzo_problem_eval": [_vp, _vp, _P(_dbl)], "dzo_problem_grad": [_vp, _vp, _vp],
    "dzo_problem_objective_cb": [_vp, _vp], "dzo_problem_gradient_cb": [_vp, _vp, _vp], "dzo_problem_constraint_cb": [_vp, _vp],
    "dzo_problem_set_l2": [_vp, _dbl], "dzo_problem_set_box_gradient": [_vp, _i32, _dbl, _dbl],
    "dzo_problem_set_box_constraint": [_vp, _i32, _dbl, _dbl], "dzo_box_clamp": [_i64, _i32, _vp, _dbl, _dbl],
    "dzo_lbfgs_create": [_i64, _i32, _i32, _vp, _vp, _dbl, _dbl, _P(_vp)],
    "dzo_lbfgs_create_callbacks": [CONSTRAINT_FN, OBJECTIVE_FN, GRADIENT_FN, _vp, _i64, _i32, _i32, _vp,
                                   _dbl, _P(_vp)],
    "dzo_lbfgs_create_problem": [_vp, _i32, _vp, _dbl, _P(_vp)], "dzo_lbfgs_destroy": [_vp],
    "dzo_lbfgs_set_callbacks": [_vp, CONSTRAINT_FN, OBJECTIVE_FN, GRADIENT_FN, _vp],
    "dzo_lbfgs_set_problem": [_vp, _vp], "dzo_lbfgs_set_two_loop_mode": [_vp, _i32],
    "dzo_lbfgs_set_max_halvings": [_vp, _i64],
    "dzo_lbfgs_set_safeguards": [_vp, _i32, _i32], "dzo_lbfgs_set_line_search": [_vp, _i32, _dbl, _dbl, _i32],
    "dzo_lbfgs_step": [_vp], "dzo_lbfgs_direction": [_vp],
    "dzo_lbfgs_begin_search": [_vp], "dzo_lbfgs_trial": [_vp, _dbl, _P(_i32)],
    "dzo_lbfgs_accept": [_vp, _dbl], "dzo_lbfgs_reject": [_vp], "dzo_lbfgs_pre_gradient": [_vp],
    "dzo_lbfgs_post_gradient": [_vp], "dzo_lbfgs_get_i": [_vp, _i32, _P(_i64)],
    "dzo_lbfgs_get_s": [_vp, _i32, _P(_dbl)], "dzo_lbfgs_set_s": [_vp, _i32, _dbl],
    "dzo_lbfgs_set_stuck": [_vp, _i32], "dzo_lbfgs_get_ptr": [_vp, _i32, _i32, _P(_vp)], "dzo_lbfgs_read": [_vp, _i32, _i32, _vp],
    "dzo_lbfgs_get_rho": [_vp, _P(_dbl), _i32, _P(_i32)],
    "dzo_lbfgs_get_alpha": [_vp, _P(_dbl), _i32, _P(_i32)],
    "dzo_lbfgs_set_history": [_vp, _i32, _vp, _vp, _P(_dbl), _i64], "dzo_lbfgs_stream": [_vp, _P(_vp)],
    "dzo_line_search_eval": [CONSTRAINT_FN, OBJECTIVE_FN, GRADIENT_FN, _vp, _i64, _i32, _vp, _dbl, _vp, _dbl,
                             _dbl, _i32, _vp, _vp, _P(_dbl), _P(_dbl), _P(_dbl)],
    "dzo_adgd_create": [_i64, _i32, _vp, _vp, _dbl, _dbl, _P(_vp)],
    "dzo_adgd_create_problem": [_vp, _vp, _dbl, _P(_vp)], "dzo_adgd_destroy": [_vp],
    "dzo_adgd_set_callbacks": [_vp, CONSTRAINT_FN, OBJECTIVE_FN, GRADIENT_FN, _vp], "dzo_adgd_step": [_vp],
    "dzo_adgd_get_i": [_vp, _i32, _P(_i64)], "dzo_adgd_get_s": [_vp, _i32, _P(_dbl)],
    "dzo_adgd_get_ptr": [_vp, _i32, _P(_vp)], "dzo_adgd_read": [_vp, _i32, _vp],
    "dzo_bfgs_create_callbacks": [OBJECTIVE_FN, GRADIENT_FN, CONSTRAINT_FN, _vp, _i64, _i32, _vp, _dbl,
                                  _P(_vp)],
    "dzo_bfgs_create_problem": [_vp, _vp, _dbl, _P(_vp)], "dzo_bfgs_destroy": [_vp], "dzo_bfgs_step": [_vp],
    "dzo_bfgs_convert_problem": [_vp, _vp, _P(_vp)],
    "dzo_bfgs_convert_callbacks": [_vp, _i32, OBJECTIVE_FN, GRADIENT_FN, CONSTRAINT_FN, _vp, _P(_vp)],
    "dzo_bfgs_update": [_i64, _i32, _vp, _dbl, _vp, _vp, _vp, _vp, _vp],
    "dzo_symv": [_i64, _i32, _vp, _vp, _vp],
    "dzo_bfgs_update_mfma": [_i64, _i32, _vp, _dbl, _vp, _vp, _vp],
    "dzo_bfgs_line_search": [_vp, _i32, _dbl, _P(_dbl), _P(_dbl)], "dzo_bfgs_set_max_increases": [_vp, _i32], "dzo_bfgs_reset": [_vp],
    "dzo_bfgs_get_i": [_vp, _i32, _P(_i64)], "dzo_bfgs_get_s": [_vp, _i32, _P(_dbl)],
    "dzo_bfgs_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_bfgs_set_s": [_vp, _i32, _dbl], "dzo_bfgs_set_i": [_vp, _i32, _i64],
    "dzo_gd_create_callbacks": [CONSTRAINT_FN, OBJECTIVE_FN, GRADIENT_FN, _vp, _i64, _i32, _vp, _dbl, _P(_vp)],
    "dzo_gd_create_problem": [_vp, _vp, _dbl, _P(_vp)], "dzo_gd_step": [_vp],
    "dzo_bfgs_batch_create": [_i32, _i64, _i64, _i32, _vp, _dbl, _P(_vp)], "dzo_bfgs_batch_destroy": [_vp],
    "dzo_bfgs_batch_step": [_vp, _i32, _P(_i32)], "dzo_bfgs_batch_get_ptr": [_vp, _i32, _P(_vp)],
    "dzo_bfgs_batch_count_active": [_vp, _P(_i64)],
    "dzo_bfgs_batch_create_on": [_i32, _i32, _i64, _i64, _i32, _vp, _dbl, _P(_vp)], "dzo_bfgs_batch_device": [_vp, _P(_i32)],
    "dzo_bfgs_batch_create_problem": [_vp, _i64, _vp, _dbl, _i32, _P(_vp)],
    "dzo_bfgs_batch_create_problem_matrices": [_vp, _i64, _vp, _i64, _vp, _dbl, _i32, _P(_vp)], "dzo_bfgs_batch_set_max_increases": [_vp, _i32],
    "dzo_comm_unique_id": [_vp], "dzo_comm_init_rank": [_vp, _i32, _i32, _P(_vp)],
    "dzo_comm_init_all": [_P(_i32), _i32, _P(_vp)], "dzo_comm_destroy": [_vp],
    "dzo_comm_info": [_vp, _P(_i32), _P(_i32), _P(_i32), _P(_i64)],
    "dzo_flag_allreduce_min": [_vp, _P(_i32), _P(_i32)],
    "dzo_flag_allreduce_min_n": [_vp, _P(_i32), _i32, _P(_i32)],
    "dzo_bfgs_batch_all_done": [_vp, _P(_vp), _i32, _P(_i32)],
}


def _declare(L):
    for name, args in ABI.items():
        fn = getattr(L, name)           # AttributeError here = symbol missing from the library
        fn.argtypes = args
        fn.restype = C.c_int32
    L.dzo_problem_objective_cb.restype = C.c_double
    L.dzo_problem_gradient_cb.restype = None
    L.dzo_last_error.restype = C.c_char_p
    L.dzo_last_error.argtypes = []
    L.dzo_version.restype = C.c_int32
    L.dzo_version.argtypes = []


def _dt(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return F64
    if dtype == np.float32:
        return F32
    raise TypeError(f"unsupported element type {dtype}")


def _np(dt: int):
    return np.float64 if dt == F64 else np.float32


# ------------------------------------------------------------------------------ device arrays
class DeviceArray:
    """Dense device vector/matrix (what ``A <: AbstractArray{T}`` is for the reference).

    Owns HBM allocated through the C ABI, or wraps a raw device pointer (``owner=False``) such
    as a ``torch.Tensor.data_ptr()`` or an optimizer field."""

    def __init__(self, shape, dtype=np.float64, ptr=None, owner=True):
        _need_init()
        self.shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.size = int(np.prod(self.shape)) if self.shape else 1
        self.nbytes = self.size * self.dtype.itemsize
        self._owner = owner and ptr is None
        if ptr is None:
            p = C.c_void_p()
            _check(lib().dzo_malloc(C.byref(p), max(self.nbytes, 16)))
            ptr = p.value
        self.ptr = int(ptr)

    @classmethod
    def from_host(cls, a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        d = cls(a.shape, a.dtype)
        d.upload(a)
        return d

    @classmethod
    def zeros(cls, shape, dtype=np.float64):
        d = cls(shape, dtype)
        _check(lib().dzo_fill(d.size, _dt(dtype), 0.0, d.ptr))
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size == self.size
        _check(lib().dzo_memcpy_h2d(self.ptr, a.ctypes.data, self.nbytes))
        return self

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        _check(lib().dzo_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes))
        return out

    def copy(self):
        d = DeviceArray(self.shape, self.dtype)
        _check(lib().dzo_memcpy_d2d(d.ptr, self.ptr, self.nbytes))
        return d

    def view(self, offset_elems, shape):
        return DeviceArray(shape, self.dtype, ptr=self.ptr + offset_elems * self.dtype.itemsize, owner=False)

    def free(self):
        if self._owner and self.ptr and _lib is not None:
            lib().dzo_free(self.ptr)
        self.ptr = 0
        self._owner = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __len__(self):
        return self.shape[0]


def _as_dev(a, dtype=None):
    return a if isinstance(a, DeviceArray) else DeviceArray.from_host(a, dtype)


# L1 primitives with the reference's call shapes (LinearAlgebra / Base)
def axpy_(alpha, x, y):
    _check(lib().dzo_axpy(x.size, _dt(x.dtype), alpha, x.ptr, y.ptr)); return y


def axpby_(alpha, x, beta, y):
    _check(lib().dzo_axpby(x.size, _dt(x.dtype), alpha, x.ptr, beta, y.ptr)); return y


def rmul_(x, alpha):
    _check(lib().dzo_scal(x.size, _dt(x.dtype), alpha, x.ptr)); return x


def copy_(dst, src):
    _check(lib().dzo_copy(src.size, _dt(src.dtype), src.ptr, dst.ptr)); return dst


def fill_(x, value):
    _check(lib().dzo_fill(x.size, _dt(x.dtype), value, x.ptr)); return x


def dot(x, y):
    r = C.c_double()
    _check(lib().dzo_dot(x.size, _dt(x.dtype), x.ptr, y.ptr, C.byref(r))); return r.value


def norm(x):
    r = C.c_double()
    _check(lib().dzo_nrm2(x.size, _dt(x.dtype), x.ptr, C.byref(r))); return r.value


def isequal(a, b):
    r = C.c_int32()
    _check(lib().dzo_isequal(a.size, _dt(a.dtype), a.ptr, b.ptr, C.byref(r))); return bool(r.value)


# legacy/Kernels.jl primitives without a LinearAlgebra twin
def norm2(x):
    """``norm2(x)``: the sum of squares, not its root (legacy/Kernels.jl:49-55,139)."""
    r = C.c_double()
    _check(lib().dzo_norm2(x.size, _dt(x.dtype), x.ptr, C.byref(r))); return r.value


def inv_norm(x):
    """``inv_norm(x) = rsqrt(norm2(x))`` (legacy/Kernels.jl:141)."""
    r = C.c_double()
    _check(lib().dzo_inv_norm(x.size, _dt(x.dtype), x.ptr, C.byref(r))); return r.value


def negate_(x):
    """``negate!(x)`` (legacy/Kernels.jl:76-83)."""
    _check(lib().dzo_negate(x.size, _dt(x.dtype), x.ptr)); return x


def scale_(dst, alpha, x=None):
    """``scale!(x, alpha)`` in place (legacy/Kernels.jl:87-94) or ``scale!(dst, alpha, x)`` out of
    place (:96-104)."""
    if x is None:
        return rmul_(dst, alpha)
    _check(lib().dzo_scal_oop(x.size, _dt(x.dtype), dst.ptr, alpha, x.ptr)); return dst


def box_clamp_(x, lower_bound, upper_bound):
    """``UniformBoxConstraint(lo, hi)(x)`` (legacy/DZOptimization.jl:264-272); returns True."""
    _check(lib().dzo_box_clamp(x.size, _dt(x.dtype), x.ptr, lower_bound, upper_bound)); return True


def trial_point_(dst, t, d, x):
    _check(lib().dzo_trial_point(x.size, _dt(x.dtype), dst.ptr, t, d.ptr, x.ptr)); return dst


def calibrate_fma_rate(dtype=np.float64, iters=1 << 16):
    """GFLOP/s (2 per fma) of a register-only loop of independent fma chains on every CU."""
    _need_init()
    r = C.c_double()
    _check(lib().dzo_calibrate_fma_rate(_dt(dtype), int(iters), C.byref(r)))
    return r.value


# ------------------------------------------------------------------------------ pairwise radial N-body functions
# src/ExampleFunctions.jl with the radial function selected by ``radial`` (the reference passes lj_energy etc.); x, y, z
# (and the outputs) are DeviceArrays of N elements each, views at any element offset included
def pairwise_radial_energy(x, y, z, radial=RADIAL_LENNARD_JONES):
    """``accelerated_pairwise_radial_energy(lj_energy, x, y, z)`` (:152-173)."""
    r = C.c_double()
    _check(lib().dzo_pairwise_energy(radial, x.size, _dt(x.dtype), x.ptr, y.ptr, z.ptr, C.byref(r)))
    return r.value


def pairwise_radial_gradient_(gx, gy, gz, x, y, z, radial=RADIAL_LENNARD_JONES):
    """``accelerated_pairwise_radial_gradient!(gx, gy, gz, lj_first_derivative, x, y, z)`` (:265-294)."""
    _check(lib().dzo_pairwise_gradient(radial, x.size, _dt(x.dtype), gx.ptr, gy.ptr, gz.ptr, x.ptr, y.ptr, z.ptr))
    return gx, gy, gz


def pairwise_radial_hvp_(px, py, pz, x, y, z, u, v, w, radial=RADIAL_LENNARD_JONES):
    """``accelerated_pairwise_radial_hvp!(px, py, pz, lj_first_derivative, lj_second_derivative, x, y, z, u, v, w)`` (:427-468)."""
    _check(lib().dzo_pairwise_hvp(radial, x.size, _dt(x.dtype), px.ptr, py.ptr, pz.ptr, x.ptr, y.ptr, z.ptr, u.ptr, v.ptr, w.ptr))
    return px, py, pz


def pairwise_radial_energy_delta(x, y, z, i, x_new, y_new, z_new, radial=RADIAL_LENNARD_JONES):
    """``pairwise_radial_energy_delta(lj_energy, x, y, z, i, x_new, y_new, z_new)`` (:477-534); ``i`` is 0-based."""
    r = C.c_double()
    _check(lib().dzo_pairwise_energy_delta(radial, x.size, _dt(x.dtype), x.ptr, y.ptr, z.ptr, int(i), float(x_new), float(y_new),
                                           float(z_new), C.byref(r)))
    return r.value


# ------------------------------------------------------------------------------ handles of the C ABI
class _Handle:
    """An object of the C ABI and its lifetime.  A subclass names the prefix of its unit's entry points (``_prefix``, spelled
    out: ``"dzo_<unit>_"``) and sets ``h`` to what its ``create`` entry returned."""
    _prefix = None
    h = None

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    def _call(self, name, *args):
        _check(self._fn(name)(*args))

    def close(self):
        """Destroys the handle.  Safe to call again, on an object whose constructor raised, and once the library is gone."""
        h, self.h = self.h, None
        if h and _lib is not None:
            self._fn("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _HandleArrays(_Handle):
    """``read`` / ``ptr`` / ``_set`` of a handle whose device arrays are numbered by a ``what`` constant.  A subclass has
    ``_shape(what)`` -> (shape, dtype)."""

    def read(self, what):
        """A blocking host copy of one of the handle's arrays; row k = replica / instance k."""
        shape, dtype = self._shape(what)
        out = np.empty(shape, dtype=dtype)
        self._call("read", self.h, int(what), out.ctypes.data)
        return out

    def ptr(self, what):
        p = C.c_void_p()
        self._call("get_ptr", self.h, int(what), C.byref(p))
        return p.value

    def _set(self, what, values):
        shape, dtype = self._shape(what)
        a = np.ascontiguousarray(values, dtype=dtype)
        assert a.shape == shape
        self._call("set", self.h, int(what), a.ctypes.data)


def _u64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _per_walker(inverse_temperatures, perturbation_radii):
    """The two host sequences of a tempering or basin-hopping handle, one entry per replica / walker, as fp64 arrays."""
    beta = np.ascontiguousarray(inverse_temperatures, dtype=np.float64)
    rad = np.ascontiguousarray(perturbation_radii, dtype=np.float64)
    assert beta.ndim == 1 and beta.shape == rad.shape
    return beta, rad


def _batch_of(points, n_particles, name="points", least=0, batch=None):
    """``(n, batch)`` of an array of ``3 * n_particles * batch`` elements, instance b ``[x | y | z]`` at ``3 * n_particles * b``,
    with at least ``least`` instances; ``batch``: the number the array must hold, where something else tells it."""
    n = int(n_particles)
    batch = int(batch) if batch is not None else points.size // (3 * n) if n > 0 else 0
    assert points.size == 3 * n * batch and batch >= least, name + " must hold 3 * n_particles * batch elements"
    return n, batch


# ------------------------------------------------------------------------------ parallel tempering (scripts/MonteCarlo.jl)
TEMPERING_MAX_PARTICLES = 1024
(TEMPERING_REPLICAS, TEMPERING_RADII, TEMPERING_INV_TEMPS, TEMPERING_NUM_ACCEPT, TEMPERING_NUM_REJECT, TEMPERING_RNG_STATES,
 TEMPERING_REC_INDEX, TEMPERING_REC_NORMALS, TEMPERING_REC_UNIFORM, TEMPERING_REC_CODE, TEMPERING_REC_SWAP,
 TEMPERING_REC_SWAP_LOGP) = range(12)


class ParallelTempering(_HandleArrays):
    """``parallel_temper!`` / ``parallel_swap!`` / ``analyze`` of scripts/MonteCarlo.jl with the loop over the moves on the
    device.  ``replicas`` is a DeviceArray of ``3 * n_particles * n_replicas`` elements, per replica ``[x | y | z]`` (the
    reference's ``Array{T,3}(particles, 3, replicas)``); it is aliased and mutated, as the reference mutates its argument.
    ``inverse_temperatures`` and ``perturbation_radii`` are host sequences.  The random-number rule is in include/dzo.h.

    ``temper``, ``swap`` and ``run`` do not block; every property that reads device state does."""
    _prefix = "dzo_tempering_"

    def __init__(self, replicas, n_particles, inverse_temperatures, perturbation_radii, constraining_radius, base_seed=0,
                 radial=RADIAL_LENNARD_JONES):
        _need_init()
        self.replicas = replicas
        self.dtype = replicas.dtype
        self.n_particles = int(n_particles)
        beta, rad = _per_walker(inverse_temperatures, perturbation_radii)
        self.n_replicas = int(beta.size)
        assert replicas.size == 3 * self.n_particles * self.n_replicas, "replicas must hold 3 * n_particles * n_replicas elements"
        self.constraining_radius = float(constraining_radius)
        self.record_capacity = 0
        self.radial = int(radial)
        h = C.c_void_p()
        _check(lib().dzo_tempering_create(radial, self.n_particles, self.n_replicas, _dt(self.dtype), replicas.ptr,
                                          beta.ctypes.data_as(_P(_dbl)), rad.ctypes.data_as(_P(_dbl)), self.constraining_radius,
                                          _u64(base_seed), C.byref(h)))
        self.h = h

    @staticmethod
    def _trace(energies, ld, rows):
        if energies is None:
            return None, 0
        return energies.ptr, int(ld if ld is not None else (energies.shape[0] if len(energies.shape) == 2 else rows))

    def temper(self, num_steps, energies=None, ld=None):
        """``parallel_temper!``: ``energies[i + ld * k]`` is the energy of replica k after move i (``ld`` defaults to
        ``num_steps``)."""
        p, ld = self._trace(energies, ld, num_steps)
        _check(lib().dzo_tempering_temper(self.h, int(num_steps), p, ld))

    def swap(self, odd):
        _check(lib().dzo_tempering_swap(self.h, int(bool(odd))))

    def run(self, num_steps, num_batches, energies=None, ld=None):
        """The body of ``main``'s loop: per batch temper, swap(false), temper, swap(true); ``energies`` holds
        ``2 * num_steps * num_batches`` rows per replica."""
        p, ld = self._trace(energies, ld, 2 * num_steps * num_batches)
        _check(lib().dzo_tempering_run(self.h, int(num_steps), int(num_batches), p, ld))

    def analyze(self, energies, n_iterations, ld=None):
        """``analyze``: (cv, cv_prime, moments) with moments[k] = (V1, V2, V3), as float64 arrays holding values of T."""
        p, ld = self._trace(energies, ld, n_iterations)
        r = self.n_replicas
        cv, cvp, mom = np.empty(r), np.empty(r), np.empty((r, 3))
        _check(lib().dzo_tempering_analyze(self.h, int(n_iterations), p, ld, cv.ctypes.data_as(_P(_dbl)), cvp.ctypes.data_as(_P(_dbl)),
                                           mom.ctypes.data_as(_P(_dbl))))
        return cv, cvp, mom

    def set_record(self, capacity_steps):
        _check(lib().dzo_tempering_set_record(self.h, int(capacity_steps)))
        self.record_capacity = int(capacity_steps)

    def _shape(self, what):
        r, cap = self.n_replicas, self.record_capacity
        return {TEMPERING_REPLICAS: ((r, 3, self.n_particles), self.dtype), TEMPERING_RADII: ((r,), self.dtype),
                TEMPERING_INV_TEMPS: ((r,), self.dtype), TEMPERING_NUM_ACCEPT: ((r,), np.int64), TEMPERING_NUM_REJECT: ((r,), np.int64),
                TEMPERING_RNG_STATES: ((r,), np.uint64), TEMPERING_REC_INDEX: ((r, cap), np.int32),
                TEMPERING_REC_NORMALS: ((r, cap, 3), self.dtype), TEMPERING_REC_UNIFORM: ((r, cap), self.dtype),
                TEMPERING_REC_CODE: ((r, cap), np.int8), TEMPERING_REC_SWAP: ((r,), np.int8),
                TEMPERING_REC_SWAP_LOGP: ((r,), self.dtype)}[what]

    coordinates = property(lambda self: self.read(TEMPERING_REPLICAS))
    inverse_temperatures = property(lambda self: self.read(TEMPERING_INV_TEMPS))
    perturbation_radii = property(lambda self: self.read(TEMPERING_RADII), lambda self, v: self._set(TEMPERING_RADII, v))
    rng_states = property(lambda self: self.read(TEMPERING_RNG_STATES), lambda self, v: self._set(TEMPERING_RNG_STATES, v))
    num_accept = property(lambda self: self.read(TEMPERING_NUM_ACCEPT))
    num_reject = property(lambda self: self.read(TEMPERING_NUM_REJECT))

    def quench(self, history_length=10, initial_step_length=0.01, steps_per_launch=50, max_steps=2000, optimizer="lbfgs"):
        """The inherent structures of the replicas: a device-to-device COPY of the replica array is quenched by a
        ``BatchedLBFGS`` (``steps_per_launch`` calls of ``step!()`` per launch until every instance is stuck, at most
        ``max_steps`` per instance).  ``optimizer="adgd"`` quenches the copy with a ``BatchedAdGD`` instead
        (``history_length`` is ignored).  Returns ``(energies, copy, optimizer)``: the minima's energies (host array), the
        DeviceArray that holds them, and the handle (its ``is_stuck`` tells which instances finished).  The Markov chain's
        own array is not touched.  The quench runs under the radial the tempering was created with."""
        assert optimizer in ("lbfgs", "adgd"), "optimizer must be 'lbfgs' or 'adgd'"
        minima = self.replicas.copy()
        if optimizer == "adgd":
            opt = BatchedAdGD(minima, self.n_particles, initial_step_length, radial=self.radial)
        else:
            opt = BatchedLBFGS(minima, self.n_particles, initial_step_length, history_length, radial=self.radial)
        opt._run(max_steps, steps_per_launch)
        return opt.current_objective_values, minima, opt


# ------------------------------------------------------------------------------ batched L-BFGS over Lennard-Jones clusters
LBFGS_BATCH_MAX_PARTICLES = 1024
LBFGS_BATCH_MAX_HISTORY = 32
(LBFGS_BATCH_POINTS, LBFGS_BATCH_GRADIENTS, LBFGS_BATCH_DIRECTIONS, LBFGS_BATCH_DELTA_POINTS, LBFGS_BATCH_DELTA_GRADIENTS,
 LBFGS_BATCH_OBJECTIVES, LBFGS_BATCH_DELTA_OBJECTIVES, LBFGS_BATCH_IS_STUCK, LBFGS_BATCH_ITERATION_COUNTS,
 LBFGS_BATCH_HISTORY_COUNTS, LBFGS_BATCH_S, LBFGS_BATCH_Y, LBFGS_BATCH_RHO, LBFGS_BATCH_LAST_HALVINGS) = range(14)


def pairwise_batch_energy_gradient(points, n_particles, gradients=None, radial=RADIAL_LENNARD_JONES):
    """Energy (host array, one per instance) of every instance of ``points`` (``3 * n_particles * batch`` elements, instance b
    ``[x | y | z]`` at ``3 * n_particles * b``) and, into ``gradients`` when given, its gradient: the device routine and the
    summation order of ``BatchedLBFGS``."""
    n, batch = _batch_of(points, n_particles, least=1)
    e = DeviceArray(batch, points.dtype)
    _check(lib().dzo_pairwise_batch_energy_gradient(radial, n, batch, _dt(points.dtype), points.ptr, e.ptr,
                                                    gradients.ptr if gradients is not None else None))
    return e.to_host()


class _ClusterHandle(_HandleArrays):
    """A handle over ``points``: a DeviceArray of ``3 * n_particles * batch`` elements (the tempering replica layout), aliased.
    A subclass calls ``_create`` with the arguments that follow ``points`` in its ``create`` entry."""

    def _create(self, points, n_particles, radial, *args, batch=None):
        """Adopts ``points`` and creates the handle; ``batch``: where it is not the points' to tell (one per walker)."""
        _need_init()
        self.points = points
        self.dtype = points.dtype
        self.n_particles, self.batch = _batch_of(points, n_particles, batch=batch)
        h = C.c_void_p()
        self._call("create", radial, self.n_particles, self.batch, _dt(self.dtype), points.ptr, *args, C.byref(h))
        self.h = h


class _SteppedCluster(_ClusterHandle):
    """A cluster handle whose unit has the entries ``step`` and ``count_active``: an instance is active until it is stuck,
    converged or failed, and ``step`` moves the active ones."""

    def step(self, steps=1, wait=True):
        """``steps`` steps (calls of ``step!()``) of every active instance.  ``wait=True``: blocks and returns whether no
        instance is active any more; ``wait=False``: enqueues only and returns None."""
        flag = C.c_int32(0) if wait else None
        self._call("step", self.h, int(steps), C.byref(flag) if wait else None)
        return bool(flag.value) if wait else None

    def count_active(self):
        n = C.c_int64(0)
        self._call("count_active", self.h, C.byref(n))
        return int(n.value)

    def _run(self, max_steps, steps_per_call):
        """Steps in chunks of ``steps_per_call`` until no instance is active, at most ``max_steps`` per instance.  Returns the
        steps enqueued."""
        done, taken = self.count_active() == 0, 0
        while not done and taken < max_steps:
            k = min(int(steps_per_call), int(max_steps) - taken)
            done = self.step(k)
            taken += k
        return taken


class _BatchedOptimizer(_SteppedCluster):
    """What ``BatchedLBFGS`` and ``BatchedAdGD`` share.  A subclass names the ``what`` constants of the arrays both have
    (``_what``: property name -> constant) and has ``_shape(what)``."""
    _what = {}

    def set_max_halvings(self, v):
        self._call("set_max_halvings", self.h, int(v))

    current_points = property(lambda self: self.read(self._what["current_points"]))
    current_gradients = property(lambda self: self.read(self._what["current_gradients"]))
    current_objective_values = property(lambda self: self.read(self._what["current_objective_values"]))
    delta_points = property(lambda self: self.read(self._what["delta_points"]))
    delta_gradients = property(lambda self: self.read(self._what["delta_gradients"]))
    delta_objective_values = property(lambda self: self.read(self._what["delta_objective_values"]))
    is_stuck = property(lambda self: self.read(self._what["is_stuck"]).astype(bool))
    iteration_counts = property(lambda self: self.read(self._what["iteration_counts"]))
    last_halvings = property(lambda self: self.read(self._what["last_halvings"]))


class BatchedLBFGS(_BatchedOptimizer):
    """``LBFGSOptimizer`` (src/DZOptimization.jl:321-509, no constraint) of many small Lennard-Jones clusters at once:
    ``step(k)`` runs k calls of ``step!()`` of every instance in ONE launch.  ``points`` is a DeviceArray of
    ``3 * n_particles * batch`` elements (the tempering replica layout); it is aliased, as the live constructor aliases
    ``initial_point``.  Arrays come back instance-major (row b = instance b)."""
    _prefix = "dzo_lbfgs_batch_"
    _what = dict(current_points=LBFGS_BATCH_POINTS, current_gradients=LBFGS_BATCH_GRADIENTS, current_objective_values=LBFGS_BATCH_OBJECTIVES,
                 delta_points=LBFGS_BATCH_DELTA_POINTS, delta_gradients=LBFGS_BATCH_DELTA_GRADIENTS,
                 delta_objective_values=LBFGS_BATCH_DELTA_OBJECTIVES, is_stuck=LBFGS_BATCH_IS_STUCK,
                 iteration_counts=LBFGS_BATCH_ITERATION_COUNTS, last_halvings=LBFGS_BATCH_LAST_HALVINGS)

    def __init__(self, points, n_particles, initial_step_length, history_length, radial=RADIAL_LENNARD_JONES):
        self.history_length = int(history_length)
        self._create(points, n_particles, radial, float(initial_step_length), self.history_length)

    def _shape(self, what):
        b, n3, m = self.batch, 3 * self.n_particles, self.history_length
        vec, sc = ((b, n3), self.dtype), ((b,), self.dtype)
        return {LBFGS_BATCH_POINTS: vec, LBFGS_BATCH_GRADIENTS: vec, LBFGS_BATCH_DIRECTIONS: vec, LBFGS_BATCH_DELTA_POINTS: vec,
                LBFGS_BATCH_DELTA_GRADIENTS: vec, LBFGS_BATCH_OBJECTIVES: sc, LBFGS_BATCH_DELTA_OBJECTIVES: sc,
                LBFGS_BATCH_IS_STUCK: ((b,), np.int32), LBFGS_BATCH_ITERATION_COUNTS: ((b,), np.int64),
                LBFGS_BATCH_HISTORY_COUNTS: ((b,), np.int32), LBFGS_BATCH_S: ((b, m, n3), self.dtype),
                LBFGS_BATCH_Y: ((b, m, n3), self.dtype), LBFGS_BATCH_RHO: ((b, m), np.float64),
                LBFGS_BATCH_LAST_HALVINGS: ((b,), np.int32)}[what]

    step_directions = property(lambda self: self.read(LBFGS_BATCH_DIRECTIONS))
    history_counts = property(lambda self: self.read(LBFGS_BATCH_HISTORY_COUNTS))


# ------------------------------------------------------------------------------ the Thomson problem: Riesz energy on the unit sphere
SPHERE_ENERGY_RIESZ1 = 0


def sphere_project_(points, n_particles):
    """Projects every particle of every instance of ``points`` (``3 * n_particles * batch`` elements, instance b ``[x | y | z]``
    at ``3 * n_particles * b``) onto the unit sphere, in place: ``p / |p|`` by one square root and three IEEE divisions, the
    ``constraint_function!`` of ``SphereLBFGS``.  Returns ``points``."""
    n, batch = _batch_of(points, n_particles, least=1)
    _check(lib().dzo_sphere_batch_project(n, batch, _dt(points.dtype), points.ptr))
    return points


def sphere_energy_gradient(points, n_particles, gradients=None, tangent=True):
    """Riesz (Coulomb, s = 1) energy (host array, one per instance) of every instance of ``points`` (the layout of
    ``sphere_project_``; the points are taken as they are) and, into ``gradients`` when given, its gradient: the raw
    ``riesz_gradient!`` of legacy/ExampleFunctions.jl:47-83 with ``tangent=False``, after ``constrain_riesz_gradient_sphere!``
    (:361-374) with ``tangent=True``.  The device routine and the summation order of ``SphereLBFGS``."""
    n, batch = _batch_of(points, n_particles, least=1)
    e = DeviceArray(batch, points.dtype)
    _check(lib().dzo_sphere_batch_energy_gradient(SPHERE_ENERGY_RIESZ1, n, batch, _dt(points.dtype), points.ptr, e.ptr,
                                                  gradients.ptr if gradients is not None else None, 1 if tangent else 0))
    return e.to_host()


class SphereLBFGS(_BatchedOptimizer):
    """``LBFGSOptimizer`` (src/DZOptimization.jl:321-509) with the unit sphere as its ``constraint_function!`` over many
    configurations of ``n_particles`` charges at once (the Thomson problem): the constrained sibling of ``BatchedLBFGS``, with
    its arrays and their shapes.  ``points`` is aliased and projected in place by the constructor (:412-414); every trial point
    is projected before it is evaluated (:133-135) and every gradient is made tangent."""
    _prefix = "dzo_sphere_lbfgs_batch_"
    _what = BatchedLBFGS._what
    _shape = BatchedLBFGS._shape

    def __init__(self, points, n_particles, initial_step_length, history_length, energy=SPHERE_ENERGY_RIESZ1):
        self.history_length = int(history_length)
        self._create(points, n_particles, energy, float(initial_step_length), self.history_length)

    step_directions = BatchedLBFGS.step_directions
    history_counts = BatchedLBFGS.history_counts


# ------------------------------------------------------------------------------ batched basin hopping over Lennard-Jones clusters
BASIN_HOPPING_MAX_PARTICLES = 1024
(BASIN_HOPPING_POINTS, BASIN_HOPPING_ENERGIES, BASIN_HOPPING_BEST_POINTS, BASIN_HOPPING_BEST_ENERGIES, BASIN_HOPPING_RADII,
 BASIN_HOPPING_INV_TEMPS, BASIN_HOPPING_NUM_ACCEPT, BASIN_HOPPING_NUM_REJECT, BASIN_HOPPING_RNG_STATES, BASIN_HOPPING_HOP_COUNTS,
 BASIN_HOPPING_QUENCH_ITERATIONS, BASIN_HOPPING_QUENCH_UNFINISHED, BASIN_HOPPING_REC_NORMALS, BASIN_HOPPING_REC_UNIFORM,
 BASIN_HOPPING_REC_TRIAL_ENERGY, BASIN_HOPPING_REC_QUENCH_ITERATIONS, BASIN_HOPPING_REC_CODE) = range(17)


class BasinHopping(_ClusterHandle):
    """Basin hopping (Monte Carlo over the quenched landscape) of many walkers over Lennard-Jones clusters: ``hop(k)`` runs k
    hops -- perturb every particle, quench with the batched L-BFGS, Metropolis test on the quenched energies -- of every walker
    at the walker's own pace, ``hops_per_launch`` hops per launch.  ``points`` is a DeviceArray of ``3 * n_particles * batch``
    elements (the quench's layout); it is aliased and always holds the walkers' current minima.  ``inverse_temperatures`` and
    ``perturbation_radii`` are host sequences, one per walker.  The rule is in include/dzo.h.

    The constructor and ``hop(wait=False)`` do not block; every property that reads device state does."""
    _prefix = "dzo_basin_hopping_"

    def __init__(self, points, n_particles, inverse_temperatures, perturbation_radii, constraining_radius, initial_step_length=0.01,
                 history_length=10, quench_steps=400, base_seed=0, radial=RADIAL_LENNARD_JONES):
        beta, rad = _per_walker(inverse_temperatures, perturbation_radii)
        self.constraining_radius = float(constraining_radius)
        self.history_length, self.quench_steps = int(history_length), int(quench_steps)
        self.record_capacity = 0
        self._create(points, n_particles, radial, beta.ctypes.data_as(_P(_dbl)), rad.ctypes.data_as(_P(_dbl)), self.constraining_radius,
                     float(initial_step_length), self.history_length, self.quench_steps, _u64(base_seed), batch=beta.size)

    def set_max_halvings(self, v):
        self._call("set_max_halvings", self.h, int(v))

    def hop(self, num_hops, adapt=True, hops_per_launch=8, wait=True):
        """``num_hops`` hops of every walker in ``ceil(num_hops / hops_per_launch)`` launches (a launch lasts as long as its
        slowest walker's quenches: keep it short).  With ``adapt`` the radii are adapted once, at the end of the last launch,
        on that launch's counts.  ``wait=False`` enqueues only."""
        num_hops, per = int(num_hops), int(hops_per_launch)
        assert num_hops >= 0 and per >= 1
        done = 0
        while done < num_hops:
            k = min(per, num_hops - done)
            done += k
            _check(lib().dzo_basin_hopping_hop(self.h, k, int(bool(adapt) and done == num_hops)))
        if wait:
            synchronize()

    def set_record(self, capacity_hops):
        _check(lib().dzo_basin_hopping_set_record(self.h, int(capacity_hops)))
        self.record_capacity = int(capacity_hops)

    def _shape(self, what):
        b, n, cap = self.batch, self.n_particles, self.record_capacity
        vec, sc, cnt = ((b, 3 * n), self.dtype), ((b,), self.dtype), ((b,), np.int64)
        return {BASIN_HOPPING_POINTS: vec, BASIN_HOPPING_ENERGIES: sc, BASIN_HOPPING_BEST_POINTS: vec, BASIN_HOPPING_BEST_ENERGIES: sc,
                BASIN_HOPPING_RADII: sc, BASIN_HOPPING_INV_TEMPS: sc, BASIN_HOPPING_NUM_ACCEPT: cnt, BASIN_HOPPING_NUM_REJECT: cnt,
                BASIN_HOPPING_RNG_STATES: ((b,), np.uint64), BASIN_HOPPING_HOP_COUNTS: cnt, BASIN_HOPPING_QUENCH_ITERATIONS: cnt,
                BASIN_HOPPING_QUENCH_UNFINISHED: cnt, BASIN_HOPPING_REC_NORMALS: ((b, cap, n, 3), self.dtype),
                BASIN_HOPPING_REC_UNIFORM: ((b, cap), self.dtype), BASIN_HOPPING_REC_TRIAL_ENERGY: ((b, cap), self.dtype),
                BASIN_HOPPING_REC_QUENCH_ITERATIONS: ((b, cap), np.int32), BASIN_HOPPING_REC_CODE: ((b, cap), np.int8)}[what]

    current_points = property(lambda self: self.read(BASIN_HOPPING_POINTS))
    energies = property(lambda self: self.read(BASIN_HOPPING_ENERGIES))
    best_points = property(lambda self: self.read(BASIN_HOPPING_BEST_POINTS))
    best_energies = property(lambda self: self.read(BASIN_HOPPING_BEST_ENERGIES))
    inverse_temperatures = property(lambda self: self.read(BASIN_HOPPING_INV_TEMPS))
    perturbation_radii = property(lambda self: self.read(BASIN_HOPPING_RADII), lambda self, v: self._set(BASIN_HOPPING_RADII, v))
    rng_states = property(lambda self: self.read(BASIN_HOPPING_RNG_STATES), lambda self, v: self._set(BASIN_HOPPING_RNG_STATES, v))
    num_accept = property(lambda self: self.read(BASIN_HOPPING_NUM_ACCEPT))
    num_reject = property(lambda self: self.read(BASIN_HOPPING_NUM_REJECT))
    hop_counts = property(lambda self: self.read(BASIN_HOPPING_HOP_COUNTS))
    quench_iterations = property(lambda self: self.read(BASIN_HOPPING_QUENCH_ITERATIONS))
    quench_unfinished = property(lambda self: self.read(BASIN_HOPPING_QUENCH_UNFINISHED))


# ------------------------------------------------------------------------------ batched AdGD over Lennard-Jones clusters
ADGD_BATCH_MAX_PARTICLES = 1024
(ADGD_BATCH_POINTS, ADGD_BATCH_GRADIENTS, ADGD_BATCH_DELTA_POINTS, ADGD_BATCH_DELTA_GRADIENTS, ADGD_BATCH_OBJECTIVES,
 ADGD_BATCH_DELTA_OBJECTIVES, ADGD_BATCH_IS_STUCK, ADGD_BATCH_ITERATION_COUNTS, ADGD_BATCH_CURRENT_STEP_SIZES,
 ADGD_BATCH_PREVIOUS_STEP_SIZES, ADGD_BATCH_LAST_HALVINGS) = range(11)


class BatchedAdGD(_BatchedOptimizer):
    """``AdGDOptimizer`` (src/DZOptimization.jl:179-312, no constraint) of many small Lennard-Jones clusters at once:
    ``step(k)`` runs k calls of ``step!()`` of every instance in ONE launch.  ``points`` is a DeviceArray of
    ``3 * n_particles * batch`` elements (the tempering replica layout); it is aliased, as the live constructor aliases
    ``initial_point``.  Arrays come back instance-major (row b = instance b)."""
    _prefix = "dzo_adgd_batch_"
    _what = dict(current_points=ADGD_BATCH_POINTS, current_gradients=ADGD_BATCH_GRADIENTS, current_objective_values=ADGD_BATCH_OBJECTIVES,
                 delta_points=ADGD_BATCH_DELTA_POINTS, delta_gradients=ADGD_BATCH_DELTA_GRADIENTS,
                 delta_objective_values=ADGD_BATCH_DELTA_OBJECTIVES, is_stuck=ADGD_BATCH_IS_STUCK,
                 iteration_counts=ADGD_BATCH_ITERATION_COUNTS, last_halvings=ADGD_BATCH_LAST_HALVINGS)

    def __init__(self, points, n_particles, initial_step_length, radial=RADIAL_LENNARD_JONES):
        self._create(points, n_particles, radial, float(initial_step_length))

    def _shape(self, what):
        b, n3 = self.batch, 3 * self.n_particles
        vec, sc = ((b, n3), self.dtype), ((b,), self.dtype)
        return {ADGD_BATCH_POINTS: vec, ADGD_BATCH_GRADIENTS: vec, ADGD_BATCH_DELTA_POINTS: vec, ADGD_BATCH_DELTA_GRADIENTS: vec,
                ADGD_BATCH_OBJECTIVES: sc, ADGD_BATCH_DELTA_OBJECTIVES: sc, ADGD_BATCH_IS_STUCK: ((b,), np.int32),
                ADGD_BATCH_ITERATION_COUNTS: ((b,), np.int64), ADGD_BATCH_CURRENT_STEP_SIZES: sc,
                ADGD_BATCH_PREVIOUS_STEP_SIZES: sc, ADGD_BATCH_LAST_HALVINGS: ((b,), np.int32)}[what]

    current_step_sizes = property(lambda self: self.read(ADGD_BATCH_CURRENT_STEP_SIZES))
    previous_step_sizes = property(lambda self: self.read(ADGD_BATCH_PREVIOUS_STEP_SIZES))


# ------------------------------------------------------------------------------ batched Hessians of Lennard-Jones clusters
HESSIAN_BATCH_MAX_PARTICLES = 1024


def pairwise_batch_hvp(points, directions, n_particles, products=None, curvatures=False, shared_point=False,
                       radial=RADIAL_LENNARD_JONES):
    """``accelerated_pairwise_radial_hvp!`` (src/ExampleFunctions.jl:367-468) of every instance in one launch.  ``directions``
    is a DeviceArray of ``3 * n_particles * batch`` elements, instance b ``[u | v | w]`` at ``3 * n_particles * b``; ``points``
    has the same layout, or with ``shared_point=True`` holds ONE point to which every direction is applied.  The products go
    into ``products`` (allocated when None).  Returns the products' DeviceArray, or with ``curvatures=True`` the pair
    ``(products, c)`` where ``c`` is a host array ``(batch, 2)`` of ``u.Hu`` and ``u.u`` in fp64."""
    n, batch = _batch_of(directions, n_particles, "directions", least=1)
    assert points.size == (3 * n if shared_point else 3 * n * batch), "points must hold one point per instance, or one point when shared"
    assert points.dtype == directions.dtype, "points and directions must have one element type"
    if products is None:
        products = DeviceArray(directions.shape, directions.dtype)
    assert products.size == directions.size and products.dtype == directions.dtype
    curv = DeviceArray((batch, 2), np.float64) if curvatures else None
    _check(lib().dzo_pairwise_batch_hvp(radial, n, batch, _dt(points.dtype), points.ptr, 0 if shared_point else 3 * n, directions.ptr,
                                        products.ptr, curv.ptr if curvatures else None))
    return (products, curv.to_host()) if curvatures else products


def pairwise_batch_hessian(points, n_particles, out=None, radial=RADIAL_LENNARD_JONES):
    """The dense ``3N x 3N`` Hessian of every instance of ``points`` (``3 * n_particles * batch`` elements, instance b
    ``[x | y | z]``) from one launch.  Returns a host array ``[b, c, r]``: column c, row r of instance b (the device layout,
    column-major per instance).  ``out``: a DeviceArray of ``9 * n_particles**2 * batch`` elements to hold the device copy."""
    n, batch = _batch_of(points, n_particles, least=1)
    if out is None:
        out = DeviceArray((batch, 3 * n, 3 * n), points.dtype)
    assert out.size == 9 * n * n * batch and out.dtype == points.dtype
    _check(lib().dzo_pairwise_batch_hessian(radial, n, batch, _dt(points.dtype), points.ptr, out.ptr))
    return out.to_host().reshape(batch, 3 * n, 3 * n)


def hessian_eigenvalues(points, n_particles, radial=RADIAL_LENNARD_JONES):
    """Eigenvalues of the Hessian of every instance, ascending, as a ``(batch, 3N)`` fp64 host array: the device Hessians,
    symmetrised as ``(H + H^T) / 2`` in fp64 on the host (the device does not promise bitwise symmetry), then
    ``numpy.linalg.eigvalsh``."""
    h = pairwise_batch_hessian(points, n_particles, radial=radial).astype(np.float64)
    return np.linalg.eigvalsh(0.5 * (h + h.transpose(0, 2, 1)))


def morse_index(eigenvalues, zero_tol):
    """``(negatives, zeros)`` per instance: the eigenvalues below ``-zero_tol`` (the Morse index) and those with
    ``|lambda| <= zero_tol`` (six rigid-body modes for a cluster in free space).  ``zero_tol`` is an absolute value in the
    eigenvalues' unit and depends on the element type and on the scale of the spectrum: there is no default."""
    ev = np.atleast_2d(np.asarray(eigenvalues, dtype=np.float64))
    tol = float(zero_tol)
    return (ev < -tol).sum(axis=1), (np.abs(ev) <= tol).sum(axis=1)


# ------------------------------------------------------------------------------ batched symmetric eigensolver
SYMEIG_MAX_N = 384
SYMEIG_STORAGE_LDS, SYMEIG_STORAGE_MEMORY = 0, 1


def symeig_plan(n, dtype):
    """``(storage, ld, lds_bytes)`` of ``dzo_symeig_plan``: where the eigensolver keeps an ``n x n`` matrix of ``dtype`` while
    it iterates.  A pure function; needs no device."""
    storage, ld, lds = C.c_int32(), C.c_int64(), C.c_int64()
    _check(lib().dzo_symeig_plan(int(n), _dt(dtype), C.byref(storage), C.byref(ld), C.byref(lds)))
    return storage.value, ld.value, lds.value


def _symeig_device(matrices, n, batch, vectors, max_sweeps, want_sweeps=True):
    """The device call on a DeviceArray of matrices: DeviceArrays (eigenvalues, eigenvectors or None, sweeps or None)."""
    w = DeviceArray((batch, n), matrices.dtype)
    v = DeviceArray((batch, n, n), matrices.dtype) if vectors else None
    s = DeviceArray((batch,), np.int32) if want_sweeps else None
    _check(lib().dzo_symmetric_batch_eigen(n, batch, _dt(matrices.dtype), matrices.ptr, w.ptr, v.ptr if vectors else None,
                                           s.ptr if want_sweeps else None, int(max_sweeps)))
    return w, v, s


def symmetric_batch_eigen(matrices, n, vectors=False, max_sweeps=0):
    """Eigenvalues, ascending, and with ``vectors=True`` eigenvectors of the symmetric part of every ``n x n`` matrix of
    ``matrices``, on the device in one launch (``dzo_symmetric_batch_eigen``: cyclic Jacobi, one block per matrix).  ``matrices``
    is a DeviceArray of ``n * n * batch`` elements, column-major per instance (what ``pairwise_batch_hessian`` writes into its
    ``out``), or a host array ``(batch, n, n)`` indexed ``[b, c, r]``, which is uploaded.  Returns host arrays: the eigenvalues
    ``(batch, n)`` in the element type, the eigenvectors ``(batch, n, n)`` in the device layout (``[b, k, :]`` is the vector of
    eigenvalue k) or None, and the sweeps ``(batch,)`` each instance ran, -1 where ``max_sweeps`` (0: the default, 30) did not
    suffice.  The matrices are not modified."""
    n = int(n)
    if not isinstance(matrices, DeviceArray):
        matrices = DeviceArray.from_host(matrices)
    batch = matrices.size // (n * n) if n > 0 else 0
    assert n >= 1 and matrices.size == n * n * batch and batch >= 1, "matrices must hold n * n * batch elements"
    w, v, s = _symeig_device(matrices, n, batch, vectors, max_sweeps)
    return w.to_host().reshape(batch, n), (v.to_host().reshape(batch, n, n) if vectors else None), s.to_host().reshape(batch)


def hessian_spectrum(points, n_particles, vectors=False, radial=RADIAL_LENNARD_JONES):
    """The spectrum of the Hessian of every instance of ``points`` without leaving the device: ``dzo_pairwise_batch_hessian``
    into ``dzo_symmetric_batch_eigen``; only the results travel to the host.  Returns the eigenvalues, ascending, as a
    ``(batch, 3N)`` fp64 host array, or with ``vectors=True`` the pair ``(eigenvalues, eigenvectors)`` with the eigenvectors
    ``(batch, 3N, 3N)`` in the points' element type (``[b, k, :]`` is the normal mode of eigenvalue k).  Raises when an
    instance did not converge (non-finite Hessian: coincident particles)."""
    n, batch = _batch_of(points, n_particles, least=1)
    h = DeviceArray((batch, 3 * n, 3 * n), points.dtype)
    _check(lib().dzo_pairwise_batch_hessian(radial, n, batch, _dt(points.dtype), points.ptr, h.ptr))
    w, v, s = _symeig_device(h, 3 * n, batch, vectors, 0)
    sweeps = s.to_host().reshape(batch)
    if np.any(sweeps < 0):
        raise DzoError(6, "hessian_spectrum: no convergence in instances %s" % np.flatnonzero(sweeps < 0).tolist())
    ev = w.to_host().reshape(batch, 3 * n).astype(np.float64)
    return (ev, v.to_host().reshape(batch, 3 * n, 3 * n)) if vectors else ev


# ------------------------------------------------------------------------------ batched lowest Hessian mode (Lanczos)
LOWMODE_MAX_PARTICLES = 1024
LOWMODE_MAX_KRYLOV = 32
LOWMODE_CONVERGED, LOWMODE_UNFINISHED, LOWMODE_FAILED = 0, 1, 2
# relative residual an instance is asked to reach by default: 16 times the smallest the CPU twin of the iteration still reaches
# within 20 cycles on the 38-atom octahedron and on a 257-atom cluster (DESIGN.md has the two numbers per element type)
LOWMODE_DEFAULT_RES_TOL = {np.dtype(np.float64): 4.3e-15, np.dtype(np.float32): 7.0e-7}


class LowestModes:
    """What ``lowest_modes`` returns: ``eigenvalues`` (host, ``(batch,)`` in the element type), ``vectors`` (a DeviceArray
    ``(batch, 3N)``, unit norm), ``residuals`` (host, fp64), ``status``, ``cycles`` and ``products`` (host, int32)."""

    def __init__(self, eigenvalues, vectors, residuals, info):
        self.eigenvalues, self.vectors, self.residuals = eigenvalues, vectors, residuals
        self.status, self.cycles, self.products = info[:, 0].copy(), info[:, 1].copy(), info[:, 2].copy()


def lowest_modes(points, n_particles, project_rigid=True, krylov=32, max_cycles=40, res_tol=None, start=None, seed=0,
                 radial=RADIAL_LENNARD_JONES):
    """The lowest eigenpair of the Hessian of every instance of ``points`` (``3 * n_particles * batch`` elements, instance b
    ``[x | y | z]``) by restarted Lanczos inside one launch (``dzo_pairwise_batch_lowest_mode``, include/dzo.h): Hessian-vector
    products only, up to 1024 particles.  With ``project_rigid`` net translation and rotation are projected out, so that the
    eigenvalue is the lowest vibration (a minimum has it positive, a saddle negative); without, it is the lowest eigenvalue
    of the Hessian itself.  ``krylov`` Lanczos vectors per cycle (2 .. 32), at most ``max_cycles`` cycles; an instance is
    CONVERGED when the residual of its Ritz pair is at most ``res_tol`` times the largest eigenvalue estimate seen
    (None: ``LOWMODE_DEFAULT_RES_TOL`` of the element type).  ``start``: a DeviceArray of start vectors laid out like
    ``points``, or None to draw them in the kernel from ``seed``.  Returns a ``LowestModes``."""
    n, batch = _batch_of(points, n_particles, least=1)
    assert start is None or (start.size == points.size and start.dtype == points.dtype), "start must be laid out like points"
    if res_tol is None:
        res_tol = LOWMODE_DEFAULT_RES_TOL[np.dtype(points.dtype)]
    w = DeviceArray((batch,), points.dtype)
    v = DeviceArray((batch, 3 * n), points.dtype)
    r = DeviceArray((batch,), np.float64)
    info = DeviceArray((batch, 3), np.int32)
    _check(lib().dzo_pairwise_batch_lowest_mode(radial, n, batch, _dt(points.dtype), points.ptr, 1 if project_rigid else 0, int(krylov),
                                                int(max_cycles), float(res_tol), _u64(seed),
                                                start.ptr if start is not None else None, w.ptr, v.ptr, r.ptr, info.ptr))
    return LowestModes(w.to_host(), v, r.to_host(), info.to_host().reshape(batch, 3))


# ------------------------------------------------------------------------------ batched eigenvector following
MODEFOLLOW_MAX_PARTICLES = 128
MODEFOLLOW_ACTIVE, MODEFOLLOW_CONVERGED, MODEFOLLOW_FAILED = 0, 1, 2
(MODEFOLLOW_POINTS, MODEFOLLOW_GRADIENTS, MODEFOLLOW_ENERGIES, MODEFOLLOW_GRMS, MODEFOLLOW_STATUS, MODEFOLLOW_INDEX, MODEFOLLOW_ZEROS,
 MODEFOLLOW_FOLLOWED_MODE, MODEFOLLOW_STEP_LENGTHS, MODEFOLLOW_ITERATION_COUNTS, MODEFOLLOW_EIGENVALUES, MODEFOLLOW_EIGENVECTORS,
 MODEFOLLOW_SWEEPS, MODEFOLLOW_FOLLOW) = range(14)


def modefollow_apply(points, eigenvalues, eigenvectors, n_particles, target_index=0, start_mode=0, max_step=0.2, zero_tol=1e-4,
                     grad_tol=0.0, follow=None, follow_set=None, radial=RADIAL_LENNARD_JONES):
    """``dzo_modefollow_batch_apply``: ONE eigenvector-following step (include/dzo.h) of every instance from modes the caller
    supplies.  ``points`` (DeviceArray, ``3 * n_particles * batch`` elements) is moved in place; ``eigenvalues`` ``(batch, 3N)``
    ascending and ``eigenvectors`` ``(batch, 3N, 3N)`` in the device layout (``[b, k, :]`` is the vector of eigenvalue k) are
    DeviceArrays or host arrays, which are uploaded.  ``target_index=1`` needs ``follow`` (DeviceArray ``(batch, 3N)``, updated)
    and ``follow_set`` (DeviceArray of int32 ``(batch,)``, updated).  Returns a dict of host arrays: ``energies``, ``gradients``,
    ``projections`` (F), ``grms``, ``status``, ``index``, ``zeros``, ``followed_mode``, ``step_lengths``."""
    n, batch = _batch_of(points, n_particles, least=1)
    n3 = 3 * n
    lam, vec = _as_dev(eigenvalues, points.dtype), _as_dev(eigenvectors, points.dtype)
    assert lam.dtype == points.dtype and vec.dtype == points.dtype, "points and modes must have one element type"
    assert lam.size == n3 * batch and vec.size == n3 * n3 * batch, "modes must hold 3N and 3N * 3N elements per instance"
    if int(target_index) == 1:
        assert follow is not None and follow_set is not None, "target_index=1 needs follow and follow_set"
        assert follow.size == n3 * batch and follow.dtype == points.dtype and follow_set.size == batch and follow_set.dtype == np.int32
    e, g, f = DeviceArray(batch, points.dtype), DeviceArray((batch, n3), points.dtype), DeviceArray.zeros((batch, n3), points.dtype)
    grms, sl = DeviceArray(batch, np.float64), DeviceArray(batch, np.float64)
    st, ix, zr, fm = (DeviceArray(batch, np.int32) for _ in range(4))
    _check(lib().dzo_modefollow_batch_apply(radial, n, batch, _dt(points.dtype), points.ptr, lam.ptr, vec.ptr,
                                            follow.ptr if follow is not None else None, follow_set.ptr if follow_set is not None else None,
                                            int(target_index), int(start_mode), float(max_step), float(zero_tol), float(grad_tol), e.ptr, g.ptr,
                                            f.ptr, grms.ptr, st.ptr, ix.ptr, zr.ptr, fm.ptr, sl.ptr))
    return dict(energies=e.to_host(), gradients=g.to_host(), projections=f.to_host(), grms=grms.to_host(), status=st.to_host(),
                index=ix.to_host(), zeros=zr.to_host(), followed_mode=fm.to_host(), step_lengths=sl.to_host())


class ModeFollowing(_SteppedCluster):
    """Eigenvector following (Cerjan-Miller / Wales; include/dzo.h states the step) of many small Lennard-Jones clusters at once:
    ``step(k)`` enqueues, k times, the dense Hessians, their eigenvalues and eigenvectors and the step kernel, with no host wait
    in between.  ``target_index=0`` polishes minima, ``target_index=1`` searches transition states.  ``points`` is a DeviceArray
    of ``3 * n_particles * batch`` elements (the tempering replica layout), aliased and moved.  An instance ends CONVERGED
    (``grms <= grad_tol``) or FAILED (non-finite values, no convergence of the eigensolver, no mode to follow) and is then left
    alone; ``index`` and ``zeros`` tell what kind of stationary point it ended on."""
    _prefix = "dzo_modefollow_batch_"

    def __init__(self, points, n_particles, target_index=0, max_step=0.2, zero_tol=1e-4, grad_tol=1e-10, radial=RADIAL_LENNARD_JONES):
        self._create(points, n_particles, radial, int(target_index), float(max_step), float(zero_tol), float(grad_tol))

    def set_start_mode(self, mode):
        self._call("set_start_mode", self.h, int(mode))

    def set_directions(self, directions):
        """An initial followed vector per instance: a DeviceArray or host array ``(batch, 3N)``."""
        d = _as_dev(directions, self.dtype)
        assert d.size == 3 * self.n_particles * self.batch and d.dtype == self.dtype
        self._call("set_directions", self.h, d.ptr)
        synchronize()                                       # `d` may be a temporary

    def run(self, max_steps, steps_per_call=10):
        """Steps until no instance is ACTIVE, at most ``max_steps`` per instance.  Returns the steps enqueued."""
        return self._run(max_steps, steps_per_call)

    def _shape(self, what):
        b, n3 = self.batch, 3 * self.n_particles
        vec, sc, i32, f64 = ((b, n3), self.dtype), ((b,), self.dtype), ((b,), np.int32), ((b,), np.float64)
        return {MODEFOLLOW_POINTS: vec, MODEFOLLOW_GRADIENTS: vec, MODEFOLLOW_ENERGIES: sc, MODEFOLLOW_GRMS: f64, MODEFOLLOW_STATUS: i32,
                MODEFOLLOW_INDEX: i32, MODEFOLLOW_ZEROS: i32, MODEFOLLOW_FOLLOWED_MODE: i32, MODEFOLLOW_STEP_LENGTHS: f64,
                MODEFOLLOW_ITERATION_COUNTS: ((b,), np.int64), MODEFOLLOW_EIGENVALUES: vec,
                MODEFOLLOW_EIGENVECTORS: ((b, n3, n3), self.dtype), MODEFOLLOW_SWEEPS: i32, MODEFOLLOW_FOLLOW: vec}[what]

    current_points = property(lambda self: self.read(MODEFOLLOW_POINTS))
    current_gradients = property(lambda self: self.read(MODEFOLLOW_GRADIENTS))
    energies = property(lambda self: self.read(MODEFOLLOW_ENERGIES))
    grms = property(lambda self: self.read(MODEFOLLOW_GRMS))
    status = property(lambda self: self.read(MODEFOLLOW_STATUS))
    index = property(lambda self: self.read(MODEFOLLOW_INDEX))
    zeros = property(lambda self: self.read(MODEFOLLOW_ZEROS))
    followed_mode = property(lambda self: self.read(MODEFOLLOW_FOLLOWED_MODE))
    step_lengths = property(lambda self: self.read(MODEFOLLOW_STEP_LENGTHS))
    iteration_counts = property(lambda self: self.read(MODEFOLLOW_ITERATION_COUNTS))
    eigenvalues = property(lambda self: self.read(MODEFOLLOW_EIGENVALUES))
    eigenvectors = property(lambda self: self.read(MODEFOLLOW_EIGENVECTORS))
    sweeps = property(lambda self: self.read(MODEFOLLOW_SWEEPS))
    follow = property(lambda self: self.read(MODEFOLLOW_FOLLOW))


def polish_minima(points, n_particles, grad_tol=1e-10, max_steps=50, max_step=0.2, zero_tol=1e-4, radial=RADIAL_LENNARD_JONES):
    """Polishes the points a quench left at ``is_stuck`` (a DeviceArray, moved in place) with eigenvector following of target
    index 0 until ``grms <= grad_tol``, at most ``max_steps`` steps.  Returns the ``ModeFollowing`` handle: ``status``,
    ``energies``, ``grms``, ``index`` and ``zeros`` tell how every instance ended."""
    mf = ModeFollowing(points, n_particles, 0, max_step, zero_tol, grad_tol, radial)
    mf.run(max_steps)
    return mf


def find_saddles(minima, n_particles, start_mode=0, kick=0.05, grad_tol=1e-10, max_steps=300, max_step=0.1, zero_tol=1e-4,
                 polish_steps=50, radial=RADIAL_LENNARD_JONES):
    """Transition-state searches from the minima in ``minima`` (a DeviceArray, moved in place): polishes them
    (``polish_minima``), displaces every polished minimum by ``kick`` along its ``start_mode``-th non-zero eigenvector, sets that
    eigenvector as the followed vector and follows it uphill (target index 1) for at most ``max_steps`` steps.  Returns
    ``(saddles, polished)``: the two ``ModeFollowing`` handles; ``saddles.index == 1`` with ``status == MODEFOLLOW_CONVERGED``
    marks the transition states, ``polished.energies`` holds the minima's energies."""
    n3 = 3 * int(n_particles)
    polished = polish_minima(minima, n_particles, grad_tol, polish_steps, 0.2, zero_tol, radial)
    # the modes at the polished minima: those of the step that found them converged
    lam, vec, x = polished.eigenvalues.astype(np.float64), polished.eigenvectors, polished.current_points
    dirs = np.zeros((polished.batch, n3), dtype=minima.dtype)
    for b in range(polished.batch):
        nonzero = np.flatnonzero(np.abs(lam[b]) > float(zero_tol))
        if len(nonzero) > int(start_mode):
            dirs[b] = vec[b, nonzero[int(start_mode)]]
    minima.upload((x + np.asarray(kick, dtype=minima.dtype) * dirs).reshape(minima.shape))
    saddles = ModeFollowing(minima, n_particles, 1, max_step, zero_tol, grad_tol, radial)
    saddles.set_start_mode(start_mode)
    saddles.set_directions(dirs)
    saddles.run(max_steps)
    return saddles, polished


# ------------------------------------------------------------------------------ batched hybrid eigenvector following
HYBRIDEF_MAX_PARTICLES = 1024
HYBRIDEF_ACTIVE, HYBRIDEF_CONVERGED, HYBRIDEF_FAILED = 0, 1, 2
(HYBRIDEF_POINTS, HYBRIDEF_GRADIENTS, HYBRIDEF_ENERGIES, HYBRIDEF_GRMS, HYBRIDEF_STATUS, HYBRIDEF_EIGENVALUES, HYBRIDEF_MODES,
 HYBRIDEF_MODE_RESIDUALS, HYBRIDEF_PROJECTIONS, HYBRIDEF_UPHILL_STEPS, HYBRIDEF_TANGENT_STEPS, HYBRIDEF_ITERATION_COUNTS, HYBRIDEF_PRODUCTS,
 HYBRIDEF_EVALUATIONS) = range(14)


def hybridef_apply(points, eigenvalues, modes, n_particles, max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05,
                   tangent_first=0.01, zero_tol=1e-4, grad_tol=0.0, radial=RADIAL_LENNARD_JONES):
    """``dzo_hybridef_batch_apply``: ONE step of hybrid eigenvector following (include/dzo.h) of every instance from a mode the
    caller supplies.  ``points`` (DeviceArray, ``3 * n_particles * batch`` elements) is moved in place; ``eigenvalues``
    ``(batch,)`` and ``modes`` ``(batch, 3N)`` (unit vectors) are DeviceArrays or host arrays, which are uploaded.  Returns a
    dict of host arrays: ``energies``, ``gradients``, ``projections`` (F), ``uphill_steps`` (h), ``grms``, ``status``,
    ``tangent_steps``."""
    n, batch = _batch_of(points, n_particles, least=1)
    n3 = 3 * n
    lam, vec = _as_dev(eigenvalues, points.dtype), _as_dev(modes, points.dtype)
    assert lam.dtype == points.dtype and vec.dtype == points.dtype, "points and modes must have one element type"
    assert lam.size == batch and vec.size == n3 * batch, "a mode holds one eigenvalue and 3N elements per instance"
    e, g = DeviceArray(batch, points.dtype), DeviceArray((batch, n3), points.dtype)
    f, h = DeviceArray(batch, points.dtype), DeviceArray(batch, points.dtype)
    grms, st, ts = DeviceArray(batch, np.float64), DeviceArray(batch, np.int32), DeviceArray(batch, np.int32)
    _check(lib().dzo_hybridef_batch_apply(radial, n, batch, _dt(points.dtype), points.ptr, lam.ptr, vec.ptr, float(max_step), int(tangent_steps),
                                          int(tangent_steps_convex), float(tangent_cap), float(tangent_first), float(zero_tol), float(grad_tol),
                                          e.ptr, g.ptr, f.ptr, h.ptr, grms.ptr, st.ptr, ts.ptr))
    return dict(energies=e.to_host(), gradients=g.to_host(), projections=f.to_host(), uphill_steps=h.to_host(), grms=grms.to_host(),
                status=st.to_host(), tangent_steps=ts.to_host())


class HybridModeFollowing(_SteppedCluster):
    """Hybrid eigenvector following (Munro & Wales 1999; include/dzo.h states the step) of many Lennard-Jones clusters at once,
    up to 1024 particles: a transition-state search from Hessian-vector products and gradients alone.  ``step(k)`` enqueues, k
    times, the refinement of the lowest mode from the previous step's vector (``krylov`` Lanczos vectors, ``mode_cycles``
    cycles, stopped early at a relative residual of ``mode_tol``) and the step kernel -- uphill along the mode, then
    ``tangent_steps`` Barzilai-Borwein gradient steps orthogonal to it (``tangent_steps_convex`` while the mode's eigenvalue is
    not negative) -- with no host wait in between.  ``points`` is a DeviceArray of ``3 * n_particles * batch`` elements (the
    tempering replica layout), aliased and moved; ``directions`` ``(batch, 3N)`` are the first modes (None: drawn in the kernel
    from ``seed``).  An instance ends CONVERGED (``grms <= grad_tol``) or FAILED and is then left alone.  CONVERGED says that
    the point is stationary; ``eigenvalues < -zero_tol`` says that it is a saddle, and only the spectrum (``hessian_spectrum``,
    ``hessian_eigenvalues``) tells its index: the method can end on a saddle of higher index."""
    _prefix = "dzo_hybridef_batch_"

    def __init__(self, points, n_particles, directions=None, max_step=0.1, tangent_steps=10, tangent_steps_convex=2, tangent_cap=0.05,
                 tangent_first=0.01, krylov=8, mode_cycles=1, mode_tol=1e-3, zero_tol=1e-4, grad_tol=1e-10, seed=0,
                 radial=RADIAL_LENNARD_JONES):
        d = None if directions is None else _as_dev(directions, points.dtype)
        assert d is None or (d.size == points.size and d.dtype == points.dtype), "directions must be laid out like points"
        self._create(points, n_particles, radial, d.ptr if d is not None else None, float(max_step), int(tangent_steps),
                     int(tangent_steps_convex), float(tangent_cap), float(tangent_first), int(krylov), int(mode_cycles), float(mode_tol),
                     float(zero_tol), float(grad_tol), _u64(seed))

    def set_directions(self, directions):
        """The mode the next refinement of every instance starts from: a DeviceArray or host array ``(batch, 3N)``."""
        d = _as_dev(directions, self.dtype)
        assert d.size == 3 * self.n_particles * self.batch and d.dtype == self.dtype
        self._call("set_directions", self.h, d.ptr)
        synchronize()                                       # `d` may be a temporary

    def run(self, max_steps, steps_per_call=20):
        """Steps until no instance is ACTIVE, at most ``max_steps`` per instance.  Returns the steps enqueued."""
        return self._run(max_steps, steps_per_call)

    def _shape(self, what):
        b, n3 = self.batch, 3 * self.n_particles
        vec, sc, i32, i64, f64 = ((b, n3), self.dtype), ((b,), self.dtype), ((b,), np.int32), ((b,), np.int64), ((b,), np.float64)
        return {HYBRIDEF_POINTS: vec, HYBRIDEF_GRADIENTS: vec, HYBRIDEF_ENERGIES: sc, HYBRIDEF_GRMS: f64, HYBRIDEF_STATUS: i32,
                HYBRIDEF_EIGENVALUES: sc, HYBRIDEF_MODES: vec, HYBRIDEF_MODE_RESIDUALS: f64, HYBRIDEF_PROJECTIONS: sc, HYBRIDEF_UPHILL_STEPS: sc,
                HYBRIDEF_TANGENT_STEPS: i32, HYBRIDEF_ITERATION_COUNTS: i64, HYBRIDEF_PRODUCTS: i64, HYBRIDEF_EVALUATIONS: i64}[what]

    current_points = property(lambda self: self.read(HYBRIDEF_POINTS))
    current_gradients = property(lambda self: self.read(HYBRIDEF_GRADIENTS))
    energies = property(lambda self: self.read(HYBRIDEF_ENERGIES))
    grms = property(lambda self: self.read(HYBRIDEF_GRMS))
    status = property(lambda self: self.read(HYBRIDEF_STATUS))
    eigenvalues = property(lambda self: self.read(HYBRIDEF_EIGENVALUES))
    modes = property(lambda self: self.read(HYBRIDEF_MODES))
    mode_residuals = property(lambda self: self.read(HYBRIDEF_MODE_RESIDUALS))
    projections = property(lambda self: self.read(HYBRIDEF_PROJECTIONS))
    uphill_steps = property(lambda self: self.read(HYBRIDEF_UPHILL_STEPS))
    tangent_steps = property(lambda self: self.read(HYBRIDEF_TANGENT_STEPS))
    iteration_counts = property(lambda self: self.read(HYBRIDEF_ITERATION_COUNTS))
    products = property(lambda self: self.read(HYBRIDEF_PRODUCTS))
    evaluations = property(lambda self: self.read(HYBRIDEF_EVALUATIONS))


def find_saddles_hybrid(minima, n_particles, kick=0.05, grad_tol=1e-10, max_steps=300, max_step=0.1, zero_tol=1e-4, start_res_tol=1e-6,
                        seed=0, radial=RADIAL_LENNARD_JONES, **options):
    """Transition-state searches from the minima in ``minima`` (a DeviceArray, moved in place) without a dense Hessian, for up
    to 1024 particles: takes the lowest mode of every minimum (``lowest_modes`` to the loose relative residual
    ``start_res_tol``), displaces every point by ``kick`` along its vector, sets that vector as the first mode and runs a
    ``HybridModeFollowing`` (which takes ``options``) for at most ``max_steps`` steps.  Returns the handle:
    ``status == HYBRIDEF_CONVERGED`` with ``eigenvalues < -zero_tol`` marks the saddles found."""
    modes = lowest_modes(minima, n_particles, True, LOWMODE_MAX_KRYLOV, 40, start_res_tol, None, seed, radial)
    axpy_(float(kick), modes.vectors, minima)
    search = HybridModeFollowing(minima, n_particles, modes.vectors, max_step=max_step, zero_tol=zero_tol, grad_tol=grad_tol, seed=seed,
                                 radial=radial, **options)
    search.run(max_steps)
    return search


# ------------------------------------------------------------------------------ structure fingerprints, classification, pathways
STRUCTURE_MAX_PARTICLES = 1024
STRUCTURE_MAX_BATCH = 16384


def structure_fingerprints(points, n_particles, radial=RADIAL_LENNARD_JONES):
    """The fingerprint of every instance of ``points`` (``3 * n_particles * batch`` elements, instance b ``[x | y | z]``) in one
    launch (``dzo_structure_batch_fingerprint``, include/dzo.h): the per-particle energies sorted ascending, then the squared
    distances from the centroid sorted ascending.  It does not change under rotation, translation, reflection or a relabelling
    of the particles beyond rounding; it does not tell a structure from its mirror image.  Returns ``(fingerprints, energies)``:
    a DeviceArray ``(batch, 2 * n_particles)`` and the total energies (host array, the bits of
    ``pairwise_batch_energy_gradient``)."""
    n, batch = _batch_of(points, n_particles, least=1)
    fp = DeviceArray((batch, 2 * n), points.dtype)
    e = DeviceArray((batch,), points.dtype)
    _check(lib().dzo_structure_batch_fingerprint(radial, n, batch, _dt(points.dtype), points.ptr, fp.ptr, e.ptr))
    return fp, e.to_host()


def classify_structures(fingerprints, tol):
    """Greedy leader labels of the rows of ``fingerprints`` (a DeviceArray ``(batch, length)``) on the device
    (``dzo_structure_batch_classify``): rows a and b match iff ``|a_i - b_i| <= tol * max(1, |a_i|, |b_i|)`` for every i, in
    fp64; row k takes the label of the first representative before it that it matches, or becomes a representative with
    label k; a row with a non-finite element gets -1.  Returns ``(labels, representatives)``: host int32 ``(batch,)`` and the
    indices of the representatives, ascending.  Rows placed first keep their own labels as long as they are distinct: put
    known structures there to match against a database."""
    assert len(fingerprints.shape) == 2, "fingerprints must be a (batch, length) DeviceArray"
    batch, length = fingerprints.shape
    labels = DeviceArray((batch,), np.int32)
    count = C.c_int32(0)
    _check(lib().dzo_structure_batch_classify(length, batch, _dt(fingerprints.dtype), fingerprints.ptr, float(tol), labels.ptr, C.byref(count)))
    labels = labels.to_host()
    representatives = np.flatnonzero(labels == np.arange(batch))
    assert len(representatives) == count.value
    return labels, representatives


def unique_structures(points, n_particles, tol, radial=RADIAL_LENNARD_JONES):
    """The distinct structures among the instances of ``points``: ``structure_fingerprints`` then ``classify_structures``.
    Returns ``(labels, representatives, counts, energies)``: the label of every instance, the indices of the distinct
    structures, how many instances carry each of those labels, and the energies of the distinct structures.  ``tol`` has no
    default: see ``connect_saddles``."""
    fp, e = structure_fingerprints(points, n_particles, radial)
    labels, reps = classify_structures(fp, tol)
    counts = np.array([(labels == r).sum() for r in reps], dtype=np.int64)
    return labels, reps, counts, e[reps]


class Pathways:
    """What ``connect_saddles`` returns.  ``minima``: DeviceArray ``(n_minima, 3N)`` of the distinct end points, the known ones
    first; ``minimum_energies`` (host, ``(n_minima,)``); ``saddle_energies`` (host, ``(batch,)``); ``edges`` (host int32
    ``(batch, 2)``: the minimum below the saddle on the + and on the - side of its mode, -1 where that end was not stuck and at
    rest after ``max_steps`` or has a non-finite fingerprint); ``barriers`` (host ``(batch, 2)``: saddle energy minus minimum energy, NaN
    where the edge is -1); ``degenerate`` (host bool: both ends carry the same label); ``ends`` (DeviceArray ``(2 batch, 3N)``,
    the + ends then the - ends); ``end_stuck`` (host bool ``(2 batch,)``); ``labels`` (of ``[known_minima | ends]``)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def triples(self):
        """``[(minimum, saddle, minimum)]`` of the saddles with both ends identified."""
        return [(int(a), k, int(b)) for k, (a, b) in enumerate(self.edges) if a >= 0 and b >= 0]


def quench_to_rest(points, n_particles, history_length=10, initial_step_length=0.01, steps_per_launch=50, max_steps=2000,
                   radial=RADIAL_LENNARD_JONES):
    """Quenches ``points`` (moved in place) with ``BatchedLBFGS`` handles until the points are at rest.  ``is_stuck`` alone does
    not say that: the reference's L-BFGS has no curvature safeguard, and a pair (s, y) with s.y < 0, which is what a start next
    to a saddle gives, turns its direction uphill, so that the backtracking search halves the step to nothing and the
    instance is stuck on a slope (measured on LJ7: every end 0.02 from a saddle stuck with |g| = 0.2).  So when every instance
    is stuck a FRESH handle (empty history: its first step is the plain gradient step) takes over, and an instance is at rest
    when it is stuck and a fresh handle has not lowered its energy by a single bit.  At most ``max_steps`` steps are taken
    by any instance over all handles (a handle counts as one step at least).  Returns the host bool array "at rest"."""
    n, batch = _batch_of(points, n_particles)
    taken, before = 0, None
    at_rest = np.zeros(batch, dtype=bool)
    while taken < max_steps and not at_rest.all():
        opt = BatchedLBFGS(points, n, initial_step_length, history_length, radial)
        try:
            opt._run(max_steps - taken, steps_per_launch)
            energies, stuck = opt.current_objective_values, opt.is_stuck
            taken += max(1, int(opt.iteration_counts.max()))
        finally:
            opt.close()
        if before is not None:
            at_rest = stuck & (energies.view(np.int64 if energies.itemsize == 8 else np.int32)
                               == before.view(np.int64 if before.itemsize == 8 else np.int32))
        before = energies
    return at_rest


def connect_saddles(saddles, modes, n_particles, displacement, tol, known_minima=None, history_length=10, initial_step_length=0.01,
                    steps_per_launch=50, max_steps=2000, radial=RADIAL_LENNARD_JONES, descent_steps=0):
    """Which two minima every transition state joins.  ``saddles`` and ``modes`` are DeviceArrays of ``3 * n_particles * batch``
    elements (for instance the points and ``HYBRIDEF_MODES`` of ``find_saddles_hybrid``); neither is changed.  The 2 batch points
    ``saddle +- displacement * mode`` are formed on the device, quenched together by ``quench_to_rest`` (``BatchedLBFGS`` until
    every instance is stuck, again from a fresh handle until none moves any more, ``max_steps`` steps at most), and then ``[known_minima | ends]`` is fingerprinted and classified with ``tol``
    (``known_minima``: a DeviceArray of ``3 * n_particles * K`` elements, or None).  Returns a ``Pathways``.

    ``displacement`` and ``tol`` have no default: their right values depend on the element type and the system (the precedent
    is ``morse_index``'s ``zero_tol``).  ``tol`` must sit between the largest fingerprint distance of copies of one minimum
    (what the quench leaves, not rounding alone) and the smallest distance of two different minima; ``displacement`` must leave
    the saddle's flat top without jumping a neighbouring barrier.  Measured for 38 atoms (the ``structure-readme`` block of
    README.md, profiles/structure_bench.json): in fp64 copies of one minimum at rest are at most 9.2e-7 apart and two minima of
    different energy at least 2.0e-2, so anything from 1e-5 to 1e-3 serves; in fp32 the two figures are NOT a factor 100 apart
    (instances that energy and spectrum call one minimum are up to 1.2e-1 apart, minima of different energy as close as 8.1e-3),
    so no ``tol`` identifies fp32 minima of that size reliably: bring them to rest in fp64 first.  Of the displacements 1e-3 .. 1e-1, 3e-2 and 1e-1 gave every saddle two different ends in fp64.

    ``descent_steps`` > 0: before the L-BFGS quench every end first takes up to that many steps of ``BatchedAdGD`` (a plain
    gradient method with a step from the local curvature).  The minima a saddle joins are those its two steepest-descent paths
    end in; L-BFGS does not follow them, and from the shoulder of a saddle its long early steps can cross a low neighbouring
    barrier (seen on the 13-atom cluster: an end that steepest descent takes to the minimum at -40.3489 quenched into the
    icosahedron).  0, the default, is the quench alone."""
    n, batch = _batch_of(saddles, n_particles, "saddles", least=1)
    n3 = 3 * n
    assert modes.size == saddles.size and modes.dtype == saddles.dtype, "modes must be laid out like saddles"
    dtype, es = saddles.dtype, saddles.dtype.itemsize
    known = 0
    if known_minima is not None:
        known = known_minima.size // n3
        assert known_minima.size == n3 * known and known_minima.dtype == dtype, "known_minima must hold 3 * n_particles * K elements"
    both = DeviceArray((known + 2 * batch, n3), dtype)
    if known:
        _check(lib().dzo_memcpy_d2d(both.ptr, known_minima.ptr, known_minima.nbytes))
    ends = both.view(known * n3, (2 * batch, n3))
    for side, sign in enumerate((1.0, -1.0)):
        end = ends.view(side * batch * n3, (batch * n3,))
        _check(lib().dzo_memcpy_d2d(end.ptr, saddles.ptr, saddles.nbytes))
        axpy_(sign * float(displacement), modes, end)
    if descent_steps > 0:
        descent = BatchedAdGD(ends, n, initial_step_length, radial)
        try:
            taken, done = 0, False
            while not done and taken < int(descent_steps):
                k = min(int(steps_per_launch), int(descent_steps) - taken)
                done = descent.step(k)
                taken += k
        finally:
            descent.close()
    stuck = quench_to_rest(ends, n, history_length, initial_step_length, steps_per_launch, max_steps, radial)
    fp, energies = structure_fingerprints(both, n, radial)
    for k in np.flatnonzero(~stuck):                         # an end that is still moving names no minimum
        fill_(fp.view((known + int(k)) * 2 * n, (1,)), float("nan"))
    labels, reps = classify_structures(fp, tol)
    position = {int(r): i for i, r in enumerate(reps)}
    minima = DeviceArray((len(reps), n3), dtype)
    for i, r in enumerate(reps):
        _check(lib().dzo_memcpy_d2d(minima.ptr + i * n3 * es, both.ptr + int(r) * n3 * es, n3 * es))
    minimum_energies = energies[reps]
    saddle_energies = pairwise_batch_energy_gradient(saddles, n, radial=radial)
    edges = np.array([[position.get(int(labels[known + side * batch + b]), -1) for side in range(2)] for b in range(batch)],
                     dtype=np.int32).reshape(batch, 2)
    barriers = np.full((batch, 2), np.nan, dtype=dtype)
    ok = edges >= 0
    if ok.any():
        barriers[ok] = (saddle_energies[:, None] - minimum_energies[np.where(ok, edges, 0)])[ok]
    degenerate = ok[:, 0] & (edges[:, 0] == edges[:, 1])
    return Pathways(minima=minima, minimum_energies=minimum_energies, saddle_energies=saddle_energies, edges=edges, barriers=barriers,
                    degenerate=degenerate, ends=ends, end_stuck=stuck, labels=labels, n_known=known, _both=both)


# ------------------------------------------------------------------------------ batched nudged elastic band
NEB_MAX_PARTICLES = 1024
NEB_MAX_IMAGES = 32
NEB_ACTIVE, NEB_CONVERGED, NEB_FAILED = 0, 1, 2
NEB_SHAPE_WAVE, NEB_SHAPE_BLOCK = 0, 1
NEB_STORAGE_LDS, NEB_STORAGE_MEMORY = 0, 1
(NEB_BAND, NEB_VELOCITIES, NEB_FORCES, NEB_TANGENTS, NEB_ENERGIES, NEB_FORCE_RMS, NEB_RESIDUALS, NEB_CLIMBING_IMAGES, NEB_HIGHEST_IMAGES,
 NEB_STATUS, NEB_ITERATION_COUNTS) = range(11)


def neb_plan(n_particles, n_images, dtype):
    """``(shape, storage, lds_bytes)`` of ``dzo_neb_plan``: the launch shape that serves a band of ``n_images`` images of
    ``n_particles`` particles, where its points, velocities and forces live during a launch, and the dynamic LDS of the launch.
    A pure function; needs no device."""
    shape, storage, lds = C.c_int32(), C.c_int32(), C.c_int64()
    _check(lib().dzo_neb_plan(int(n_particles), int(n_images), _dt(dtype), C.byref(shape), C.byref(storage), C.byref(lds)))
    return shape.value, storage.value, lds.value


def _bands_of(band, n_particles, n_images):
    """``(n, M, batch)`` of a band array of ``3 * n_particles * n_images * batch`` elements."""
    n, m = int(n_particles), int(n_images)
    batch = band.size // (3 * n * m) if n > 0 and m > 0 else 0
    assert band.size == 3 * n * m * batch and batch >= 1, "band must hold 3 * n_particles * n_images * batch elements"
    return n, m, batch


def interpolate_band(a, b, n_particles, n_images, band=None):
    """``dzo_neb_batch_interpolate``: the straight bands of ``n_images`` images between the points ``a`` and ``b`` (DeviceArrays
    of ``3 * n_particles * batch`` elements in a common frame).  Returns the band, a DeviceArray ``(batch, n_images, 3N)``
    (``band`` when given): images 0 and ``n_images - 1`` are copies of ``a`` and ``b``."""
    n, batch = _batch_of(a, n_particles, "a", least=1)
    assert b.size == a.size and b.dtype == a.dtype, "a and b must be laid out alike"
    if band is None:
        band = DeviceArray((batch, int(n_images), 3 * n), a.dtype)
    assert band.size == a.size * int(n_images) and band.dtype == a.dtype
    _check(lib().dzo_neb_batch_interpolate(n, int(n_images), batch, _dt(a.dtype), a.ptr, b.ptr, band.ptr))
    return band


def neb_apply(band, velocities, n_particles, n_images, spring=1.0, dt=0.02, max_move=0.1, force_tol=0.0, climb=True,
              radial=RADIAL_LENNARD_JONES):
    """``dzo_neb_batch_apply``: ONE iteration of the nudged elastic band (include/dzo.h) of every band, from the band and the
    velocities given (DeviceArrays of ``3 * n_particles * n_images * batch`` elements, both moved in place); ``climb``: the
    highest interior image climbs.  Returns a dict of host arrays: ``energies`` and ``force_rms`` ``(batch, M)``;
    ``gradients``, ``forces`` and ``tangents`` ``(batch, M, 3N)``; ``residuals``, ``climbing_images``, ``highest_images`` and
    ``status`` ``(batch,)``."""
    n, m, batch = _bands_of(band, n_particles, n_images)
    assert velocities.size == band.size and velocities.dtype == band.dtype, "velocities must be laid out like the band"
    t = band.dtype
    e, frms = DeviceArray((batch, m), t), DeviceArray((batch, m), np.float64)
    g, f, tau = (DeviceArray((batch, m, 3 * n), t) for _ in range(3))
    res = DeviceArray(batch, np.float64)
    ci, hi, st = (DeviceArray(batch, np.int32) for _ in range(3))
    _check(lib().dzo_neb_batch_apply(radial, n, m, batch, _dt(t), band.ptr, velocities.ptr, float(spring), float(dt), float(max_move),
                                     float(force_tol), int(bool(climb)), e.ptr, g.ptr, f.ptr, tau.ptr, frms.ptr, res.ptr, ci.ptr, hi.ptr, st.ptr))
    return dict(energies=e.to_host(), gradients=g.to_host(), forces=f.to_host(), tangents=tau.to_host(), force_rms=frms.to_host(),
                residuals=res.to_host(), climbing_images=ci.to_host(), highest_images=hi.to_host(), status=st.to_host())


class ElasticBand(_SteppedCluster):
    """The nudged elastic band with a climbing image (Henkelman & Jonsson 2000; include/dzo.h states the iteration) of many
    pairs of Lennard-Jones minima at once, up to 1024 particles and 32 images.  ``band`` is a DeviceArray of
    ``3 * n_particles * n_images * batch`` elements (image m of band b ``[x | y | z]`` at ``3 * n_particles * (n_images * b + m)``,
    for instance from ``interpolate_band``), aliased and moved; images 0 and ``n_images - 1`` are the fixed ends.  ``step(k)``
    enqueues ONE launch that iterates every ACTIVE band k times: improved tangents, the spring force along the band, projected
    velocity Verlet with time step ``dt`` and moves capped at ``max_move``, and from iteration ``climb_after`` on (``climb``) a
    climbing image.  A band ends CONVERGED (the largest force rms of its images ``<= force_tol``) or FAILED and is then left
    alone.  ``force_tol`` has no default: what a band can reach depends on the element type and the system (on 7-atom bands of
    five images 1e-6 in float64 and 1e-5 in float32, tests/test_gpu_neb.py; the ``neb-readme`` block of README.md has how many
    38-atom bands reach 1e-6 and 1e-4)."""
    _prefix = "dzo_neb_batch_"

    def __init__(self, band, n_particles, n_images, spring=1.0, dt=0.02, max_move=0.1, *, force_tol, climb=True, climb_after=50,
                 radial=RADIAL_LENNARD_JONES):
        _need_init()
        self.points = self.band = band
        self.dtype = band.dtype
        self.n_particles, self.n_images, self.batch = _bands_of(band, n_particles, n_images)
        h = C.c_void_p()
        self._call("create", radial, self.n_particles, self.n_images, self.batch, _dt(self.dtype), band.ptr, float(spring), float(dt),
                   float(max_move), float(force_tol), int(bool(climb)), int(climb_after), C.byref(h))
        self.h = h

    def run(self, max_iterations, steps_per_call=100):
        """Iterates until no band is ACTIVE, at most ``max_iterations`` per band.  Returns the iterations enqueued."""
        return self._run(max_iterations, steps_per_call)

    def _shape(self, what):
        b, m, n3 = self.batch, self.n_images, 3 * self.n_particles
        vec, per, i32 = ((b, m, n3), self.dtype), ((b, m), self.dtype), ((b,), np.int32)
        return {NEB_BAND: vec, NEB_VELOCITIES: vec, NEB_FORCES: vec, NEB_TANGENTS: vec, NEB_ENERGIES: per, NEB_FORCE_RMS: ((b, m), np.float64),
                NEB_RESIDUALS: ((b,), np.float64), NEB_CLIMBING_IMAGES: i32, NEB_HIGHEST_IMAGES: i32, NEB_STATUS: i32,
                NEB_ITERATION_COUNTS: ((b,), np.int64)}[what]

    images = property(lambda self: self.read(NEB_BAND))
    velocities = property(lambda self: self.read(NEB_VELOCITIES))
    forces = property(lambda self: self.read(NEB_FORCES))
    tangents = property(lambda self: self.read(NEB_TANGENTS))
    energies = property(lambda self: self.read(NEB_ENERGIES))
    force_rms = property(lambda self: self.read(NEB_FORCE_RMS))
    residuals = property(lambda self: self.read(NEB_RESIDUALS))
    climbing_images = property(lambda self: self.read(NEB_CLIMBING_IMAGES))
    highest_images = property(lambda self: self.read(NEB_HIGHEST_IMAGES))
    status = property(lambda self: self.read(NEB_STATUS))
    iteration_counts = property(lambda self: self.read(NEB_ITERATION_COUNTS))


class BandConnections:
    """What ``connect_minima`` returns.  ``band``: DeviceArray ``(batch, M, 3N)`` of the relaxed bands; ``energies`` (host,
    ``(batch, M)``: the profile of every band); ``status``, ``climbing_images``, ``iteration_counts`` and ``residuals`` (host,
    ``(batch,)``); ``converged`` (host indices of the CONVERGED bands); ``saddles`` (DeviceArray ``(len(converged), 3N)``: their
    climbing images after the refinement), ``saddle_energies``, ``saddle_status`` (``HYBRIDEF_*``), ``saddle_eigenvalues`` and
    ``saddle_grms`` (host, per converged band); ``barriers`` (host ``(batch, 2)``: refined saddle energy minus the energy of
    image 0 and of image M - 1, NaN for a band that did not converge); ``alignment`` (the ``Alignment`` of the end pairs, only
    when ``connect_minima`` was asked to align them)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def connect_minima(a, b, n_particles, n_images, force_tol, grad_tol=1e-10, max_iterations=10000, steps_per_call=100, refine_steps=100,
                   radial=RADIAL_LENNARD_JONES, align=False, **band_options):
    """The double-ended search: what joins minimum ``a[k]`` to minimum ``b[k]``, and how high is the barrier.  ``a`` and ``b``
    are DeviceArrays of ``3 * n_particles * batch`` elements in a common frame (no alignment is done: the two ``ends`` of one
    saddle in ``connect_saddles`` are in one); neither is changed.  ``align=True``, or a dict of ``align_pairs`` options, brings
    arbitrary pairs into one first: ``b`` is replaced by ``align_pairs(a, b, n_particles, **options).aligned`` and the result
    carries the ``Alignment`` as ``alignment``; with the default nothing of that happens.  Interpolates (``interpolate_band``),
    relaxes the bands (``ElasticBand`` with ``band_options``: spring, dt, max_move, climb_after) to ``force_tol`` in at most ``max_iterations``
    iterations, then takes the climbing image and its tangent of every CONVERGED band and refines them with
    ``HybridModeFollowing(directions=tangent)`` to ``grad_tol`` in at most ``refine_steps`` steps.  Returns a
    ``BandConnections``.  ``force_tol`` has no default, like ``tol`` in ``connect_saddles``: it depends on the element type."""
    n, batch = _batch_of(a, n_particles, "a", least=1)
    m, n3, es = int(n_images), 3 * n, a.dtype.itemsize
    extra = {}
    if align is not False and align is not None:
        extra["alignment"] = align_pairs(a, b, n, **(align if isinstance(align, dict) else {}))
        b = extra["alignment"].aligned
    band = interpolate_band(a, b, n, m)
    neb = ElasticBand(band, n, m, force_tol=force_tol, radial=radial, **band_options)
    try:
        neb.run(max_iterations, steps_per_call)
        energies, status, climbing = neb.energies, neb.status, neb.climbing_images
        counts, residuals = neb.iteration_counts, neb.residuals
        converged = np.flatnonzero((status == NEB_CONVERGED) & (climbing >= 0))
        k = len(converged)
        saddles, tangents = DeviceArray((k, n3), a.dtype), DeviceArray((k, n3), a.dtype)
        # two small copies per converged band from the host: fine for the hundreds of bands of one call
        for i, bi in enumerate(converged):
            offset = ((int(bi) * m + int(climbing[bi])) * n3) * es
            _check(lib().dzo_memcpy_d2d(saddles.ptr + i * n3 * es, band.ptr + offset, n3 * es))
            _check(lib().dzo_memcpy_d2d(tangents.ptr + i * n3 * es, neb.ptr(NEB_TANGENTS) + offset, n3 * es))
    finally:
        neb.close()
    barriers = np.full((batch, 2), np.nan, dtype=a.dtype)
    fields = dict(saddle_energies=np.empty(0, a.dtype), saddle_status=np.empty(0, np.int32), saddle_eigenvalues=np.empty(0, a.dtype),
                  saddle_grms=np.empty(0, np.float64))
    if k:
        search = HybridModeFollowing(saddles, n, tangents, grad_tol=grad_tol, radial=radial)
        try:
            search.run(refine_steps)
            fields = dict(saddle_energies=search.energies, saddle_status=search.status, saddle_eigenvalues=search.eigenvalues,
                          saddle_grms=search.grms)
        finally:
            search.close()
        barriers[converged] = fields["saddle_energies"][:, None] - energies[converged][:, [0, m - 1]]
    return BandConnections(band=band, energies=energies, status=status, climbing_images=climbing, iteration_counts=counts, residuals=residuals,
                           converged=converged, saddles=saddles, barriers=barriers, **fields, **extra)


# ------------------------------------------------------------------------------ rigid and permutational alignment of pairs
ALIGN_MAX_PARTICLES = 1024
ALIGN_MAX_RANDOM_TRIALS = 64
ALIGN_MAX_CYCLES = 64
ALIGN_TRIAL_IDENTITY, ALIGN_TRIAL_PRINCIPAL = 1, 2
ALIGN_CONVERGED, ALIGN_CYCLE_LIMIT, ALIGN_FAILED = 0, 1, 2


def _pair_of(a, b, n_particles):
    """``(n, batch)`` of two arrays of ``3 * n_particles * batch`` elements of one element type."""
    n, batch = _batch_of(a, n_particles, "a", least=1)
    _batch_of(b, n_particles, "b", batch=batch)
    assert b.dtype == a.dtype, "a and b must have one element type"
    return n, batch


def assign_particles(a, b, n_particles):
    """``dzo_align_batch_assign``: for every pair of points ``a[k]``, ``b[k]`` (DeviceArrays of ``3 * n_particles * batch``
    elements, ``[x | y | z]``; neither is changed) the permutation p that minimises ``sum_i |a_i - b_p(i)|^2`` in the frames
    given, by the shortest augmenting path in fp64 on the device.  Returns ``(perm, cost)``: host int32 ``(batch, N)`` and
    host float64 ``(batch,)``.  A pair with a non-finite coordinate gets the identity and NaN."""
    n, batch = _pair_of(a, b, n_particles)
    perm, cost = DeviceArray((batch, n), np.int32), DeviceArray((batch,), np.float64)
    _check(lib().dzo_align_batch_assign(n, batch, _dt(a.dtype), a.ptr, b.ptr, perm.ptr, cost.ptr))
    return perm.to_host(), cost.to_host()


class Alignment:
    """What ``align_pairs`` returns.  ``aligned``: DeviceArray ``(batch, 3N)``, ``b`` in ``a``'s frame with ``a``'s labels;
    ``permutations`` (host int32 ``(batch, N)``: particle i of ``a`` is particle ``p[i]`` of ``b``); ``rotations`` (host float64
    ``(batch, 3, 3)``, the inversion folded in: det = +-1); ``distances`` (host float64 ``(batch,)``); ``best_trials``,
    ``cycles`` and ``status`` (host int32 ``(batch,)``, ``ALIGN_CONVERGED`` / ``ALIGN_CYCLE_LIMIT`` / ``ALIGN_FAILED``, of the
    winning start); ``trial_distances`` (host float64 ``(batch, n_starts)`` when asked for, else None)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def align_pairs(a, b, n_particles, trials=ALIGN_TRIAL_IDENTITY | ALIGN_TRIAL_PRINCIPAL, random_trials=8, max_cycles=20,
                allow_inversion=False, seed=0, want_trials=False):
    """``dzo_align_batch_pairs`` (include/dzo.h states the rule): brings every ``b[k]`` onto ``a[k]`` by a translation, a
    rotation, a relabelling of its identical particles and, with ``allow_inversion``, an inversion, so that
    ``sum_i |a_i - x'_i|^2`` is small.  From every start (the identity, the four principal-axis rotations, ``random_trials``
    random ones from the stream ``seed``; all of them once more inverted) it alternates the optimal assignment with the best
    rotation until the permutation repeats, ``max_cycles`` cycles at most, and keeps the best start.  ``a`` and ``b`` are
    DeviceArrays of ``3 * n_particles * batch`` elements; neither is changed.  A multi-start local method: the distance is an
    upper bound of the true one (the ``align-readme`` block of README.md has what it finds).  Returns an ``Alignment``."""
    n, batch = _pair_of(a, b, n_particles)
    n_orient = (int(trials) & 1) + 4 * ((int(trials) >> 1) & 1) + int(random_trials)
    n_starts = (2 if allow_inversion else 1) * n_orient
    aligned = DeviceArray((batch, 3 * n), a.dtype)
    perm, rot, dist = DeviceArray((batch, n), np.int32), DeviceArray((batch, 3, 3), np.float64), DeviceArray((batch,), np.float64)
    best, cycles, status = (DeviceArray((batch,), np.int32) for _ in range(3))
    per_trial = DeviceArray((batch, max(n_starts, 1)), np.float64) if want_trials else None
    _check(lib().dzo_align_batch_pairs(n, batch, _dt(a.dtype), a.ptr, b.ptr, int(trials), int(random_trials), int(max_cycles),
                                       int(bool(allow_inversion)), _u64(seed), aligned.ptr, perm.ptr, rot.ptr, dist.ptr, best.ptr,
                                       cycles.ptr, status.ptr, per_trial.ptr if want_trials else None))
    return Alignment(aligned=aligned, permutations=perm.to_host(), rotations=rot.to_host(), distances=dist.to_host(),
                     best_trials=best.to_host(), cycles=cycles.to_host(), status=status.to_host(),
                     trial_distances=per_trial.to_host() if want_trials else None)


# ------------------------------------------------------------------------------ multi-step pathways: candidates, graph, connect cycle
PATHWAY_MAX_PARTICLES = 1024
PATHWAY_MAX_IMAGES = 32
PATHWAY_MAX_BATCH = 1048576
PATHWAY_OVERFLOW = 7


class BandCandidates:
    """What ``band_candidates`` returns.  ``count``; ``points`` and ``tangents`` (DeviceArrays ``(count, 3N)``: the candidate
    images and the band's unit tangents there); ``energies`` (host ``(count,)``); ``band_index`` and ``image_index`` (host
    int32 ``(count,)``); ``offsets`` (host int32 ``(batch + 1,)``: the candidates of band b are
    ``offsets[b] .. offsets[b + 1] - 1``); ``band_energies`` (host ``(batch, M)``: the profiles the candidates were taken from)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def band_candidates(band, n_particles, n_images, energies=None, radial=RADIAL_LENNARD_JONES):
    """``dzo_pathway_batch_candidates`` (include/dzo.h states the rule): the transition-state candidates of every band of
    ``band`` (a DeviceArray of ``3 * n_particles * n_images * batch`` elements, the layout of ``ElasticBand``; not changed).
    Interior image m is a candidate iff ``E[m] > E[m - 1]`` and ``E[m] >= E[m + 1]``; a band need not have converged, or be
    ACTIVE, to have some.  ``energies``: a DeviceArray ``(batch, n_images)`` of the band's element type (for instance an
    ``ElasticBand``'s record); None evaluates the band as it stands as ``n_images * batch`` points with
    ``pairwise_batch_energy_gradient``'s routine, and only that path takes ``radial``.  Returns a ``BandCandidates``,
    compacted band-major with the image index ascending inside a band; a tangent is bit for bit the one ``neb_apply`` records
    for that image of that band."""
    n, m, batch = _bands_of(band, n_particles, n_images)
    t = band.dtype
    if energies is None:
        energies = DeviceArray((batch, m), t)
        _check(lib().dzo_pairwise_batch_energy_gradient(radial, n, batch * m, _dt(t), band.ptr, energies.ptr, None))
    assert energies.size == batch * m and energies.dtype == t, "energies must hold n_images * batch elements of the band's type"
    capacity = batch * ((m - 1) // 2)                        # the most the bands can hold
    points, tangents = DeviceArray((capacity, 3 * n), t), DeviceArray((capacity, 3 * n), t)
    e = DeviceArray((capacity,), t)
    bi, ii = DeviceArray((capacity,), np.int32), DeviceArray((capacity,), np.int32)
    offsets = DeviceArray((batch + 1,), np.int32)
    count = C.c_int64(0)
    _check(lib().dzo_pathway_batch_candidates(n, m, batch, _dt(t), band.ptr, energies.ptr, capacity, points.ptr, tangents.ptr, e.ptr,
                                              bi.ptr, ii.ptr, offsets.ptr, C.byref(count)))
    k = int(count.value)
    return BandCandidates(count=k, points=points.view(0, (k, 3 * n)), tangents=tangents.view(0, (k, 3 * n)),
                          energies=e.to_host()[:k], band_index=bi.to_host()[:k], image_index=ii.to_host()[:k],
                          offsets=offsets.to_host(), band_energies=energies.to_host().reshape(batch, m), _owners=(points, tangents))


class PathwayGraph:
    """The database side of the connect cycle (Carr, Trygubenko & Wales 2005), on the host: minima and saddles by index and
    energy, edges ``(minimum, saddle, minimum)``, a cache of pair distances and a count of the bands tried per pair.  Holds no
    coordinates and needs no device.  ``max_attempts``: after that many bands between one pair of minima the pair is not
    proposed again."""

    def __init__(self, max_attempts=2):
        self.max_attempts = int(max_attempts)
        self.minimum_energies, self.saddle_energies, self.edges = [], [], []
        # (n_minima, n_minima) tables, grown by doubling: the cached distances (inf: none), the bands tried, "a saddle joins them"
        self._d, self._tries, self._joined = np.full((0, 0), np.inf), np.zeros((0, 0), np.int64), np.zeros((0, 0), bool)
        self._weights = None                                 # the table next_attempts searches, until the next change

    n_minima = property(lambda self: len(self.minimum_energies))
    n_saddles = property(lambda self: len(self.saddle_energies))

    @staticmethod
    def _key(i, j):
        return (int(i), int(j)) if i <= j else (int(j), int(i))

    def add_minimum(self, energy):
        """Returns the index of the new minimum."""
        self.minimum_energies.append(float(energy))
        k, room = len(self.minimum_energies), len(self._d)
        if k > room:
            grown = max(2 * room, 16)
            for name, fill in (("_d", np.inf), ("_tries", 0), ("_joined", False)):
                old = getattr(self, name)
                new = np.full((grown, grown), fill, dtype=old.dtype)
                new[:room, :room] = old
                setattr(self, name, new)
        self._d[k - 1, k - 1] = 0.0
        self._weights = None
        return k - 1

    def add_saddle(self, energy, i, j):
        """A saddle of ``energy`` that joins minima i and j (i != j).  Returns its index."""
        assert 0 <= i < self.n_minima and 0 <= j < self.n_minima and i != j, (i, j)
        self.saddle_energies.append(float(energy))
        self.edges.append((int(i), len(self.saddle_energies) - 1, int(j)))
        self._joined[i, j] = self._joined[j, i] = True
        self._weights = None
        return len(self.saddle_energies) - 1

    def set_distance(self, i, j, d):
        """Caches the distance of minima i and j; arrays set many pairs at once."""
        self._d[i, j] = self._d[j, i] = d
        self._weights = None

    def distance(self, i, j):
        """The cached distance of minima i and j; inf where none was set."""
        return float(self._d[i, j])

    def note_attempt(self, i, j):
        self._tries[i, j] += 1
        if i != j:
            self._tries[j, i] += 1
        self._weights = None

    def attempts(self, i, j):
        return int(self._tries[i, j])

    def _neighbours(self):
        out = [[] for _ in range(self.n_minima)]
        for i, s, j in self.edges:
            out[i].append((j, s))
            out[j].append((i, s))
        return out

    def connected(self, i, j):
        """Whether a chain of saddles joins minima i and j."""
        component = self.components()
        return bool(component[i] == component[j])

    def components(self):
        """The label of every minimum's connected component (the lowest index in it), as an int array."""
        n = self.n_minima
        label = np.arange(n)
        for i, _, j in self.edges:                           # union by the lower root, paths halved on the way
            while label[i] != i:
                label[i] = label[label[i]]
                i = label[i]
            while label[j] != j:
                label[j] = label[label[j]]
                j = label[j]
            label[max(i, j)] = min(i, j)
        for k in range(n):
            label[k] = label[label[k]]                       # roots have lower indices: one ascending pass flattens
        return label

    def best_path(self, i, j):
        """The path from i to j whose highest saddle is lowest, among those the one with the fewest steps:
        ``[i, saddle, minimum, ..., saddle, j]`` (``[i]`` for i == j), or None when nothing joins them."""
        import heapq
        i, j = int(i), int(j)
        nb = self._neighbours()
        # the minimax value: the lowest "highest saddle" of any way from i to j
        best, heap = {i: -float("inf")}, [(-float("inf"), i)]
        while heap:
            top, u = heapq.heappop(heap)
            if top != best[u]:
                continue
            if u == j:
                break
            for v, s in nb[u]:
                cand = max(top, self.saddle_energies[s])
                if v not in best or cand < best[v]:
                    best[v] = cand
                    heapq.heappush(heap, (cand, v))
        if j not in best:
            return None
        # ... and the fewest steps over the saddles at or below it, breadth first; of several saddles between two minima the lowest
        limit, back, front = best[j], {i: None}, [i]
        while front and j not in back:
            reached = []
            for u in front:
                for v, s in sorted(nb[u], key=lambda e: (self.saddle_energies[e[1]], e[1])):
                    if v not in back and self.saddle_energies[s] <= limit:
                        back[v] = (u, s)
                        reached.append(v)
            front = reached
        path, u = [j], j
        while u != i:
            u, s = back[u]
            path += [s, u]
        return path[::-1]

    def next_attempts(self, i, j):
        """The bands to try next for the pair (i, j): Dijkstra from i to j over ALL minima with the weight 0 for a pair a
        saddle joins, the squared cached distance otherwise, and infinity for a pair without a cached distance or tried
        ``max_attempts`` times; returns the pairs ``(p, q)`` of non-zero weight on that path, in path order.  Empty when i and
        j are connected already, and when every way across is used up."""
        n, i, j = self.n_minima, int(i), int(j)
        joined = self._joined[:n, :n]
        if self._weights is None:
            d = self._d[:n, :n]
            self._weights = np.where(joined, 0.0, np.where(self._tries[:n, :n] >= self.max_attempts, np.inf, d * d))
        w = self._weights
        dist, back, done = np.full(n, np.inf), np.full(n, -1), np.zeros(n, bool)
        dist[i] = 0.0
        for _ in range(n):                                   # dense Dijkstra: the graph is complete
            u = int(np.argmin(np.where(done, np.inf, dist)))
            if done[u] or dist[u] == np.inf or u == j:
                break
            done[u] = True
            through = dist[u] + w[u]
            better = (through < dist) & ~done
            dist[better], back[better] = through[better], u
        if dist[j] == np.inf:
            return []
        hops, u = [], j
        while u != i:
            hops.append((int(back[u]), u))
            u = int(back[u])
        return [(p, q) for p, q in hops[::-1] if not joined[p, q]]


class PathwayConnections:
    """What ``connect_pathways`` returns.  ``graph`` (the ``PathwayGraph``); ``minima`` and ``saddles`` (DeviceArrays
    ``(n_minima, 3N)`` and ``(n_saddles, 3N)``, rows by graph index), ``saddle_modes`` (DeviceArray like ``saddles``: the
    downhill direction at every saddle), ``minimum_energies`` and ``saddle_energies`` (host); ``pairs`` (host int ``(P, 2)``:
    the graph indices of the ends of every pair; identical ends share a node); per pair ``connected`` (bool), ``paths``
    (``PathwayGraph.best_path`` or None), ``barriers`` (the highest saddle on the path minus the energy of the pair's first
    end; NaN where not connected, 0 for a pair of identical ends), ``cycles_used`` (the cycle after which the pair was first
    connected; the cycles run otherwise) and ``attempts_used`` (the bands proposed for the pair over all cycles, a band it shares with another pair counted for both); ``cycles`` (one dict per cycle:
    ``bands``, ``candidates``, ``refined``, ``new_saddles``, ``new_minima``, ``duplicates``, ``degenerate``, ``unresolved``,
    ``connected`` (pairs, after the cycle), ``minima`` and ``saddles`` (the database's size after it) and ``seconds``, the
    cycle's time by phase: distances, search (the graph), align, band, candidates, refine, connect)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _rows(host, index, dtype):
    """The rows ``index`` of the host array as a DeviceArray."""
    return DeviceArray.from_host(np.ascontiguousarray(host[np.asarray(index, dtype=np.int64)], dtype=dtype))


def connect_pathways(a, b, n_particles, n_images, *, tol, displacement, band_iterations=600, max_cycles=10, max_attempts=2,
                     grad_tol=1e-10, zero_tol=1e-4, refine_steps=300, verify_index=True, steps_per_call=100, align=None,
                     band_options=None, refine_options=None, quench_options=None, radial=RADIAL_LENNARD_JONES):
    """The connect cycle (Carr, Trygubenko & Wales 2005): which transition states and intermediate minima join minimum ``a[k]``
    to minimum ``b[k]``, for pairs that may be several elementary steps apart.  ``a`` and ``b`` are DeviceArrays of
    ``3 * n_particles * P`` elements, in any frames and labellings; neither is changed.  All ends enter one database by
    ``classify_structures`` with ``tol``, so identical ends share a node.  A cycle: (1) ``PathwayGraph.next_attempts`` of every
    pair that is not connected yet, duplicates removed; before that (2) the aligned distances of every new database member to
    all members by ONE ``align_pairs`` call (``align``: its options; ``seed`` is the cycle's number less one unless given;
    with K members of which k are new that is about k K pairs, gathered on the host and uploaded, ``2 * 3N`` elements each, and the search
    of (1) is a dense Dijkstra of K^2 operations per pair: both grow quadratically with the database, and from the second cycle on
    they are most of a cycle's time on the 38-atom workload of the ``pathways-readme`` block of README.md); (3) the attempts are aligned and interpolated
    (``n_images`` images); (4) one ``ElasticBand`` (``band_options``; ``force_tol`` 0 unless given there) runs
    ``band_iterations`` iterations, whatever its status; (5) ``band_candidates`` of the bands as they stand, FAILED ones
    included; (6) ``HybridModeFollowing(directions=tangents)`` (``grad_tol``, ``zero_tol``, ``refine_options``) for at most
    ``refine_steps`` steps; (7) the CONVERGED instances with ``eigenvalues < -zero_tol`` are kept, and for
    ``n_particles <= 128`` only those with exactly one eigenvalue of ``hessian_spectrum`` below ``-zero_tol`` unless
    ``verify_index=False`` (above 128 particles the index is NOT checked: a kept point may be a saddle of higher index);
    (8) ``connect_saddles(..., known_minima=database)`` (``displacement``, ``tol``, ``quench_options``; ``descent_steps`` is 2000 unless
    given there, so that an end is taken down its gradient before L-BFGS finishes it); (9) new minima and
    saddles are appended, a saddle that matches an earlier one in fingerprint and edge is dropped as a duplicate, a saddle
    with the same minimum on both sides or an end that did not come to rest is dropped and counted.  The cycle ends when every
    pair is connected, after ``max_cycles`` cycles, or when no pair has an attempt left.  ``tol`` and ``displacement`` have no
    default: see ``connect_saddles``.  Returns a ``PathwayConnections``."""
    import time
    n, pairs_n = _pair_of(a, b, n_particles)
    m, n3, dtype = int(n_images), 3 * n, a.dtype
    band_opts = dict(force_tol=0.0)
    band_opts.update(band_options or {})
    quench_opts = dict(descent_steps=2000)                   # the ends go down the gradient first: see connect_saddles
    quench_opts.update(quench_options or {})
    ends_host = np.concatenate([a.to_host().reshape(pairs_n, n3), b.to_host().reshape(pairs_n, n3)])
    fp, end_energies = structure_fingerprints(DeviceArray.from_host(ends_host), n, radial)
    labels, reps = classify_structures(fp, tol)
    assert np.all(labels >= 0), "an end has a non-finite fingerprint"
    node = {int(r): k for k, r in enumerate(reps)}
    graph = PathwayGraph(max_attempts)
    for r in reps:
        graph.add_minimum(end_energies[r])
    minima_host = ends_host[reps].copy()
    pairs = np.array([[node[int(labels[k])], node[int(labels[pairs_n + k])]] for k in range(pairs_n)], dtype=np.int64).reshape(pairs_n, 2)
    saddles_host, modes_host = np.empty((0, n3), dtype), np.empty((0, n3), dtype)
    have_distances = 0                                       # members whose distances to all earlier members are cached
    cycles_used, attempts_used = np.zeros(pairs_n, np.int64), np.zeros(pairs_n, np.int64)

    def is_connected():
        component = graph.components()
        return component[pairs[:, 0]] == component[pairs[:, 1]]

    connected, cycles = is_connected(), []
    for cycle in range(1, int(max_cycles) + 1):
        if connected.all():
            break
        clock, seconds = time.perf_counter(), {}

        def lap(name):
            nonlocal clock
            synchronize()
            now = time.perf_counter()
            seconds[name] = seconds.get(name, 0.0) + now - clock
            clock = now

        # the random starts of this cycle's alignments: a second attempt at a pair is not a copy of the first
        align_opts = dict(seed=cycle - 1)
        align_opts.update(align or {})
        # 2. distances of the new members to all members
        k_all = graph.n_minima
        q_new = np.repeat(np.arange(have_distances, k_all), np.arange(have_distances, k_all))
        p_all = np.concatenate([np.arange(q) for q in range(have_distances, k_all)] + [np.empty(0, np.int64)]).astype(np.int64)
        if len(q_new):
            graph.set_distance(p_all, q_new, align_pairs(_rows(minima_host, p_all, dtype), _rows(minima_host, q_new, dtype), n, **align_opts).distances)
        have_distances = k_all
        lap("distances")
        # 1. this cycle's bands
        attempts, seen = [], set()
        for k in np.flatnonzero(~connected):
            for p, q in graph.next_attempts(*pairs[k]):
                attempts_used[k] += 1
                if graph._key(p, q) not in seen:
                    seen.add(graph._key(p, q))
                    attempts.append((p, q))
        lap("search")
        if not attempts:
            break
        for p, q in attempts:
            graph.note_attempt(p, q)
        cycles_used[~connected] = cycle
        # 3, 4. align, interpolate, relax
        ends_a = _rows(minima_host, [p for p, _ in attempts], dtype)
        aligned = align_pairs(ends_a, _rows(minima_host, [q for _, q in attempts], dtype), n, **align_opts).aligned
        band = interpolate_band(ends_a, aligned, n, m)
        lap("align")
        neb = ElasticBand(band, n, m, radial=radial, **band_opts)
        try:
            neb.run(int(band_iterations), steps_per_call)
        finally:
            neb.close()
        lap("band")
        # 5 .. 7. candidates, refinement, the saddles among them
        cand = band_candidates(band, n, m, radial=radial)
        lap("candidates")
        stats = dict(bands=len(attempts), candidates=cand.count, refined=0, new_saddles=0, new_minima=0, duplicates=0, degenerate=0, unresolved=0)
        kept_points = kept_modes = None
        if cand.count:
            search = HybridModeFollowing(cand.points, n, cand.tangents, zero_tol=zero_tol, grad_tol=grad_tol, radial=radial, **(refine_options or {}))
            try:
                search.run(int(refine_steps))
                keep = np.flatnonzero((search.status == HYBRIDEF_CONVERGED) & (search.eigenvalues < -float(zero_tol)))
                kept_points, kept_modes = search.current_points[keep], search.modes[keep]
            finally:
                search.close()
            if len(keep) and 3 * n <= SYMEIG_MAX_N and verify_index:
                negatives, _ = morse_index(hessian_spectrum(DeviceArray.from_host(kept_points), n, radial=radial), zero_tol)
                kept_points, kept_modes = kept_points[negatives == 1], kept_modes[negatives == 1]
            stats["refined"] = len(kept_points)
        lap("refine")
        # 8, 9. the minima on both sides of every saddle, and the database
        if kept_points is not None and len(kept_points):
            known = DeviceArray.from_host(minima_host)
            pw = connect_saddles(DeviceArray.from_host(kept_points), DeviceArray.from_host(kept_modes), n, displacement, tol, known_minima=known,
                                 radial=radial, **quench_opts)
            # position in pw.minima -> graph index: a database member keeps its own, every other distinct end is new
            found, gid, fresh = pw.minima.to_host().reshape(-1, n3), [], []
            for pos, r in enumerate(np.flatnonzero(pw.labels == np.arange(len(pw.labels)))):
                if r < k_all:
                    gid.append(int(r))
                else:
                    gid.append(graph.add_minimum(pw.minimum_energies[pos]))
                    fresh.append(pos)
            minima_host = np.concatenate([minima_host, found[fresh]])
            stats["new_minima"] = len(fresh)
            # duplicates: the fingerprints of [saddles so far | this cycle's], an earlier row of the same label and the same edge
            both = np.concatenate([saddles_host, kept_points])
            sfp, _ = structure_fingerprints(DeviceArray.from_host(both), n, radial)
            slabels, _ = classify_structures(sfp, tol)
            s0 = len(saddles_host)
            have = {}                                        # (fingerprint label, edge) of every saddle of the graph
            for i, s, j in graph.edges:
                have[(int(slabels[s]), graph._key(i, j))] = s
            taken = []
            for r, (i, j) in enumerate(pw.edges):
                if i < 0 or j < 0:
                    stats["unresolved"] += 1
                    continue
                i, j = gid[i], gid[j]
                key = (int(slabels[s0 + r]), graph._key(i, j))
                if i == j:
                    stats["degenerate"] += 1
                elif key[0] >= 0 and key in have:
                    stats["duplicates"] += 1
                else:
                    have[key] = graph.add_saddle(pw.saddle_energies[r], i, j)
                    taken.append(r)
            saddles_host = np.concatenate([saddles_host, kept_points[taken]])
            modes_host = np.concatenate([modes_host, kept_modes[taken]])
            stats["new_saddles"] = len(taken)
        lap("connect")
        connected = is_connected()
        stats.update(connected=int(connected.sum()), minima=graph.n_minima, saddles=graph.n_saddles, seconds=seconds)
        cycles.append(stats)
    paths = [graph.best_path(i, j) for i, j in pairs]
    e_min, e_sad = np.array(graph.minimum_energies, dtype=np.float64), np.array(graph.saddle_energies, dtype=np.float64)
    barriers = np.array([np.nan if p is None else 0.0 if len(p) == 1 else e_sad[p[1::2]].max() - e_min[p[0]] for p in paths], dtype=np.float64)
    return PathwayConnections(graph=graph, minima=DeviceArray.from_host(minima_host), saddles=DeviceArray.from_host(saddles_host) if len(saddles_host) else None,
                              saddle_modes=DeviceArray.from_host(modes_host) if len(modes_host) else None, minimum_energies=e_min,
                              saddle_energies=e_sad, pairs=pairs, connected=connected, paths=paths, barriers=barriers,
                              cycles_used=cycles_used, attempts_used=attempts_used, cycles=cycles)


# ------------------------------------------------------------------------------ profiling
def profile_enable(level=2):
    """0/False off, 1 = the roofline kernels only (cheap), 2/True = every kernel."""
    _check(lib().dzo_profile_enable(2 if level is True else int(level)))


def profile_reset():
    _check(lib().dzo_profile_reset())


def unsealed_first_reads() -> int:
    """Diagnostic (include/dzo.h): how often a host wait found a kernel's published result not yet matching its seal."""
    v = C.c_int64(0)
    _check(lib().dzo_unsealed_first_reads(C.byref(v)))
    return int(v.value)


def profile_table():
    """{kernel name: (launches, total_ms)} measured with HIP events on the launching stream."""
    n = C.c_int32()
    _check(lib().dzo_profile_count(C.byref(n)))
    out = {}
    for i in range(n.value):
        name = C.create_string_buffer(96)
        launches, ms = C.c_int64(), C.c_double()
        _check(lib().dzo_profile_get(i, name, 96, C.byref(launches), C.byref(ms)))
        if launches.value:
            out[name.value.decode()] = (launches.value, ms.value)
    return out


# ------------------------------------------------------------------------------ problems
class Problem(_Handle):
    """Built-in device objective; callable like the reference's callbacks:
    ``p(x)`` = objective_function(x), ``p.gradient_(g, x)`` = gradient_function!(g, x)."""
    _prefix = "dzo_problem_"

    def __init__(self, kind, n, dtype=np.float64, A=None, c=None, lam=0.0, l2=0.0, box_gradient=None,
                 box_constraint=None):
        """``l2``: L2RegularizationWrapper + L2GradientWrapper lambda; ``box_gradient=(lo, hi)``:
        UniformBoxGradientWrapper; ``box_constraint=(lo, hi)``: UniformBoxConstraint as the
        constraint_function! of optimizers built from this problem (legacy/DZOptimization.jl:219-296)."""
        _need_init()
        self.kind, self.n, self.dtype = kind, int(n), np.dtype(dtype)
        # device layout is column-major (legacy/DZOptimization.jl:746): C-order of A' == F-order of A
        self.A = None if A is None else (A if isinstance(A, DeviceArray) else _as_dev(np.ascontiguousarray(np.asarray(A).T), dtype))
        self.c = None if c is None else _as_dev(c, dtype)
        h = C.c_void_p()
        _check(lib().dzo_problem_create(kind, self.n, _dt(dtype), self.A.ptr if self.A else None,
                                        self.c.ptr if self.c else None, lam, C.byref(h)))
        self.h = h
        if l2:
            _check(lib().dzo_problem_set_l2(h, l2))
        if box_gradient is not None:
            _check(lib().dzo_problem_set_box_gradient(h, 1, box_gradient[0], box_gradient[1]))
        if box_constraint is not None:
            _check(lib().dzo_problem_set_box_constraint(h, 1, box_constraint[0], box_constraint[1]))

    def __call__(self, x):
        f = C.c_double()
        _check(lib().dzo_problem_eval(self.h, x.ptr, C.byref(f)))
        return f.value

    def gradient_(self, g, x):
        _check(lib().dzo_problem_grad(self.h, g.ptr, x.ptr))
        return g

    def native_callbacks(self, with_constraint=False):
        """This objective in the shape of the reference's three callbacks (src/DZOptimization.jl:323-325): C function
        pointers exported by the library (``dzo_problem_*_cb``, ctx = the problem handle).  Pass the result as
        ``objective_function`` of an optimizer (the other two callback arguments are then ignored): it runs its
        general, callback-driven path with no Python frame in the loop -- what a Julia host's closures over
        ``dzo_problem_eval`` / ``dzo_problem_grad`` amount to."""
        return NativeCallbacks(self, with_constraint)


class NativeCallbacks:
    """See :meth:`Problem.native_callbacks`."""

    def __init__(self, problem, with_constraint=False):
        self.problem = problem
        L = lib()
        self.cf = C.cast(L.dzo_problem_constraint_cb, CONSTRAINT_FN) if with_constraint else C.cast(None, CONSTRAINT_FN)
        self.of = C.cast(L.dzo_problem_objective_cb, OBJECTIVE_FN)
        self.gf = C.cast(L.dzo_problem_gradient_cb, GRADIENT_FN)
        self.ctx = problem.h


def _wrap_callbacks(constraint, objective, gradient, n, dtype):
    """Python callables taking DeviceArray views -> C function pointers."""
    def mk(ptr):
        return DeviceArray(n, dtype, ptr=ptr, owner=False)
    cf = CONSTRAINT_FN(lambda ctx, x: int(bool(constraint(mk(x))))) if constraint else C.cast(None, CONSTRAINT_FN)
    of = OBJECTIVE_FN(lambda ctx, x: float(objective(mk(x))))

    def _g(ctx, g, x):
        gradient(mk(g), mk(x))
    gf = GRADIENT_FN(_g)
    return cf, of, gf


class LineSearchEvaluator:
    """``LineSearchEvaluator(constraint_function!, objective_function, gradient_function!,
    initial_point, initial_objective_value, initial_gradient, step_direction, overlap)``
    (src/DZOptimization.jl:29-62); calling it with ``(step_size, compute_gradient)`` evaluates the
    trial point ``x + t*d``, its objective, the Armijo quotient ``improvement_ratio`` (:84) and,
    optionally, the trial gradient and the curvature quotient ``slope_ratio`` (:85-90)."""

    def __init__(self, constraint_function_, objective_function, gradient_function_, initial_point,
                 initial_objective_value, initial_gradient, step_direction, overlap):
        _need_init()
        if isinstance(objective_function, Problem):
            p = objective_function
            objective_function, gradient_function_ = p, p.gradient_
        self.current_point, self.current_gradient, self.step_direction = initial_point, initial_gradient, step_direction
        self.n, self.dtype = initial_point.size, initial_point.dtype
        assert initial_gradient.size == self.n and step_direction.size == self.n        # :40-42
        self.current_objective_value, self.overlap = float(initial_objective_value), float(overlap)
        self.trial_point = DeviceArray(self.n, self.dtype)                              # :48
        self.trial_gradient = DeviceArray(self.n, self.dtype)                           # :52
        self.trial_objective_value = self.improvement_ratio = self.slope_ratio = float("nan")
        self._cbs = _wrap_callbacks(constraint_function_, objective_function,
                                    gradient_function_ if gradient_function_ is not None else (lambda g, x: None),
                                    self.n, self.dtype)
        self._has_gradient = gradient_function_ is not None

    def __call__(self, step_size, compute_gradient):
        f, ir, sr = C.c_double(), C.c_double(), C.c_double(self.slope_ratio)
        if compute_gradient and not self._has_gradient:
            raise AssertionFailed(3, "@assert !isnothing(lse.gradient_function!) (src/DZOptimization.jl:86)")
        _check(lib().dzo_line_search_eval(self._cbs[0], self._cbs[1], self._cbs[2], None, self.n, _dt(self.dtype),
                                          self.current_point.ptr, self.current_objective_value, self.step_direction.ptr,
                                          self.overlap, step_size, int(bool(compute_gradient)), self.trial_point.ptr,
                                          self.trial_gradient.ptr, C.byref(f), C.byref(ir), C.byref(sr)))
        self.trial_objective_value, self.improvement_ratio = f.value, ir.value
        if compute_gradient or f.value >= 1e38:
            self.slope_ratio = sr.value
        return f.value


class _FieldView(DeviceArray):
    """A vector field of a live optimizer (``opt.current_point`` ...).  ``to_host()`` goes through ``dzo_<opt>_read``: a copy to
    the host without a pointer hand-out, so the step behind a monitoring read does not have to check the aliased arrays for
    host writes.  Everything that needs the device pointer (``ptr``, ``upload``, ``copy``, passing the field to a kernel) asks
    ``dzo_<opt>_get_ptr`` at that moment -- the hand-out after which the host may have written (src/DZOptimization.jl:393)."""

    def __init__(self, opt, what, idx):
        self._opt, self._what, self._idx = opt, what, idx
        self.shape = (int(opt.n),)
        self.dtype = np.dtype(opt.dtype)
        self.size = int(opt.n)
        self.nbytes = self.size * self.dtype.itemsize
        self._owner = False

    @property
    def ptr(self):
        return int(self._opt._get_ptr(self._what, self._idx))

    def free(self):
        pass

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        o = self._opt
        fn = getattr(lib(), o._prefix + "read")
        _check(fn(o.h, self._what, self._idx, out.ctypes.data) if o._ptr_idx else fn(o.h, self._what, out.ctypes.data))
        return out


class _OptBase(_Handle):
    _ptr_idx = True

    def _i(self, what):
        v = C.c_int64()
        _check(getattr(lib(), self._prefix + "get_i")(self.h, what, C.byref(v)))
        return v.value

    def _s(self, what):
        v = C.c_double()
        _check(getattr(lib(), self._prefix + "get_s")(self.h, what, C.byref(v)))
        return v.value

    _has_read = False                # the C ABI has <prefix>read (a copy to the host without a pointer hand-out)

    def _get_ptr(self, what, idx=0):
        p = C.c_void_p()
        fn = getattr(lib(), self._prefix + "get_ptr")
        _check(fn(self.h, what, idx, C.byref(p)) if self._ptr_idx else fn(self.h, what, C.byref(p)))
        return p.value

    def _p(self, what, idx=0, shape=None):
        if self._has_read and shape is None:
            return _FieldView(self, what, idx)
        return DeviceArray(self.n if shape is None else shape, self.dtype, ptr=self._get_ptr(what, idx), owner=False)

    iteration_count = property(lambda s: s._i(1))
    current_objective_value = property(lambda s: s._s(0))
    current_point = property(lambda s: s._p(0))
    delta_point = property(lambda s: s._p(1))
    current_gradient = property(lambda s: s._p(2))
    delta_gradient = property(lambda s: s._p(3))


class LBFGSOptimizer(_OptBase):
    """``LBFGSOptimizer(constraint_function!, objective_function, gradient_function!,
    initial_point, initial_step_length, history_length)`` (src/DZOptimization.jl:400-407), or
    the full form with ``initial_objective_value`` and ``initial_gradient`` inserted
    (:347-356).  ``objective_function`` may be a :class:`Problem` (then ``gradient_function!``
    is ignored and may be ``None``).  The optimizer ALIASES ``initial_point`` (:393)."""

    _prefix = "dzo_lbfgs_"
    _has_read = True

    def __init__(self, constraint_function_, objective_function, gradient_function_, initial_point, *rest):
        _need_init()
        if len(rest) == 2:
            f0, g0 = None, None
            initial_step_length, history_length = rest
        elif len(rest) == 4:
            f0, g0, initial_step_length, history_length = rest
        else:
            raise TypeError("LBFGSOptimizer(c, f, g!, x0, [f0, g0,] step, m)")
        self.current_point_array = _as_dev(initial_point)
        x = self.current_point_array
        self.n, self.dtype = x.size, x.dtype
        self.history_length = int(history_length)
        self._keep = [constraint_function_, objective_function, gradient_function_, g0]
        h = C.c_void_p()
        if isinstance(objective_function, Problem) and constraint_function_ is None and g0 is None:
            self.problem = objective_function
            _check(lib().dzo_lbfgs_create_problem(self.problem.h, self.history_length, x.ptr,
                                                  initial_step_length, C.byref(h)))
        elif isinstance(objective_function, NativeCallbacks):
            nc = objective_function
            assert g0 is None, "native callbacks: use the short constructor (:400-407)"
            _check(lib().dzo_lbfgs_create_callbacks(nc.cf, nc.of, nc.gf, nc.ctx, self.n, self.history_length,
                                                    _dt(self.dtype), x.ptr, initial_step_length, C.byref(h)))
        else:
            if isinstance(objective_function, Problem):
                p = objective_function
                objective_function, gradient_function_ = p, p.gradient_
            cbs = _wrap_callbacks(constraint_function_, objective_function, gradient_function_, self.n, self.dtype)
            self._keep.append(cbs)
            if g0 is None:
                _check(lib().dzo_lbfgs_create_callbacks(cbs[0], cbs[1], cbs[2], None, self.n, self.history_length,
                                                        _dt(self.dtype), x.ptr, initial_step_length, C.byref(h)))
            else:
                _check(lib().dzo_lbfgs_create(self.n, self.history_length, _dt(self.dtype), x.ptr, g0.ptr, f0,
                                              initial_step_length, C.byref(h)))
                _check(lib().dzo_lbfgs_set_callbacks(h, cbs[0], cbs[1], cbs[2], None))
        self.h = h

    def step(self):
        """``step!(opt)`` (src/DZOptimization.jl:454-509)."""
        _check(lib().dzo_lbfgs_step(self.h))
        return self

    is_stuck = property(lambda s: bool(s._i(0)))
    has_terminated = is_stuck       # legacy/DZOptimization.jl:478
    has_converged = is_stuck        # README.md:38
    history_count = property(lambda s: s._i(4))
    last_trials = property(lambda s: s._i(5))
    delta_objective_value = property(lambda s: s._s(1))
    step_direction = property(lambda s: s._p(4))

    @property
    def delta_point_history(self):
        return [self._p(5, i) for i in range(self.history_count)]

    @property
    def delta_gradient_history(self):
        return [self._p(6, i) for i in range(self.history_count)]

    def _hist(self, fn):
        buf = (C.c_double * 64)()
        cnt = C.c_int32()
        _check(fn(self.h, buf, 64, C.byref(cnt)))
        return np.array(buf[: cnt.value])

    rho_history = property(lambda s: s._hist(lib().dzo_lbfgs_get_rho))
    alpha_history = property(lambda s: s._hist(lib().dzo_lbfgs_get_alpha))

    # split entry points (include/dzo.h)
    def set_two_loop_mode(self, mode):
        _check(lib().dzo_lbfgs_set_two_loop_mode(self.h, mode))

    def set_max_halvings(self, v):
        _check(lib().dzo_lbfgs_set_max_halvings(self.h, v))

    # optional safeguards (off = the live reference); include/dzo.h, SURVEY.md 8(f) rows 2 and 4
    def set_safeguards(self, descent_check=False, steepest_descent_fallback=False):
        """Legacy descent check (legacy/DZOptimization.jl:682-692) and steepest-descent
        fallback with history reset (:588-610)."""
        _check(lib().dzo_lbfgs_set_safeguards(self.h, int(descent_check), int(steepest_descent_fallback)))

    def set_line_search(self, kind, c1=0.0, c2=0.0, max_evals=0):
        """LINE_SEARCH_BACKTRACKING (reference) or LINE_SEARCH_WOLFE (strong Wolfe on the
        LineSearchEvaluator quotients, src/DZOptimization.jl:65-92)."""
        _check(lib().dzo_lbfgs_set_line_search(self.h, int(kind), c1, c2, int(max_evals)))

    last_step_length = property(lambda s: s._s(2))
    history_resets = property(lambda s: s._i(8))
    descent_resets = property(lambda s: s._i(9))
    last_step_kind = property(lambda s: s._i(10))
    single_pass_steps = property(lambda s: s._i(11))          # informational
    single_pass_rejections = property(lambda s: s._i(12))
    single_pass_retries = property(lambda s: s._i(13))    # rejected first trials continued by a second pass at t/2
    ring_layout = property(lambda s: s._i(14))            # 0 slabs, 1 tile-major pairs, 2 tile-major points (the point ring)
    tile_arrangement = property(lambda s: s._i(15))       # 0 no tiles (slabs), 1 tile-major, 2 stream-major
    pass_recomputes_gradients = property(lambda s: bool(s._i(16)))   # point pass: gradients of the ring's points recomputed from the point tiles
    pass_register_sets = property(lambda s: s._i(17))     # point pass: register sets per wave (1 = two waves per SIMD)
    host_write_checks = property(lambda s: s._i(18))      # point ring: steps that first compared the aliased arrays with the ring

    def compute_step_direction(self, sync=True):
        """``compute_lbfgs_step_direction!`` (:430-451).  ``sync=False`` only enqueues the kernels (the
        C entry point is asynchronous, include/dzo.h) and returns None."""
        _check(lib().dzo_lbfgs_direction(self.h))
        return self.step_direction if sync else None

    def set_history(self, S, Y, rho=None, iteration_count=None):
        S, Y = _as_dev(S, self.dtype), _as_dev(Y, self.dtype)
        k = S.shape[0] if len(S.shape) == 2 else 0
        rp = None if rho is None else (C.c_double * k)(*[float(r) for r in rho])
        _check(lib().dzo_lbfgs_set_history(self.h, k, S.ptr, Y.ptr, rp, k if iteration_count is None else iteration_count))

    def begin_search(self):
        _check(lib().dzo_lbfgs_begin_search(self.h))

    def trial(self, t):
        ch = C.c_int32()
        _check(lib().dzo_lbfgs_trial(self.h, t, C.byref(ch)))
        return bool(ch.value)

    def accept(self, f_new):
        _check(lib().dzo_lbfgs_accept(self.h, f_new))

    def reject(self):
        _check(lib().dzo_lbfgs_reject(self.h))

    def pre_gradient(self):
        _check(lib().dzo_lbfgs_pre_gradient(self.h))

    def post_gradient(self):
        _check(lib().dzo_lbfgs_post_gradient(self.h))

    def set_objective_value(self, f):
        _check(lib().dzo_lbfgs_set_s(self.h, 0, f))

    def set_last_step_length(self, v):
        _check(lib().dzo_lbfgs_set_s(self.h, 2, v))


class AdGDOptimizer(_OptBase):
    """``AdGDOptimizer(constraint!, objective, gradient!, x0, initial_step_length)``
    (src/DZOptimization.jl:245-251)."""

    _prefix = "dzo_adgd_"
    _ptr_idx = False
    _has_read = True

    def __init__(self, constraint_function_, objective_function, gradient_function_, initial_point,
                 initial_step_length):
        _need_init()
        x = self.current_point_array = _as_dev(initial_point)
        self.n, self.dtype = x.size, x.dtype
        h = C.c_void_p()
        self._keep = [constraint_function_, objective_function, gradient_function_]
        if isinstance(objective_function, Problem) and constraint_function_ is None:
            _check(lib().dzo_adgd_create_problem(objective_function.h, x.ptr, initial_step_length, C.byref(h)))
        else:
            if isinstance(objective_function, Problem):
                p = objective_function
                objective_function, gradient_function_ = p, p.gradient_
            if constraint_function_ is not None and not constraint_function_(x):
                raise AssertionFailed(3, "@assert constraint_function!(initial_point) (src/DZOptimization.jl:256-258)")
            f0 = float(objective_function(x))
            g0 = DeviceArray(self.n, self.dtype)
            gradient_function_(g0, x)
            cbs = _wrap_callbacks(constraint_function_, objective_function, gradient_function_, self.n, self.dtype)
            self._keep += [cbs, g0]
            _check(lib().dzo_adgd_create(self.n, _dt(self.dtype), x.ptr, g0.ptr, f0, initial_step_length, C.byref(h)))
            _check(lib().dzo_adgd_set_callbacks(h, cbs[0], cbs[1], cbs[2], None))
        self.h = h

    def step(self):
        _check(lib().dzo_adgd_step(self.h))
        return self

    is_stuck = property(lambda s: bool(s._i(0)))
    delta_objective_value = property(lambda s: s._s(1))
    current_step_size = property(lambda s: s._s(2))
    previous_step_size = property(lambda s: s._s(3))
    fused_steps = property(lambda s: s._i(3))
    fused_rejections = property(lambda s: s._i(4))
    pipelined_passes = property(lambda s: s._i(5))     # passes adopted that were enqueued before the previous decision was seen
    pipeline_discards = property(lambda s: s._i(6))    # passes in flight dropped (a pointer was handed out, an option changed)
    pipeline_corrections = property(lambda s: s._i(7)) # adopted passes whose device-side step size differed from the host's evaluation
    host_gradient_steps = property(lambda s: s._i(8))  # steps on the generic kernels because the host had written current_gradient


class BFGSOptimizer(_OptBase):
    """``BFGSOptimizer(objective_function, gradient_function!, [constraint_function!,]
    initial_point, initial_step_length)`` (README.md:33-36; legacy/DZOptimization.jl:753-766).
    COPIES ``initial_point`` (:769)."""

    _prefix = "dzo_bfgs_"
    _ptr_idx = False

    def __init__(self, objective_function, gradient_function_, *rest):
        _need_init()
        if len(rest) == 2:
            constraint_function_, (initial_point, initial_step_length) = None, rest
        elif len(rest) == 3:
            constraint_function_, initial_point, initial_step_length = rest
        else:
            raise TypeError("BFGSOptimizer(f, g!, [c!,] x0, step)")
        x0 = _as_dev(initial_point)
        self.n, self.dtype = x0.size, x0.dtype
        self._keep = [objective_function, gradient_function_, constraint_function_, x0]
        h = C.c_void_p()
        if isinstance(objective_function, Problem) and constraint_function_ is None:
            _check(lib().dzo_bfgs_create_problem(objective_function.h, x0.ptr, initial_step_length, C.byref(h)))
        else:
            if isinstance(objective_function, Problem):
                p = objective_function
                objective_function, gradient_function_ = p, p.gradient_
            cbs = _wrap_callbacks(constraint_function_, objective_function, gradient_function_, self.n, self.dtype)
            self._keep.append(cbs)
            _check(lib().dzo_bfgs_create_callbacks(cbs[1], cbs[2], cbs[0], None, self.n, _dt(self.dtype), x0.ptr,
                                                   initial_step_length, C.byref(h)))
        self.h = h

    @classmethod
    def convert(cls, dtype, opt, objective_function=None, gradient_function_=None, constraint_function_=None):
        """``BFGSOptimizer(::Type{T}, opt)`` / ``BFGSOptimizer(T, f, g!, c!, opt)``
        (legacy/DZOptimization.jl:812-862): continue ``opt`` in element type ``dtype``.
        ``objective_function`` must be given as a :class:`Problem` of that dtype or as callables."""
        _need_init()
        new = cls.__new__(cls)
        new.n, new.dtype = opt.n, np.dtype(dtype)
        new._keep = [objective_function, gradient_function_, constraint_function_]
        h = C.c_void_p()
        if isinstance(objective_function, Problem):
            assert objective_function.dtype == new.dtype
            _check(lib().dzo_bfgs_convert_problem(opt.h, objective_function.h, C.byref(h)))
        else:
            cbs = _wrap_callbacks(constraint_function_, objective_function, gradient_function_, new.n, new.dtype)
            new._keep.append(cbs)
            _check(lib().dzo_bfgs_convert_callbacks(opt.h, _dt(new.dtype), cbs[1], cbs[2], cbs[0], None, C.byref(h)))
        new.h = h
        return new

    def step(self):
        """``step!(opt)`` (legacy/DZOptimization.jl:891-994)."""
        _check(lib().dzo_bfgs_step(self.h))
        return self

    has_terminated = property(lambda s: bool(s._i(0)))   # legacy :738
    has_converged = has_terminated                       # README.md:38
    is_stuck = has_terminated
    last_step_type = property(lambda s: s._i(3))
    objective_evaluations = property(lambda s: s._i(4))
    last_step_length = property(lambda s: s._s(1))
    next_step_direction = property(lambda s: s._p(4))
    scratch = property(lambda s: s._p(6))                # legacy :748; after a BFGS step it holds t = H * delta_gradient (:875)

    @property
    def approximate_inverse_hessian(self):
        """n x n; ``to_host()`` gives the row-major view of the column-major (symmetric) H."""
        return self._p(5, shape=(self.n, self.n))

    def line_search(self, use_gradient_direction, t0):
        t, f = C.c_double(), C.c_double()
        _check(lib().dzo_bfgs_line_search(self.h, int(use_gradient_direction), t0, C.byref(t), C.byref(f)))
        return t.value, f.value

    def set_max_increases(self, v):
        _check(lib().dzo_bfgs_set_max_increases(self.h, v))

    def reset_inverse_hessian(self):
        """H <- I, next_step_direction <- gradient (the reset of legacy/DZOptimization.jl:981-986)."""
        _check(lib().dzo_bfgs_reset(self.h))
        return self

    def install_state(self, x, g, H, d, f, last_step_length, iteration_count=0, last_step_type=STEP_NULL,
                      dx=None, dg=None):
        """Overwrite the whole optimizer state (every field of the reference's struct is public,
        legacy/DZOptimization.jl:733-751; README.md:11 "save/load data in the middle of optimization").
        ``H``: (n, n) symmetric or column-major host array."""
        dt = self.dtype
        self.current_point.upload(np.asarray(x, dt))
        self.current_gradient.upload(np.asarray(g, dt))
        self.approximate_inverse_hessian.upload(np.ascontiguousarray(np.asarray(H, dt).T))   # column-major on the device
        self.next_step_direction.upload(np.asarray(d, dt))
        if dx is not None:
            self.delta_point.upload(np.asarray(dx, dt))
        if dg is not None:
            self.delta_gradient.upload(np.asarray(dg, dt))
        L = lib()
        _check(L.dzo_bfgs_set_s(self.h, 0, float(f)))
        _check(L.dzo_bfgs_set_s(self.h, 1, float(last_step_length)))
        _check(L.dzo_bfgs_set_i(self.h, 0, 0))
        _check(L.dzo_bfgs_set_i(self.h, 1, int(iteration_count)))
        _check(L.dzo_bfgs_set_i(self.h, 3, int(last_step_type)))
        return self


class GradientDescentOptimizer(BFGSOptimizer):
    """``GradientDescentOptimizer([constraint_function!,] objective_function, gradient_function!,
    line_search_function!, initial_point, initial_step_length)`` (legacy/DZOptimization.jl:330-390).
    ``line_search_function!`` must be ``QuadraticLineSearch()`` -- pass ``None`` or the string;
    it is the only search the reference defines (:181-216)."""

    def __init__(self, *args):
        _need_init()
        if len(args) == 5:
            constraint_function_, (objective_function, gradient_function_, _ls, initial_point, initial_step_length) = None, args
        elif len(args) == 6:
            constraint_function_, objective_function, gradient_function_, _ls, initial_point, initial_step_length = args
        else:
            raise TypeError("GradientDescentOptimizer([c!,] f, g!, line_search!, x0, step)")
        x0 = _as_dev(initial_point)
        self.n, self.dtype = x0.size, x0.dtype
        self._keep = [objective_function, gradient_function_, constraint_function_, x0]
        h = C.c_void_p()
        if isinstance(objective_function, Problem) and constraint_function_ is None:
            _check(lib().dzo_gd_create_problem(objective_function.h, x0.ptr, initial_step_length, C.byref(h)))
        else:
            if isinstance(objective_function, Problem):
                p = objective_function
                objective_function, gradient_function_ = p, p.gradient_
            cbs = _wrap_callbacks(constraint_function_, objective_function, gradient_function_, self.n, self.dtype)
            self._keep.append(cbs)
            _check(lib().dzo_gd_create_callbacks(cbs[0], cbs[1], cbs[2], None, self.n, _dt(self.dtype), x0.ptr,
                                                 initial_step_length, C.byref(h)))
        self.h = h

    def step(self):
        """``step!(opt)`` (legacy/DZOptimization.jl:393-449)."""
        _check(lib().dzo_gd_step(self.h))
        return self

    delta_objective_value = property(lambda s: s._s(2))
    approximate_inverse_hessian = property(lambda s: None)


def update_inverse_hessian_(H, step_length, d, dg, scratch, g=None, d_next=None):
    """``update_inverse_hessian!`` (legacy/DZOptimization.jl:864-889) on device arrays, with
    the optional fused next direction ``d_next = H_new * g`` (:958-960)."""
    _check(lib().dzo_bfgs_update(d.size, _dt(d.dtype), H.ptr, step_length, d.ptr, dg.ptr, scratch.ptr,
                                 g.ptr if g is not None else None, d_next.ptr if d_next is not None else None))
    return H


def update_inverse_hessian_mfma_(H, step_length, d, dg, scratch):
    """``update_inverse_hessian!`` with the rank-2 term on MFMA (fp64, n % 16 == 0); see dzo.h."""
    _check(lib().dzo_bfgs_update_mfma(d.size, _dt(d.dtype), H.ptr, step_length, d.ptr, dg.ptr, scratch.ptr))
    return H


def symv_(out, H, v):
    _check(lib().dzo_symv(v.size, _dt(v.dtype), H.ptr, v.ptr, out.ptr))
    return out


class BatchedBFGS(_Handle):
    """B independent ``BFGSOptimizer`` instances on one device (config 5)."""
    _prefix = "dzo_bfgs_batch_"

    def __init__(self, problem_kind, x0, initial_step_length, device=None, matrices=None):
        """``device``: the GPU this shard lives on (default: the device selected with ``init``); a host that
        drives several shards from one process passes each shard's device and a :class:`Comm` built with
        ``Comm.init_all``.  ``matrices`` (B x n x n, each symmetric; with a QUADRATIC ``Problem``): instance b
        minimises 1/2 x'A_b x instead of sharing the problem's A (dzo_bfgs_batch_create_problem_matrices)."""
        _need_init()
        if device is not None:
            init(int(device))                           # x0 is uploaded to that device
        x0 = _as_dev(x0)
        self.batch, self.n = x0.shape
        self.dtype = x0.dtype
        self._x0 = x0
        h = C.c_void_p()
        if matrices is not None:
            assert isinstance(problem_kind, Problem), "per-instance matrices need a QUADRATIC Problem (n, dtype, decorators)"
            self.problem = problem_kind
            assert self.problem.n == self.n and self.problem.dtype == self.dtype
            if not isinstance(matrices, DeviceArray):   # symmetric, so the row-major host layout IS column-major
                matrices = DeviceArray.from_host(np.ascontiguousarray(matrices, dtype=self.dtype))
            assert tuple(matrices.shape) == (self.batch, self.n, self.n), matrices.shape
            self._matrices = matrices                   # the caller's array must outlive the batch
            _check(lib().dzo_bfgs_batch_create_problem_matrices(self.problem.h, self.batch, matrices.ptr, self.n * self.n, x0.ptr,
                                                                initial_step_length, -1 if device is None else int(device), C.byref(h)))
        elif isinstance(problem_kind, Problem):
            # objective, shared matrix and decorators from a problem handle (dzo_bfgs_batch_create_problem)
            self.problem = problem_kind
            assert self.problem.n == self.n and self.problem.dtype == self.dtype
            _check(lib().dzo_bfgs_batch_create_problem(self.problem.h, self.batch, x0.ptr, initial_step_length,
                                                       -1 if device is None else int(device), C.byref(h)))
        elif device is None:
            _check(lib().dzo_bfgs_batch_create(problem_kind, self.batch, self.n, _dt(self.dtype), x0.ptr,
                                               initial_step_length, C.byref(h)))
        else:
            _check(lib().dzo_bfgs_batch_create_on(int(device), problem_kind, self.batch, self.n, _dt(self.dtype), x0.ptr,
                                                  initial_step_length, C.byref(h)))
        self.h = h

    @property
    def device(self):
        v = C.c_int32()
        _check(lib().dzo_bfgs_batch_device(self.h, C.byref(v)))
        return v.value

    def set_max_increases(self, v):
        """``QuadraticLineSearch.max_increases`` (legacy/DZOptimization.jl:181-188) of every instance."""
        _check(lib().dzo_bfgs_batch_set_max_increases(self.h, int(v)))

    def step(self, steps=1, poll=True):
        """Runs ``steps`` step! calls on every live instance; returns all_done if ``poll``."""
        done = C.c_int32()
        _check(lib().dzo_bfgs_batch_step(self.h, steps, C.byref(done) if poll else None))
        return bool(done.value) if poll else None

    def _p(self, what, shape, dtype=None):
        p = C.c_void_p()
        _check(lib().dzo_bfgs_batch_get_ptr(self.h, what, C.byref(p)))
        return DeviceArray(shape, self.dtype if dtype is None else dtype, ptr=p.value, owner=False)

    current_point = property(lambda s: s._p(0, (s.batch, s.n)))
    current_gradient = property(lambda s: s._p(1, (s.batch, s.n)))
    approximate_inverse_hessian = property(lambda s: s._p(2, (s.batch, s.n, s.n)))
    current_objective_value = property(lambda s: s._p(3, (s.batch,), np.float64))
    has_terminated = property(lambda s: s._p(4, (s.batch,), np.int32))
    iteration_count = property(lambda s: s._p(5, (s.batch,), np.int64))
    delta_point = property(lambda s: s._p(6, (s.batch, s.n)))
    delta_gradient = property(lambda s: s._p(7, (s.batch, s.n)))
    next_step_direction = property(lambda s: s._p(8, (s.batch, s.n)))
    last_step_length = property(lambda s: s._p(9, (s.batch,), np.float64))
    last_step_type = property(lambda s: s._p(10, (s.batch,), np.int32))

    def count_active(self):
        v = C.c_int64()
        _check(lib().dzo_bfgs_batch_count_active(self.h, C.byref(v)))
        return v.value

    def install_state(self, x, g, H, d, f, last_step_length, iteration_count=None, last_step_type=None,
                      has_terminated=None, dx=None, dg=None):
        """Overwrite the state of every instance: the arrays behind ``dzo_bfgs_batch_get_ptr`` ARE the
        state (include/dzo.h).  ``H``: (B, n, n), each symmetric or column-major."""
        B, n, dt = self.batch, self.n, self.dtype
        self.current_point.upload(np.asarray(x, dt).reshape(B, n))
        self.current_gradient.upload(np.asarray(g, dt).reshape(B, n))
        self.approximate_inverse_hessian.upload(np.ascontiguousarray(np.transpose(np.asarray(H, dt).reshape(B, n, n), (0, 2, 1))))
        self.next_step_direction.upload(np.asarray(d, dt).reshape(B, n))
        self.current_objective_value.upload(np.asarray(f, np.float64).reshape(B))
        self.last_step_length.upload(np.asarray(last_step_length, np.float64).reshape(B))
        self.iteration_count.upload(np.zeros(B, np.int64) if iteration_count is None else np.asarray(iteration_count, np.int64))
        self.last_step_type.upload(np.zeros(B, np.int32) if last_step_type is None else np.asarray(last_step_type, np.int32))
        self.has_terminated.upload(np.zeros(B, np.int32) if has_terminated is None else np.asarray(has_terminated, np.int32))
        if dx is not None:
            self.delta_point.upload(np.asarray(dx, dt).reshape(B, n))
        if dg is not None:
            self.delta_gradient.upload(np.asarray(dg, dt).reshape(B, n))
        return self


def _preload_rccl():
    """Same reasoning as _preload_hip_runtime: libdzo_hip.so dlopen()s librccl.so.1 at first use; when
    PyTorch is installed its bundled copy (same SONAME) must be the one in the process."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


class Comm(_Handle):
    """The one collective of the design (include/dzo.h): all-reduce(MIN) of the convergence flag of
    sharded independent optimizers over RCCL / xGMI, behind the C ABI.

    ``Comm.init_all(devices)``: one process, several GPUs (ncclCommInitAll).
    ``Comm.init_rank(uid, nranks, rank)``: one process per GPU; ``Comm.unique_id()`` on rank 0, carried to
    the other ranks by the launcher (``Comm.from_torch_distributed()`` does that over an initialised
    ``torch.distributed`` group)."""
    _prefix = "dzo_comm_"

    def __init__(self, h):
        self.h = h

    @staticmethod
    def unique_id() -> bytes:
        _need_init()
        _preload_rccl()
        buf = C.create_string_buffer(128)
        _check(lib().dzo_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def init_rank(cls, uid: bytes, nranks: int, rank: int):
        _need_init()
        _preload_rccl()
        assert len(uid) == 128
        h = C.c_void_p()
        _check(lib().dzo_comm_init_rank(C.create_string_buffer(uid, 128), nranks, rank, C.byref(h)))
        return cls(h)

    @classmethod
    def init_all(cls, devices):
        lib()
        _preload_rccl()
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _check(lib().dzo_comm_init_all(arr, len(devices), C.byref(h)))
        global _inited
        _inited = True
        return cls(h)

    @classmethod
    def from_torch_distributed(cls):
        """One rank per process of an initialised ``torch.distributed`` group: rank 0's unique id is
        broadcast through the group (any backend), then every rank joins."""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        # Every rank runs the SAME sequence of collectives whatever fails locally (a rank that raised before a
        # collective the others have entered would hang the group): (1) every rank probes that it can load RCCL
        # through the C ABI -- rank 0's probe is the id itself -- and the outcomes are gathered; (2) only when all
        # are fine does anyone enter the RCCL bootstrap; (3) the outcomes of that are gathered as well.
        uid, err = None, None
        try:
            uid = cls.unique_id()                         # (ranks > 0: a probe; their id is dropped)
        except Exception as e:                            # noqa: BLE001 -- reported to every rank below
            err = f"rank {rank}: {e}"
        box = [None] * world
        dist.all_gather_object(box, (uid if rank == 0 else None, err))
        errs = [b[1] for b in box if b[1]]
        if errs:
            raise DzoError(5, "RCCL communicator not created (no rank entered the bootstrap): " + "; ".join(errs))
        comm, err = None, None
        try:
            comm = cls.init_rank(box[0][0], world, rank)
        except Exception as e:                            # noqa: BLE001
            err = f"rank {rank}: {e}"
        box = [None] * world
        dist.all_gather_object(box, err)
        errs = [b for b in box if b]
        if errs:
            if comm is not None:
                comm.close()
            raise DzoError(2, "ncclCommInitRank failed: " + "; ".join(errs))
        return comm

    def _info(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().dzo_comm_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    nranks = property(lambda s: s._info()[0])
    nlocal = property(lambda s: s._info()[1])
    first_rank = property(lambda s: s._info()[2])
    collectives = property(lambda s: s._info()[3])

    def allreduce_min(self, local_flags) -> int:
        flags = [int(local_flags)] if np.isscalar(local_flags) or isinstance(local_flags, bool) else [int(f) for f in local_flags]
        arr = (C.c_int32 * len(flags))(*flags)
        out = C.c_int32()
        _check(lib().dzo_flag_allreduce_min_n(self.h, arr, len(flags), C.byref(out)))   # (the count is checked against the local ranks)
        return out.value

    def all_done(self, batches) -> bool:
        """``dzo_bfgs_batch_all_done``: every instance of every shard (local and remote) has terminated."""
        hs = (C.c_void_p * len(batches))(*[b.h for b in batches])
        out = C.c_int32()
        _check(lib().dzo_bfgs_batch_all_done(self.h, hs, len(batches), C.byref(out)))
        return bool(out.value)


def batches_all_done(batches, comm=None) -> bool:
    """``dzo_bfgs_batch_all_done`` with or without a communicator."""
    hs = (C.c_void_p * len(batches))(*[b.h for b in batches])
    out = C.c_int32()
    _check(lib().dzo_bfgs_batch_all_done(comm.h if comm is not None else None, hs, len(batches), C.byref(out)))
    return bool(out.value)


def step_(opt):
    """``step!(opt)``: the reference's generic function (src/DZOptimization.jl:104)."""
    return opt.step()


# every public class and function of the module, in the order of their definitions (tests/test_abi.py holds it to that)
__all__ = [
    "DzoError", "AssertionFailed", "build", "lib", "init", "device_info", "device_count", "synchronize",
    "calibrate_read_bandwidth", "selftest_fast_div", "calibrate_read_bandwidth_of", "DeviceArray", "axpy_", "axpby_", "rmul_",
    "copy_", "fill_", "dot", "norm", "isequal", "norm2", "inv_norm", "negate_", "scale_", "box_clamp_", "trial_point_",
    "calibrate_fma_rate", "pairwise_radial_energy", "pairwise_radial_gradient_", "pairwise_radial_hvp_",
    "pairwise_radial_energy_delta", "ParallelTempering", "pairwise_batch_energy_gradient", "BatchedLBFGS", "sphere_project_",
    "sphere_energy_gradient", "SphereLBFGS", "BasinHopping",
    "BatchedAdGD", "pairwise_batch_hvp", "pairwise_batch_hessian", "hessian_eigenvalues", "morse_index", "symeig_plan",
    "symmetric_batch_eigen", "hessian_spectrum", "LowestModes", "lowest_modes", "modefollow_apply", "ModeFollowing",
    "polish_minima", "find_saddles", "hybridef_apply", "HybridModeFollowing", "find_saddles_hybrid", "structure_fingerprints",
    "classify_structures", "unique_structures", "Pathways", "quench_to_rest", "connect_saddles", "neb_plan", "interpolate_band",
    "neb_apply", "ElasticBand", "BandConnections", "connect_minima", "assign_particles", "Alignment", "align_pairs", "BandCandidates",
    "band_candidates", "PathwayGraph", "PathwayConnections", "connect_pathways", "profile_enable",
    "profile_reset", "unsealed_first_reads", "profile_table", "Problem", "NativeCallbacks", "LineSearchEvaluator",
    "LBFGSOptimizer", "AdGDOptimizer", "BFGSOptimizer", "GradientDescentOptimizer", "update_inverse_hessian_",
    "update_inverse_hessian_mfma_", "symv_", "BatchedBFGS", "Comm", "batches_all_done", "step_",
]
