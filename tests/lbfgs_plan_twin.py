"""The decisions of the L-BFGS unit restated in Python, for tests/test_lbfgs_plan.py (against csrc/dzo_lbfgs_plan.h through
tools/lbfgs_plan_table.cpp, on the CPU) and tests/test_gpu_lbfgs_plan.py (against real handles).  A helper module like
tests/quench_checks.py (no fixtures; imported by name).

Written from csrc/dzo_lbfgs.hip as it stood BEFORE the decisions moved into the plan header (commit f1e6518); the line
numbers below are that file's.  It restates what that code decided, in the order it decided it -- it is not a port of the
header.
"""
F32, F64 = 0, 1                                   # include/dzo.h:43-44
ROSENBROCK2D, ROSENBROCK_CHAIN, QUADRATIC, LSE, QUADRATIC_CHAIN = 0, 1, 2, 3, 4   # include/dzo.h:56-60
NO_PROBLEM = -1
K_WAVES, K_MAX_PARTIAL_BLOCKS, K_MAX_HISTORY = 4, 2048, 64      # dzo_common.h:25-28
K_GRAM_VALUES = 5                                 # :36
K_ROW_OWN, K_TILE_BYTES = 62, 1024                # :51, :53
K_ROW_LEAD = (64 - K_ROW_OWN) // 2                # :52
K_PAIR_MAX_K, K_FUSED_MAX_K = 20, 24              # :997, :1002
U32 = 1 << 32

KNOB_DEFAULTS = dict(SINGLE_PASS=1, POINT_RING=1, STREAM_MAJOR=None, LSE_POINTS=1, POINT_SETS=1, FUSED_FINISH=0, SPECULATE=1, FUSED_POST=1)
SCALARS = ["gram_ticket", "xg_differs", "pscal", "rho", "alpha", "coef", "scale", "alpha_sp", "coef_sp", "scale_sp", "Gyy", "Gsy", "sg", "yg",
           "gram_partials", "link_partials"]      # the order of :3965-3980


def es_of(dtype):
    return 8 if dtype == F64 else 4


def point_max_k(dtype):                           # :1001
    return 24 if dtype == F64 else 20


def ring_obj_of(kind):                            # :2700-2703
    return {ROSENBROCK_CHAIN: 0, QUADRATIC_CHAIN: 1, LSE: 2}.get(kind, -1)


def want_blocked(kind, decorated, x_al, g_al, c_al, knobs):
    """dzo_lbfgs_create_problem, :4080-4083."""
    lse_points = kind == LSE and not decorated and c_al and knobs["LSE_POINTS"] != 0
    return (kind == ROSENBROCK_CHAIN or (kind == QUADRATIC_CHAIN and not decorated) or lse_points) and x_al and g_al


def layout(n, dtype, m, kind=NO_PROBLEM, decorated=False, x_al=True, g_al=True, c_al=True, cus=256, knobs=None):
    """dzo_lbfgs_create, :3860-4001.  kind = NO_PROBLEM: the thread-locals at their defaults (dzo_lbfgs_create called directly)."""
    kn = dict(KNOB_DEFAULTS)
    kn.update(knobs or {})
    es = es_of(dtype)
    L = {}
    sb = (n * es + 1023) // 1024 * 1024           # :3882
    if (sb // 1024) % 2 == 0:                     # :3883 (the skew: always)
        sb += 1024
    L["stride"] = sb // es
    wanted = kind != NO_PROBLEM and want_blocked(kind, decorated, x_al, g_al, c_al, kn)
    L["ring_obj"] = ring_obj_of(kind) if ring_obj_of(kind) >= 1 else 0      # :4085
    vecn = 16 // es
    L["blocked"] = bool(wanted and kn["SINGLE_PASS"] != 0 and m <= point_max_k(dtype) and n >= 4 * vecn and
                        n * es < U32 and (n % vecn == 0 or kn["POINT_RING"] != 0))      # :3892-3894
    m1 = L["nslots"] = m + (2 if L["blocked"] else 1)                                 # :3896
    slab = L["slab_bytes"] = m1 * L["stride"] * es                                    # :3898
    L["ring_rows"], L["tile_stride"], L["rowbytes"], L["ring_bytes"] = 0, K_TILE_BYTES, 0, 0   # the struct's defaults (:133, :140, :141)
    if L["blocked"]:
        nvec = (n + vecn - 1) // vecn                                                 # :3905
        L["ring_rows"] = (nvec + K_ROW_OWN - 1) // K_ROW_OWN
        stream_bytes = (((L["ring_rows"] * K_TILE_BYTES + 1023) // 1024) | 1) * 1024      # :3908
        ms = m1 + (1 if L["ring_obj"] == 2 else 0)                                    # :3909
        total = 2 * ms * stream_bytes
        stream_major = kn["STREAM_MAJOR"] if kn["STREAM_MAJOR"] is not None else (1 if m >= 9 else 0)
        if stream_major != 0 and total + (1 << 20) < U32:                             # :3913
            L["tile_stride"], L["rowbytes"], L["ring_bytes"] = stream_bytes, K_TILE_BYTES, total
        else:
            L["tile_stride"], L["rowbytes"] = K_TILE_BYTES, 2 * ms * K_TILE_BYTES
            L["ring_bytes"] = L["ring_rows"] * L["rowbytes"]
        L["pair_stride"] = 0                                                          # :3922
    else:
        L["pair_stride"] = 2 * L["stride"]                                            # :3928 (one slab, s and y interleaved)
    L["lin_bytes"] = L["stride"] * es                                                 # :3923
    L["d_bytes"], L["d_offset"] = L["stride"] * es + 4096, 3 * 1024                   # :3934-3935
    grid = cus * 8                                                                    # :3951
    grid = min(grid, K_MAX_PARTIAL_BLOCKS)
    tile_v = 64 * 4
    tiles = (n // vecn + tile_v - 1) // tile_v                                        # :3955
    if tiles < grid:
        grid = tiles if tiles > 0 else 1
    L["gram_grid"] = grid
    # :3958-3959, the size of the block ...
    L["scalar_total"] = (2 + 2 + 2 * (m1 + 2) + m1 + 3 * K_MAX_HISTORY + 8 + 2 * m1 * m1 + 2 * K_MAX_HISTORY + (2 * K_MAX_HISTORY + 8) +
                         K_GRAM_VALUES * K_MAX_HISTORY * (grid * K_WAVES + 1) + 4 * K_MAX_PARTIAL_BLOCKS)
    # ... and :3965-3980, the `base += ...` lines
    lens = [2, 2, 2 * (m1 + 2), m1, K_MAX_HISTORY, K_MAX_HISTORY, 8, K_MAX_HISTORY, K_MAX_HISTORY, 8, m1 * m1, m1 * m1, K_MAX_HISTORY,
            K_MAX_HISTORY, K_GRAM_VALUES * K_MAX_HISTORY * (grid * K_WAVES + 1)]
    off, base = {}, 0
    for name, ln in zip(SCALARS, lens + [None]):
        off[name] = base
        if ln is not None:
            base += ln
    L["scalar_offsets"] = off
    L["link_partials_len"] = 4 * K_MAX_PARTIAL_BLOCKS      # (four columns of kMaxPartialBlocks: :80)
    L["points"] = bool(L["blocked"] and kn["POINT_RING"] != 0)                        # :3997
    L["point_sets"] = (1 if kn["POINT_SETS"] == 1 else 2) if L["points"] else 1       # :4001 / :183
    return L


# ------------------------------------------------------------------------------ what the getters report (:4231-4235)
def ring_layout(blocked, points):
    return 2 if points else (1 if blocked else 0)


def tile_arrangement(L):
    return (1 if L["tile_stride"] == K_TILE_BYTES else 2) if L["blocked"] else 0


def point_one_set(m, dtype, point_sets):          # :3338
    return point_sets == 1 and m <= 20 and (dtype == F64 or m <= 12)


def pass_register_sets(L, m, dtype):
    return (1 if point_one_set(m, dtype, L["point_sets"]) else 2) if L["points"] else 0


def layout_after_leaving_points(L, n, dtype, chain_mode):
    """An option the passes do not serve (lbfgs_step :3818 -> lbfgs_leave_points :2793-2818): the ring becomes a pair ring
    in place, a ragged n continues on the slabs (:2816); CHAIN mode leaves the tiles for good (lbfgs_unblock, :4136)."""
    if not L["blocked"] or chain_mode or n % (16 // es_of(dtype)) != 0:
        return 0
    return 1


# ------------------------------------------------------------------------------ step path
def points_ok(f):
    """:3145-3156.  f: the facts as a dict (see test_lbfgs_plan.FACTS)."""
    if not f["points"] or not f["single_pass"] or not f["blocked"] or f["mode"] != 1 or f["line_search"] != 0 or f["descent_check"] or f["sd_fallback"]:
        return False
    if f["callbacks"] or not f["speculate"] or not f["fused_post"] or not f["has_problem"]:
        return False
    if not f["obj_agrees"] or not f["dec_agrees"]:
        return False
    if f["ring_obj"] >= 1 and (f["ring_decorated"] or not f["lambda_agrees"]):
        return False
    if f["ring_obj"] == 2 and not f["lse_c_agrees"]:
        return False
    if f["k"] > point_max_k(f["dtype"]) or f["m"] > point_max_k(f["dtype"]) or not f["d_al16"]:
        return False
    if f["k"] > 0 and not f["spec_scalars"]:
        return False
    return True


def single_pass_ok(f):
    """:3128-3137, without the fused-post query and the twins."""
    if not f["single_pass"] or not f["blocked"] or f["mode"] != 1 or f["line_search"] != 0 or f["descent_check"] or f["sd_fallback"]:
        return False
    if f["callbacks"] or f["box_on"] or not f["speculate"] or not f["fused_post"]:
        return False
    if f["iteration_count"] == 0 or f["k"] < 1 or f["k"] > K_PAIR_MAX_K or f["m"] > K_PAIR_MAX_K:
        return False
    vecn = 16 // es_of(f["dtype"])
    if f["n"] < 4 * vecn or f["n"] * es_of(f["dtype"]) >= U32:
        return False
    return f["d_al16"]


# ------------------------------------------------------------------------------ kernel variants
def ladder(m, steps):
    """`m <= a ? A : m <= b ? B : ... : LAST`"""
    for k in steps[:-1]:
        if m <= k:
            return k
    return steps[-1]


def point_pass_variant(m, dtype, point_sets, decorated, obj, first):
    """point_pass_kernel_for / point_pass_kernel_sel, :3342-3407 -> (K, SETS, DEC, OBJ, FIRST)."""
    f64 = dtype == F64
    if first:                                     # :3404-3405
        return (8, 2, False, 1, True) if obj == 1 else (8, 2, bool(decorated), 0, True)
    one = point_one_set(m, dtype, point_sets)
    if obj == 1 or decorated:                     # :3343-3376: the same ladder for both
        dec, o = (False, 1) if obj == 1 else (True, 0)
        if one:
            return (ladder(m, [8, 12, 16, 20]) if f64 else ladder(m, [8, 12]), 1, dec, o, False)
        if f64 and m > 20:
            return (24, 2, dec, o, False)
        return (ladder(m, [12, 16, 20]), 2, dec, o, False)
    if one:                                       # :3377-3394
        return (ladder(m, [6, 8, 10, 12, 14, 16, 18, 20]) if f64 else ladder(m, [6, 8, 10, 12]), 1, False, 0, False)
    if f64 and m > 20:                            # :3396
        return (22 if m <= 22 else 24, 2, False, 0, False)
    return (ladder(m, [8, 12, 16, 20]), 2, False, 0, False)     # :3397-3400


POINT_PASS_OFFERED = {  # the instantiations the ladders name, per (dtype, SETS, DEC, OBJ)
    F64: {(1, False, 0): [6, 8, 10, 12, 14, 16, 18, 20], (2, False, 0): [8, 12, 16, 20, 22, 24], (1, True, 0): [8, 12, 16, 20],
          (2, True, 0): [12, 16, 20, 24], (1, False, 1): [8, 12, 16, 20], (2, False, 1): [12, 16, 20, 24]},
    F32: {(1, False, 0): [6, 8, 10, 12], (2, False, 0): [8, 12, 16, 20], (1, True, 0): [8, 12], (2, True, 0): [12, 16, 20],
          (1, False, 1): [8, 12], (2, False, 1): [12, 16, 20]},
}


def pair_pass_k(m):                               # :3229-3231
    return ladder(m, [8, 16, 20])


def lse_dots_k(m, dtype):                         # :3643-3644
    return 24 if dtype == F64 and m > 20 else ladder(m, [8, 12, 20])


# ------------------------------------------------------------------------------ launch shape of the point pass (:3478-3506)
def point_launch(n, dtype, m, k, point_sets, regrad, stage_rows_knob, prio_knob, plain_mb):
    P = {}
    P["nt_tiles"] = 1 if 2 * n * es_of(dtype) > (plain_mb << 20) else 0              # :3482
    one = P["one_set"] = point_one_set(m, dtype, point_sets) and k > 0                # :3487
    P["prio"] = (1 if prio_knob != 0 else 0) if one else 0                            # :3488
    tiles = P["stage_tiles"] = 2 if (k == 0 or not regrad) else 1                     # :3490
    P["stage_max"] = (72 if one else 144) // (4 * tiles)                              # :3491
    rows = max(stage_rows_knob, 1)                                                    # :3492-3494
    P["stage_rows"] = min(rows, P["stage_max"])
    P["stage_bytes"] = K_WAVES * P["stage_rows"] * tiles * K_TILE_BYTES               # :3495
    P["small_rows"] = 14 // tiles                                                     # :3503-3505
    P["small_bytes"] = K_WAVES * P["small_rows"] * tiles * K_TILE_BYTES
    return P


def pass_grid(rows, resident, gram_grid, cap):
    """points_grid :3326-3335 (cap kMaxPartialBlocks / 2), lse_grid :3646-3654 (the same), the pair pass :3235-3240 (kMaxPartialBlocks)."""
    blocks = (rows + K_WAVES - 1) // K_WAVES
    blocks = min(blocks, resident, gram_grid * K_WAVES, cap)
    return max(blocks, 1)
