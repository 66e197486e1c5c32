// dzo_lbfgs_plan.h -- every DECISION of the L-BFGS unit (dzo_lbfgs.hip) as a plain function of plain inputs: which ring
// layout and tile arrangement a handle gets, where its scalars live, which step path a step takes, which kernel
// instantiation and launch shape a pass uses.  No HIP here: the header compiles with a plain C++17 compiler, so the whole
// input range (the 2^32 byte-offset limits included) is tested on the CPU (tools/lbfgs_plan_table.cpp,
// tests/test_lbfgs_plan.py).  The host code of dzo_lbfgs.hip allocates, launches and updates state by these plans.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/dzo.h"

namespace dzo {

// dzo_common.h's values, restated (dzo_lbfgs.hip static_asserts them equal)
constexpr int kPlanWaves = 4, kPlanMaxHistory = 64, kPlanMaxPartialBlocks = 2048;

constexpr int kGramValues = 5;  // per pair: s.g, y.g, y.y_p, y.s_p, s.y_p  (p = pivot pair)
constexpr int kRowOwn = 62;                     // wave-row geometry of the single-pass kernel (see there)
constexpr int kRowLead = (64 - kRowOwn) / 2;
constexpr int kTileBytes = 64 * 16;             // one stream's share of a wave-row in the blocked ring
constexpr int kPairMaxK = 20;                  // pairs the single-pass step over a PAIR ring holds (its largest instantiation)
// points the point pass holds: K = 20 is what fits two waves per SIMD (247 of 256 registers); fp64 has one more
// instantiation, K = 24 on two register sets and one wave per SIMD (508 of 512), so that m = 21 .. 24 do not fall
// back to the two-pass kernels (n = 1e7, m = 24: 683 step!()/s there)
static inline int point_max_k(int32_t dtype) { return dtype == DZO_F64 ? 24 : 20; }
constexpr int kFusedMaxK = 24;                 // two register sets of 2k history vectors: 2*2*20 x 16 B per lane
constexpr int kStreamU = 4;                    // 16-byte vectors per thread the Gram and combine passes start from (halved for a small n)

static inline int64_t plan_dtype_size(int32_t dtype) { return dtype == DZO_F64 ? 8 : 4; }

struct RingDecor {
    double l2 = 0; bool bg_on = false; double bg_lo = 0, bg_hi = 0; bool cons_on = false; double cons_lo = 0, cons_hi = 0;
    bool any() const { return l2 != 0.0 || bg_on || cons_on; }
    bool operator==(const RingDecor &o) const {
        return l2 == o.l2 && bg_on == o.bg_on && cons_on == o.cons_on && (!bg_on || (bg_lo == o.bg_lo && bg_hi == o.bg_hi)) &&
               (!cons_on || (cons_lo == o.cons_lo && cons_hi == o.cons_hi));
    }
};

// ---------------------------------------------------------------------------- construction
// The DZO_TUNE_* values a constructor reads (dev only; the defaults are the product).  lbfgs_read_knobs fills it once
// per construction.  The knobs that are read per step stay out: tests switch those on live handles.
struct LbfgsKnobs {
    int single_pass = 1, point_ring = 1;
    bool stream_major_set = false;              // unset: stream-major from m = 9 on
    int stream_major = 0;
    int lse_points = 1, point_sets = 1;
    int fused_finish = 0, speculate = 1, fused_post = 1;
};

// What dzo_lbfgs_create_problem knows and the constructor needs; empty for dzo_lbfgs_create (no problem: never blocked).
struct LbfgsStart {
    int kind = -1;                              // DZO_PROBLEM_*; -1: none
    RingDecor dec;                              // the decorators the start point's gradient was formed under
    double lambda = 0;                          // the objective's parameter
    bool x_al16 = false, g_al16 = false, c_al16 = false;   // 16-byte alignment of the start point, its gradient, the LSE centre
};

// the chained objectives the passes serve (ChainObj): 0 Rosenbrock, 1 chained quadratic, 2 log-sum-exp (its own kernels); -1 none
static inline int ring_obj_of_kind(int kind) {
    return kind == DZO_PROBLEM_ROSENBROCK_CHAIN ? 0 : (kind == DZO_PROBLEM_QUADRATIC_CHAIN ? 1 : (kind == DZO_PROBLEM_LSE ? 2 : -1));
}

// The scalar block: ONE list gives the length of every sub-array, so their offsets and the size of the allocation
// cannot disagree.  In doubles.  kScalSlack: kMaxHistory doubles at the end that nothing uses (the allocation has
// always been that much larger than what is carved from it; kept, so that no size or address moves).
enum LbfgsScalar {
    kScalGramTicket, kScalXgDiffers, kScalPscal, kScalRho, kScalAlpha, kScalCoef, kScalScale, kScalAlphaSp, kScalCoefSp,
    kScalScaleSp, kScalGyy, kScalGsy, kScalSg, kScalYg, kScalGramPartials, kScalLinkPartials, kScalSlack, kScalCount
};
struct LbfgsScalars {
    size_t off[kScalCount], len[kScalCount], total;
};
static inline LbfgsScalars lbfgs_plan_scalars(int nslots, int gram_grid) {
    const size_t m1 = (size_t)nslots, H = kPlanMaxHistory;
    LbfgsScalars s = {{}, {
        2,                                       // gram_ticket (zeroed with the rest; re-armed by the kernel)
        2,                                       // xg_differs
        2 * (m1 + 2),                            // pscal [nslots][2] (and the LSE centre's slot)
        m1,                                      // rho, by slot
        H, H, 8,                                 // alpha, coef, scale
        H, H, 8,                                 // the _sp three
        m1 * m1, m1 * m1,                        // Gyy, Gsy
        H, H,                                    // sg, yg
        (size_t)kGramValues * H * ((size_t)gram_grid * kPlanWaves + 1),   // gram_partials (+ the reduced values)
        4 * (size_t)kPlanMaxPartialBlocks,       // link_partials: ping-pong + yy
        H,                                       // slack
    }, 0};
    for (int i = 0; i < kScalCount; ++i) { s.off[i] = s.total; s.total += s.len[i]; }
    return s;
}

// Everything the constructor decides before it allocates.
struct LbfgsLayout {
    int64_t stride = 0;                         // elements between slots: n rounded up to 1 KiB, an ODD number of KiB
    bool blocked = false, points = false;       // tile ring; ... of points
    int ring_obj = 0;                           // the objective the passes recompute
    int nslots = 0;                             // m + 1 (pairs + the spare); m + 2 for a tile ring (m + 1 POINTS + the spare)
    int64_t ring_rows = 0, tile_stride = kTileBytes, rowbytes = 0;
    size_t ring_bytes = 0;                      // tile ring: the one allocation
    int64_t pair_stride = 0;                    // elements between consecutive slots of the same history (slabs: s_0 y_0 s_1 y_1 ...)
    size_t slab_bytes = 0;                      // nslots slots of one history
    size_t lin_bytes = 0;                       // one contiguous vector (dx_lin, dg_lin; the payload of d)
    size_t d_bytes = 0, d_offset = 0;           // d's allocation, and d within it: off the allocator's alignment grid
    int gram_grid = 0;                          // upper bound of the reducing grids (sizes the partials)
    int point_sets = 1;
    LbfgsScalars scal;
};

static inline bool lbfgs_plan_want_blocked(const LbfgsStart &st, const LbfgsKnobs &kn) {
    // the pass will apply: built-in chained Rosenbrock (decorated or not), undecorated chained quadratic, undecorated
    // log-sum-exp with an aligned centre
    const bool lse_points = st.kind == DZO_PROBLEM_LSE && !st.dec.any() && st.c_al16 && kn.lse_points != 0;
    return (st.kind == DZO_PROBLEM_ROSENBROCK_CHAIN || (st.kind == DZO_PROBLEM_QUADRATIC_CHAIN && !st.dec.any()) || lse_points) &&
           st.x_al16 && st.g_al16;
}

static inline LbfgsLayout lbfgs_plan_layout(int64_t n, int32_t dtype, int m, const LbfgsStart &st, const LbfgsKnobs &kn, int cus) {
    LbfgsLayout L;
    const size_t es = (size_t)plan_dtype_size(dtype);
    const int64_t vecn = 16 / (int64_t)es;
    {
        // slot stride: n rounded up to 1 KiB, and an ODD number of KiB, so that the 2(m+1) streams
        // never sit a power-of-two distance apart (same HBM channel / bank for equal offsets)
        size_t sb = ((size_t)n * es + 1023) / 1024 * 1024;
        if ((sb / 1024) % 2 == 0) sb += 1024;
        L.stride = (int64_t)(sb / es);
    }
    L.ring_obj = ring_obj_of_kind(st.kind) >= 1 ? ring_obj_of_kind(st.kind) : 0;
    // blocked (tile) ring: when the constructor knows that the single-pass step applies
    // (a ragged n: phantom padding, load_vec_tail -- on the POINT ring only)
    L.blocked = lbfgs_plan_want_blocked(st, kn) && kn.single_pass != 0 && m <= point_max_k(dtype) &&
                n >= 4 * vecn && (uint64_t)n * es < (1ull << 32) && (n % vecn == 0 || kn.point_ring != 0);
    L.nslots = m + (L.blocked ? 2 : 1);
    L.slab_bytes = (size_t)L.nslots * (size_t)L.stride * es;
    L.lin_bytes = (size_t)L.stride * es;
    if (L.blocked) {
        const int64_t nvec = (n + vecn - 1) / vecn;
        L.ring_rows = (nvec + kRowOwn - 1) / kRowOwn;
        const int64_t stream_bytes = ((L.ring_rows * kTileBytes + 1023) / 1024 | 1) * 1024;   // an odd number of KiB (HBM channel skew)
        const int ms = L.nslots + (L.ring_obj == 2 ? 1 : 0);      // (log-sum-exp: slot nslots holds the tiles of the centre vector c)
        const uint64_t total = (uint64_t)2 * ms * (uint64_t)stream_bytes;
        // (few streams: the whole wave-row of a tile-major ring sits in a handful of DRAM pages and its reads win --
        // n = 1e7: m = 5 pass 234 us tile-major / 253 us stream-major, m = 10 398 / 383, m = 20 684 / 660)
        const bool want_stream = (kn.stream_major_set ? kn.stream_major : (m >= 9 ? 1 : 0)) != 0;
        if (want_stream && total + (1u << 20) < (1ull << 32)) {      // 32-bit byte offsets in the passes
            L.tile_stride = stream_bytes; L.rowbytes = kTileBytes; L.ring_bytes = (size_t)total;
        } else {
            L.tile_stride = kTileBytes; L.rowbytes = (int64_t)2 * ms * kTileBytes;
            L.ring_bytes = (size_t)L.ring_rows * (size_t)L.rowbytes;
        }
        L.pair_stride = 0;
    } else {
        L.pair_stride = 2 * L.stride;
    }
    L.d_bytes = L.lin_bytes + 4096;
    L.d_offset = 3 * 1024;
    L.gram_grid = cus * 8;
    if (L.gram_grid > kPlanMaxPartialBlocks) L.gram_grid = kPlanMaxPartialBlocks;
    {
        const int64_t tile_v = 64 * (int64_t)kStreamU;
        const int64_t tiles = (n / vecn + tile_v - 1) / tile_v;
        if (tiles < L.gram_grid) L.gram_grid = (int)(tiles > 0 ? tiles : 1);
    }
    if (L.blocked && kn.point_ring != 0) {
        // point ring: the start point and its gradient are point 0
        L.points = true;
        L.point_sets = kn.point_sets == 1 ? 1 : 2;
    }
    L.scal = lbfgs_plan_scalars(L.nslots, L.gram_grid);
    return L;
}

// ---------------------------------------------------------------------------- step path
// What a step looks at to choose its path (the pure part: the wrappers in dzo_lbfgs.hip add the fused-post query
// and the twin allocation).
struct LbfgsStepFacts {
    bool points = false, single_pass = false, blocked = false;
    int mode = DZO_TWOLOOP_GRAM, line_search = 0;
    bool descent_check = false, sd_fallback = false, speculate = true, fused_post = true;
    bool callbacks = false;                     // an objective, gradient or constraint callback is set
    bool box_on = false, has_problem = false;
    int64_t iteration_count = 0, n = 0;
    int k = 0, m = 0;
    int32_t dtype = DZO_F64;
    int ring_obj = 0;
    bool ring_decorated = false;                // the set the ring was stored under has a decorator on
    bool obj_agrees = false, dec_agrees = false, lambda_agrees = false, lse_c_agrees = false;   // problem handle vs ring
    bool spec_scalars = false, d_al16 = false;
};

static inline bool lbfgs_plain_options(const LbfgsStepFacts &f) {
    return f.single_pass && f.blocked && f.mode == DZO_TWOLOOP_GRAM && f.line_search == 0 && !f.descent_check && !f.sd_fallback &&
           !f.callbacks && f.speculate && f.fused_post;
}

// can this step run as one pass over a PAIR ring?  (then, in the wrapper: the problem's fused post kernel, d aligned, twins)
static inline bool single_pass_plan_ok(const LbfgsStepFacts &f) {
    if (!lbfgs_plain_options(f) || f.box_on) return false;
    if (f.iteration_count == 0 || f.k < 1 || f.k > kPairMaxK || f.m > kPairMaxK) return false;   // (m: the pass also forms the dots of pair k + 1)
    const int64_t vecn = 16 / plan_dtype_size(f.dtype);
    // (a ragged n never gets here: its tile ring exists as a POINT ring only -- lbfgs_leave_points hands it to the slabs)
    return f.n >= 4 * vecn && (uint64_t)f.n * (uint64_t)plan_dtype_size(f.dtype) < (1ull << 32);   // 32-bit byte offsets
}

// the point ring serves exactly the optimizers the single-pass step serves (and, unlike it, the first step)
static inline bool points_plan_ok(const LbfgsStepFacts &f) {
    if (!f.points || !lbfgs_plain_options(f) || !f.has_problem) return false;
    // (the decorators of legacy :219-296 ride on the pass: its DEC instantiations, under the set the ring was stored with)
    if (!f.obj_agrees || !f.dec_agrees) return false;
    if (f.ring_obj >= 1 && (f.ring_decorated || !f.lambda_agrees)) return false;   // (no DEC instantiations of those objectives)
    if (f.ring_obj == 2 && !f.lse_c_agrees) return false;
    if (f.k > point_max_k(f.dtype) || f.m > point_max_k(f.dtype) || !f.d_al16) return false;
    return f.k == 0 || f.spec_scalars;          // (the scalars come from the previous pass; anything else goes through Gram passes)
}

// ---------------------------------------------------------------------------- kernel variants
// the template arguments of lbfgs_point_pass_kernel<T, K, FIRST, SETS, DEC, OBJ>
struct PassVariant {
    int K, SETS; bool DEC; int OBJ; bool FIRST;
    bool operator==(const PassVariant &o) const { return K == o.K && SETS == o.SETS && DEC == o.DEC && OBJ == o.OBJ && FIRST == o.FIRST; }
};

// one register set per wave (two waves per SIMD)?  DZO_TUNE_POINT_SETS=1 (the default), where the instantiation fits 256 registers
// (fp32, K > 12: the fp64 copies for the dots do not fit)
static inline bool point_one_set(int m, int32_t dtype, int point_sets) { return point_sets == 1 && m <= 20 && (dtype == DZO_F64 || m <= 12); }

// the instantiation of the point pass: the smallest offered K that holds m pairs (m <= point_max_k)
static inline PassVariant point_pass_variant(int m, int32_t dtype, bool one_set, bool decorated, int obj, bool first) {
    const bool dec = obj != 1 && decorated;     // (no DEC instantiations of the chained quadratic)
    if (first) return {8, 2, dec, obj == 1 ? 1 : 0, true};      // the first step's kernel: no history
    const int by4 = m <= 8 ? 8 : m <= 12 ? 12 : m <= 16 ? 16 : 20;
    int K;
    if (obj == 1 || decorated) {
        // fewer instantiations: the next larger K serves the history lengths in between
        K = one_set ? by4 : (dtype == DZO_F64 && m > 20) ? 24 : (m <= 12 ? 12 : by4);
    } else if (one_set) {
        // every even K (K = 10: m = 10 is the history length most L-BFGS users ask for; on the K = 12 instantiation it paid
        // for two masked pairs -- 211 us per pass at n = 1e7 where m = 12 takes 218)
        K = m <= 6 ? 6 : (m + 1) / 2 * 2;
    } else {
        // (K = 22 for m = 21, 22: on K = 24 they paid for two or three masked pairs)
        K = (dtype == DZO_F64 && m > 20) ? (m <= 22 ? 22 : 24) : by4;
    }
    return {K, one_set ? 1 : 2, dec, obj == 1 ? 1 : 0, false};
}

// lbfgs_single_pass_kernel<T, K> (pair ring): register footprint follows the history length
static inline int pair_pass_k(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : 20; }
// lse_dots_kernel<T, K>
static inline int lse_dots_k(int m, int32_t dtype) { return (dtype == DZO_F64 && m > 20) ? 24 : m <= 8 ? 8 : m <= 12 ? 12 : 20; }

// ---------------------------------------------------------------------------- launch shapes
// grid of a pass: a block per kPlanWaves wave-rows, at most the blocks resident at once, bounded by the partial-sum buffers
static inline int pass_grid(int64_t rows, int64_t resident, int gram_grid, int cap) {
    int64_t blocks = (rows + kPlanWaves - 1) / kPlanWaves;
    if (blocks > resident) blocks = resident;
    if (blocks > (int64_t)gram_grid * kPlanWaves) blocks = (int64_t)gram_grid * kPlanWaves;
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}
constexpr int kPairPassGridCap = kPlanMaxPartialBlocks;        // two objective partials per block in the problem scratch
constexpr int kPointPassGridCap = kPlanMaxPartialBlocks / 2;   // up to four (2 kMaxPartialBlocks doubles)

// tile-major ring: plain stores while the two streams fit the 256-MiB Infinity Cache (695 vs 735 us at
// n = 1e7); stream-major ring: non-temporal (655-672 vs 659-682 us over four interleaved rounds)
static inline int point_plain_mb_default(int64_t tile_stride) { return tile_stride == kTileBytes ? 200 : 0; }

constexpr int kPointStageRows = 16;             // what the host asks point_pass_launch for
// Rows of new tiles a wave collects in LDS before it writes them: 1 KiB per staged tile, row and wave; the 160-KiB LDS
// of a CU is one block's with two register sets per wave (144 KiB of it staged) and two blocks' with one (72 KiB each).
struct PointLaunch {
    bool one_set;                               // this launch runs two waves per SIMD
    int stage_tiles, stage_max, stage_rows;
    size_t stage_bytes;                         // dynamic LDS
    int nt_tiles, prio;
};
static inline size_t point_stage_bytes(int stage_rows, int stage_tiles) { return (size_t)kPlanWaves * stage_rows * stage_tiles * kTileBytes; }
// a device that does not grant the dynamic-LDS attribute: stay within the default 64 KiB
static inline int point_stage_small_rows(int stage_tiles) { return 14 / stage_tiles; }
static inline PointLaunch point_pass_launch(int64_t n, int32_t dtype, int m, int k, int point_sets, bool regrad,
                                            int stage_rows_knob, int prio_knob, int64_t plain_mb) {
    PointLaunch p;
    p.nt_tiles = 2 * n * plan_dtype_size(dtype) > (plain_mb << 20) ? 1 : 0;
    p.one_set = point_one_set(m, dtype, point_sets) && k > 0;
    p.prio = p.one_set ? (prio_knob != 0 ? 1 : 0) : 0;   // (two waves per SIMD only; see the kernel)
    p.stage_tiles = (k == 0 || !regrad) ? 2 : 1;          // tiles staged per row: the point, and its gradient where the kernel writes it
    p.stage_max = (p.one_set ? 72 : 144) / (4 * p.stage_tiles);   // KiB of LDS per block / (waves x KiB per staged row)
    p.stage_rows = stage_rows_knob < 1 ? 1 : stage_rows_knob;
    if (p.stage_rows > p.stage_max) p.stage_rows = p.stage_max;
    p.stage_bytes = point_stage_bytes(p.stage_rows, p.stage_tiles);
    return p;
}

}  // namespace dzo
