// dzo_phi_search.h -- the quadratic line search of the dense BFGS step (find_three_point_bracket + QuadraticLineSearch,
// legacy/DZOptimization.jl:49-216) as ONE resumable state machine, the only statement of the search in the library.  The
// machine asks for an evaluation (phi_begin, then phi_feed after every value) and ends with t_best / f_best (phi_result).
// Three drivers run it:
//   phi_sequential_search      one evaluation at a time over an evaluator: the dense search of dzo_bfgs.hip for callbacks,
//                              constraints and every objective without a two-direction kernel.  It alone knows the
//                              tiny-step path (:91-101, :107-123).  (The batched step kernel of dzo_batch.hip keeps a copy
//                              of this search in T arithmetic: as this loop's evaluator it measured 2.5 % slower.)
//   bfgs_dual_search,          speculative: every launch evaluates the point the machine needs now plus the one or two it
//   finish_phi6_advance_kernel will most likely need next (phi_post), and phi_consume feeds the primary, then the speculative
//                              values that match what the machine asks for next.  Same decisions, values and evaluation
//                              counts -- only the order in which evaluations reach the device changes.  A first point
//                              that does not move parks the machine (kPhiSequential) for the sequential driver.
//
// For the speculative drivers trial points and gradients are INDICES: a trial point is its request slot (0: the search's
// scratch vector, 1, 2: its two speculative buffers), a gradient its entry of the gradient pool (phi_pool_index).  The
// host-driven search (bfgs_dual_search) turns them into buffers, the device-driven one works on them as they are.
//
// No HIP here: every function is __host__ __device__ under hipcc and plain inline under a C++17 compiler, so every path of
// the search runs on the CPU against the oracle (tools/phi_search_table.cpp, tests/test_phi_search.py).  Arithmetic is in
// double, rounded to the dtype (phi_rt) wherever the oracle holds a T.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define DZO_PHI_FN __host__ __device__ __forceinline__
#else
#define DZO_PHI_FN inline
#endif

namespace dzo {

constexpr int32_t kPhiF32 = 0;                     // include/dzo.h's DZO_F32, restated (dzo_bfgs.hip static_asserts them equal)

enum { kPhiFirst = 0, kPhiDoubling, kPhiShrinking, kPhiQuadratic, kPhiDone, kPhiSequential };

struct PhiMachine {
    double f0, t0, step, fa, req_t, x1, f1, x2, f2, xb, fb, t_best, f_best;
    double spec_t[3];
    int32_t state, increases, want, req_ref;
    int32_t spec_ref[3], active[3];
    int32_t step_grad, g1, g2, best_grad;          // gradient-pool entries (-1: none) of: the point `step`, the bracket ends, the best point so far
    int32_t step_round, r1, r2, best_round;        // ... and the rounds that wrote them
    int32_t ref_buf;                               // the trial-point buffer (= request slot) that holds the reference point (:136 / :155)
};

// the requests of one launch as the machines post them: step sizes (signed, already rounded to the dtype), which of the
// six run, and what each one's :150 test compares with
struct PhiReqDev {
    double ts[2][3];
    int32_t active[2][3];
    int32_t ref_req[2][3];      // the request of the same direction in this launch to compare with, or -1
    int32_t use_ref[2][3];      // [side][0]: 0 = no stored reference point, 1 + b = the direction's trial-point buffer b (point_out[b]) as it stands
};

DZO_PHI_FN double phi_rt(int32_t dt, double v) { return dt == kPhiF32 ? (double)(float)v : v; }   // round to the dtype

// the gradient pool holds the last four rounds: six entries a round, three a side
DZO_PHI_FN int phi_pool_index(int round, int side, int slot) { return (round % 4) * 6 + side * 3 + slot; }

template <typename V> DZO_PHI_FN V phi_sel3(int i, V a, V b, V c) { return i == 0 ? a : (i == 1 ? b : c); }

// :203-209: the minimum of the parabola through (0, f0), (x1, f1), (x2, f2), x2 = 2 x1; false when there is none to ask for
DZO_PHI_FN bool phi_quadratic_request(int32_t dt, double f0, double x1, double f1, double /* x2 */, double f2, double *xq) {
    const double d1 = phi_rt(dt, f0 - f1), d2 = phi_rt(dt, f2 - f1);
    const double sum = phi_rt(dt, d1 + d2);                      // :203-205
    if (!(d1 >= 0 && d2 >= 0 && sum > 0)) return false;          // :206
    const double num = phi_rt(dt, phi_rt(dt, d1 + d1) + sum);
    const double ratio = phi_rt(dt, num / phi_rt(dt, sum + sum));   // :207-208
    *xq = phi_rt(dt, ratio * x1);                                // :209
    return true;
}

DZO_PHI_FN void phi_to_quadratic(int32_t dt, PhiMachine &q) {    // QuadraticLineSearch after :195
    q.xb = 0; q.fb = q.f0; q.best_grad = -1; q.best_round = 0;   // :196
    if (q.f1 < q.fb) { q.xb = q.x1; q.fb = q.f1; q.best_grad = q.g1; q.best_round = q.r1; }   // :197-199
    if (q.f2 < q.fb) { q.xb = q.x2; q.fb = q.f2; q.best_grad = q.g2; q.best_round = q.r2; }   // :200-202
    double xq;
    if (phi_quadratic_request(dt, q.f0, q.x1, q.f1, q.x2, q.f2, &xq)) {
        q.req_t = xq;
        q.want = 1; q.req_ref = 0;
        q.state = kPhiQuadratic;
    } else {
        q.t_best = q.xb; q.f_best = q.fb;
        q.want = 0;
        q.state = kPhiDone;
    }
}

DZO_PHI_FN void phi_bracket_done(int32_t dt, PhiMachine &q, double x1, double f1, double x2, double f2, int g1 = -1, int r1 = 0,
                                 int g2 = -1, int r2 = 0) {
    q.x1 = x1; q.f1 = f1; q.x2 = x2; q.f2 = f2; q.g1 = g1; q.r1 = r1; q.g2 = g2; q.r2 = r2;
    phi_to_quadratic(dt, q);
}

DZO_PHI_FN void phi_begin(int32_t dt, PhiMachine &q, double f0, double t0) {
    q.f0 = f0; q.t0 = t0;
    q.step = q.fa = q.req_t = q.x1 = q.f1 = q.x2 = q.f2 = q.xb = q.fb = q.t_best = q.f_best = 0;
    q.increases = 0; q.want = 0; q.req_ref = 0;
    q.step_grad = q.g1 = q.g2 = q.best_grad = -1;
    q.step_round = q.r1 = q.r2 = q.best_round = 0;
    q.ref_buf = 0;
    q.state = kPhiDone;
    for (int e = 0; e < 3; ++e) { q.spec_t[e] = 0; q.spec_ref[e] = 0; q.active[e] = 0; }
    if (!__builtin_isfinite(f0) || !(t0 > 0) || !__builtin_isfinite(t0)) { phi_bracket_done(dt, q, 0, f0, 0, f0); return; }   // :64-66 -> bracket (0, f0, 0, f0)
    q.state = kPhiFirst;
    q.step = t0;
    q.req_t = t0; q.want = 1; q.req_ref = 0;
}

// the value of the pending request.  slot: where the evaluation's trial point lies; cur_grad / cur_round: its gradient;
// equal_ref(): whether the trial point is the reference point, called only if :150 is reached
template <typename EqualRef>
DZO_PHI_FN void phi_feed(int32_t dt, int32_t max_increases, PhiMachine &q, double f, bool changed, bool nonzero, EqualRef &&equal_ref,
                         int slot, int cur_grad, int cur_round, int64_t &evals) {
    q.want = 0;
    switch (q.state) {
    case kPhiFirst:
        if (!nonzero) { phi_bracket_done(dt, q, 0, q.f0, 0, q.f0); return; }   // :83-85 (the speculative value is dropped)
        if (!changed) { q.state = kPhiSequential; return; }                    // :91-101 tiny-step path: rare, done sequentially
        evals += 1;
        q.fa = f;                                                // :104
        q.step_grad = cur_grad; q.step_round = cur_round;
        if (q.fa <= q.f0) {                                      // :130
            q.increases = 0;
            q.ref_buf = slot;                                    // :136
            q.state = kPhiDoubling;
            q.req_t = phi_rt(dt, q.step + q.step); q.increases += 1;
            q.want = 1; q.req_ref = 1;
        } else {
            q.state = kPhiShrinking;
            q.req_t = phi_rt(dt, 0.5 * q.step);
            q.want = 1; q.req_ref = 0;
        }
        return;
    case kPhiDoubling: {                                         // :143-156
        evals += 1;
        const double dbl = q.req_t, fb = f;
        bool stop = (max_increases > 0 && q.increases >= max_increases) || !__builtin_isfinite(fb) || fb > q.fa;
        if (!stop) stop = equal_ref();                           // :150, asked for last: it costs a pass over the point
        if (stop) { phi_bracket_done(dt, q, q.step, q.fa, dbl, fb, q.step_grad, q.step_round, cur_grad, cur_round); return; }   // :151
        q.step = dbl; q.fa = fb; q.step_grad = cur_grad; q.step_round = cur_round;
        q.ref_buf = slot;                                        // :155
        q.req_t = phi_rt(dt, q.step + q.step); q.increases += 1;
        q.want = 1; q.req_ref = 1;
        return;
    }
    case kPhiShrinking: {                                        // :157-171
        evals += 1;
        const double hs = q.req_t, fb = f;
        if (fb <= q.f0) { phi_bracket_done(dt, q, hs, fb, q.step, q.fa, cur_grad, cur_round, q.step_grad, q.step_round); return; }   // :166
        if (hs == 0.0) { phi_bracket_done(dt, q, 0, q.f0, 0, q.f0); return; }
        q.step = hs; q.fa = fb; q.step_grad = cur_grad; q.step_round = cur_round;
        q.req_t = phi_rt(dt, 0.5 * q.step);
        q.want = 1; q.req_ref = 0;
        return;
    }
    case kPhiQuadratic:                                          // :210-213
        evals += 1;
        if (f < q.fb) { q.xb = q.req_t; q.fb = f; q.best_grad = cur_grad; q.best_round = cur_round; }
        q.t_best = q.xb; q.f_best = q.fb;
        q.state = kPhiDone;
        return;
    default:
        return;
    }
}

// The requests of the next launch: the evaluation the machine needs now (slot 0) plus the one or two it will most likely
// need next (slots 1, 2) -- the first doubling and the first halving after the first point, the next doubling / halving
// inside those loops.  All of them ride on the same pass over A; phi_consume uses a speculative value only if the machine
// then asks for exactly that point.
DZO_PHI_FN void phi_post(int32_t dt, double sign, PhiMachine &q, PhiReqDev &R, int side) {
    for (int e = 0; e < 3; ++e) {
        q.spec_t[e] = 0; q.spec_ref[e] = 0; q.active[e] = 0;
        R.ts[side][e] = 0; R.active[side][e] = 0; R.ref_req[side][e] = -1; R.use_ref[side][e] = 0;
    }
    if (!q.want) return;
    auto post = [&](int slot, double t, int use_ref, int ref_req, int is_ref) {
        R.ts[side][slot] = phi_rt(dt, sign * t);
        R.active[side][slot] = 1; R.use_ref[side][slot] = use_ref; R.ref_req[side][slot] = ref_req;
        q.spec_t[slot] = t; q.spec_ref[slot] = is_ref; q.active[slot] = 1;
    };
    post(0, q.req_t, q.req_ref ? 1 + q.ref_buf : 0, -1, q.req_ref);
    if (q.state == kPhiFirst) {
        post(1, phi_rt(dt, q.req_t + q.req_t), 0, 0, 1);         // first doubling (:143), :150 against slot 0
        post(2, phi_rt(dt, 0.5 * q.req_t), 0, -1, 0);            // first halving (:158)
    } else if (q.state == kPhiDoubling) {
        post(1, phi_rt(dt, q.req_t + q.req_t), 0, 0, 1);
    } else if (q.state == kPhiShrinking) {
        post(1, phi_rt(dt, 0.5 * q.req_t), 0, -1, 0);
    }
}

// One launch's results for one direction: its three values (rounded to the dtype), its nine flag words {changed, nonzero,
// differs from the reference} x slot, the gradient-pool entry of this round's and side's slot 0.  The primary request is
// fed first, then every speculative one that is what the machine asks for next; the others are dropped uncounted.
// Returns the slots fed, in order, as slot + 1 in two bits a turn (tools/phi_search_table.cpp prints them).
// (phi_sel3 and a bit mask: no dynamically indexed private arrays, which would land in scratch memory on the device)
DZO_PHI_FN int phi_consume(int32_t dt, int32_t max_increases, PhiMachine &q, double f_0, double f_1, double f_2, const int32_t *hf,
                           int pool_base, int round, int64_t &evals) {
    int fed = 0;
    if (!q.active[0]) return fed;
    int used = 0, slot = 0;
    for (int turn = 0; turn < 3; ++turn) {                       // (at most the three requests of this direction)
        used |= 1 << slot;
        fed |= (slot + 1) << (2 * turn);
        const int changed = phi_sel3(slot, hf[0], hf[3], hf[6]);
        const int nonzero = phi_sel3(slot, hf[1], hf[4], hf[7]);
        const int differs = phi_sel3(slot, hf[2], hf[5], hf[8]);
        phi_feed(dt, max_increases, q, phi_sel3(slot, f_0, f_1, f_2), changed != 0, nonzero != 0, [equal = differs == 0] { return equal; }, slot,
                 pool_base + slot, round, evals);
        if (!q.want) break;
        int next = -1;
        for (int e = 1; e < 3; ++e)
            if (q.active[e] && !(used & (1 << e)) && q.spec_t[e] == q.req_t && q.spec_ref[e] == q.req_ref) next = e;
        if (next < 0) break;
        slot = next;
    }
    return fed;
}

// What a search that stopped asking hands to the step: t_best / f_best and the gradient-pool entry of the gradient at the
// best point -- or -1 when there is none to use: the search moved nowhere, or the entry has been recycled since (the pool
// holds four rounds).  state == kPhiSequential is the caller's to finish (the tiny-step path, :91-101).
DZO_PHI_FN void phi_result(const PhiMachine &q, int round, double *t, double *f, int *grad_index) {
    *t = q.t_best; *f = q.f_best;
    *grad_index = (q.state == kPhiDone && q.t_best != 0.0 && q.best_grad >= 0 && round - q.best_round < 4) ? q.best_grad : -1;
}

// ------------------------------------------------------------------------------------------------------------------
// The sequential search: one evaluation at a time, the tiny-step path included.

DZO_PHI_FN double phi_typemax(int32_t dt) { return dt == kPhiF32 ? 3.4028234663852886e38 : 1.7976931348623157e308; }   // typemax(T), :41

// :91-101: the first trial point is x itself -- ask again at twice the step; a step that overflows ends the search at x
DZO_PHI_FN void phi_tiny_double(int32_t dt, PhiMachine &q) {
    q.step = q.req_t = phi_rt(dt, q.step + q.step);
    if (!__builtin_isfinite(q.step)) phi_bracket_done(dt, q, 0, q.f0, 0, q.f0);
}

enum { kPhiAtT0 = 0, kPhiAtTinyDouble, kPhiAtDoubling, kPhiAtOther };

// The whole search over an evaluator E, which holds x, the direction, the trial point and the reference point:
//   void   point(double t, int at, bool &changed, bool &nonzero)
//                                       trial point <- x + sign t dir.  at (kPhiAt...) says which point of the search this is, and
//                                       so what is wanted: at t0 both flags of :71-80, after a tiny doubling `changed` alone (and
//                                       objective() will likely not follow), else no flag (while doubling same_as_reference() may follow)
//   double objective(bool *feasible)    P(trial point) and, if feasible, the objective there -- E counts this evaluation
//   bool   same_as_x(), same_as_reference()                             the trial point against x (:119), the reference point (:150)
//   void   keep_reference()             reference point <- trial point (:136 / :155)
//   bool   failed()                     stops the loop; what was found so far is returned
// The objective is asked for only where the oracle asks: not at a point that did not move (:91-101), not at an infeasible one
// (its value is typemax(T), uncounted), and :150 only when the cheaper tests of :147-149 have not ended the doubling.
template <typename E> DZO_PHI_FN void phi_sequential_run(int32_t dt, int32_t max_increases, E &ev, double f0, double t0, PhiMachine &q) {
    phi_begin(dt, q, f0, t0);
    bool small = false;
    int64_t fed = 0;                                             // (E counts: an infeasible point is fed, not evaluated)
    while (q.want && !ev.failed()) {
        const bool first = q.state == kPhiFirst;
        bool changed = true, nonzero = true, feasible = true;
        ev.point(q.req_t, first ? (small ? kPhiAtTinyDouble : kPhiAtT0) : (q.req_ref ? kPhiAtDoubling : kPhiAtOther), changed, nonzero);
        if (nonzero && !changed) { small = true; phi_tiny_double(dt, q); continue; }
        const double f = nonzero ? ev.objective(&feasible) : 0.0;
        if (small && first && (!feasible || ev.same_as_x())) { phi_bracket_done(dt, q, 0, f0, 0, f0); continue; }   // :107-123
        phi_feed(dt, max_increases, q, feasible ? f : phi_typemax(dt), true, nonzero, [&] { return ev.same_as_reference(); }, 0, -1, 0, fed);
        if (q.state == kPhiDoubling) ev.keep_reference();
    }
}
template <typename E>
DZO_PHI_FN void phi_sequential_search(int32_t dt, int32_t max_increases, E &ev, double f0, double t0, double *t_best, double *f_best) {
    PhiMachine q;
    phi_sequential_run(dt, max_increases, ev, f0, t0, q);
    int grad_index;
    phi_result(q, 0, t_best, f_best, &grad_index);
}

}  // namespace dzo
