// phi_search_table.cpp -- stand-alone driver of csrc/dzo_phi_search.h (no GPU, no HIP): runs line searches the way the two
// drivers of dzo_bfgs.hip do -- phi_begin, then phi_post / evaluate every active slot / phi_consume until the machine stops
// asking -- on small objectives evaluated here, and prints what each search did.  tests/test_phi_search.py compares every
// line with the oracle's sequential search.
//
//   phi_search_table FILE       one query per line of FILE (reals as C hex floats, exact in the query's dtype):
//       dtype kind n  x[n] dir[n] c[n] m[n]  f0_given f0  t0 max_increases sign
//     dtype: 0 fp32, 1 fp64 (include/dzo.h).  The objective, every operation rounded to the dtype, summed in index order:
//       kind 0: sum c_i * d_i     kind 1: sum c_i * (d_i * d_i)     kind 2: sum c_i * ((d_i * d_i) * (d_i * d_i)),   d_i = p_i - m_i
//     f0_given 0: f0 is the objective at x.  The trial point of step t is fma(sign * t, dir_i, x_i).
//   one answer per line (reals as the bit patterns of their doubles, in hex):
//       state increases quadratic_asked evals rounds posted grad_index t_best f_best f0 x1 f1 x2 f2 consumed
//       then per consumed evaluation, in order:  round slot t f point[n]
//
//   phi_search_table --sequential FILE      the same queries through the header's own sequential loop (phi_sequential_run) over
//     an evaluator defined here; a query may end with a constraint  cons lo hi  (1: clamp every coordinate into [lo, hi], 2: a point
//     with a coordinate outside [lo, hi] is infeasible).  The answer format stands above run_sequential.
//
//   g++ -std=c++17 -Wall -Werror -ffp-contract=off -fsanitize=address,undefined tools/phi_search_table.cpp -o phi_search_table
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../dzoptimization.jl_amd/csrc/dzo_phi_search.h"

using namespace dzo;

constexpr int kMaxN = 3;

template <typename T> struct Query {
    int kind = 0, n = 0, cons = 0;
    T x[kMaxN], dir[kMaxN], c[kMaxN], m[kMaxN], lo = 0, hi = 0;
};

template <typename T> static T objective(const Query<T> &Q, const T *p) {
    T acc = 0;
    for (int i = 0; i < Q.n; ++i) {
        const T d = p[i] - Q.m[i];
        T w = d;
        if (Q.kind >= 1) w = d * d;
        if (Q.kind == 2) w = w * w;
        w = Q.c[i] * w;
        acc = acc + w;
    }
    return acc;
}

static unsigned long long bits(double v) {
    unsigned long long u;
    memcpy(&u, &v, sizeof u);
    return u;
}

template <typename T>
static int run(int32_t dt, const Query<T> &Q, bool f0_given, double f0, double t0, int32_t max_increases, double sign) {
    if (!f0_given) f0 = (double)objective(Q, Q.x);
    PhiMachine q;
    PhiReqDev R;
    phi_begin(dt, q, f0, t0);
    T pts[3][kMaxN] = {};                                        // the trial-point buffer of each request slot, as the last launch left it
    int round = 0, posted = 0, consumed = 0;
    bool quadratic_asked = false;
    int64_t evals = 0;
    std::string trace;
    char buf[64];
    for (;;) {
        phi_post(dt, sign, q, R, 0);
        if (!q.want) break;
        round += 1;
        T np[3][kMaxN] = {};
        double f[3] = {0, 0, 0};
        int32_t hf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};             // {changed, nonzero, differs from the reference} x slot
        for (int e = 0; e < 3; ++e) {
            if (!R.active[0][e]) continue;
            posted += 1;
            const T ts = (T)R.ts[0][e];
            for (int i = 0; i < Q.n; ++i) {
                np[e][i] = std::fma(ts, Q.dir[i], Q.x[i]);
                hf[e * 3 + 0] |= Q.x[i] != np[e][i];
                hf[e * 3 + 1] |= Q.dir[i] != (T)0;
            }
            f[e] = (double)objective(Q, np[e]);
        }
        for (int e = 0; e < 3; ++e) {                            // :150 against a request of this launch, or a buffer as it stands
            if (!R.active[0][e]) continue;
            const T *ref = R.ref_req[0][e] >= 0 ? np[R.ref_req[0][e]] : (R.use_ref[0][e] ? pts[R.use_ref[0][e] - 1] : nullptr);
            for (int i = 0; ref && i < Q.n; ++i) hf[e * 3 + 2] |= np[e][i] != ref[i];
        }
        for (int e = 0; e < 3; ++e)
            if (R.active[0][e]) memcpy(pts[e], np[e], sizeof pts[e]);
        const int64_t before = evals;
        const int fed = phi_consume(dt, max_increases, q, phi_rt(dt, f[0]), phi_rt(dt, f[1]), phi_rt(dt, f[2]), hf,
                                    phi_pool_index(round, 0, 0), round, evals);
        int nfed = 0;
        while (nfed < 3 && ((fed >> (2 * nfed)) & 3) != 0) nfed += 1;
        if (evals != before) {                                   // (a first point that is dropped -- zero direction, tiny step -- is fed uncounted)
            if (evals - before != nfed) return 4;
            for (int turn = 0; turn < nfed; ++turn) {
                const int slot = ((fed >> (2 * turn)) & 3) - 1;
                snprintf(buf, sizeof buf, " %d %d %llx %llx", round, slot, bits(q.spec_t[slot]), bits(phi_rt(dt, f[slot])));
                trace += buf;
                for (int i = 0; i < Q.n; ++i) { snprintf(buf, sizeof buf, " %llx", bits((double)pts[slot][i])); trace += buf; }
                consumed += 1;
            }
        }
        quadratic_asked |= q.state == kPhiQuadratic;
    }
    double t_best, f_best;
    int grad_index;
    phi_result(q, round, &t_best, &f_best, &grad_index);
    printf("%d %d %d %lld %d %d %d %llx %llx %llx %llx %llx %llx %llx %d%s\n", q.state, q.increases, (int)quadratic_asked, (long long)evals,
           round, posted, grad_index, bits(t_best), bits(f_best), bits(f0), bits(q.x1), bits(q.f1), bits(q.x2), bits(q.f2), consumed,
           trace.c_str());
    return 0;
}

// The evaluator of the header's sequential loop over the same objectives, with the query's constraint; it records every point
// whose objective was asked for and what the tiny-step path met.
template <typename T> struct Evaluator {
    const Query<T> &Q;
    int32_t dt;
    double sign;
    T y[kMaxN] = {}, ref[kMaxN] = {};
    double t = 0, last_f = 0;                                    // last_f: what the last call of objective() stood for in the search
    int unchanged = 0, infeasible = 0, at_x = 0, compared = 0;
    std::string trace;
    int evaluated = 0;
    bool failed() const { return false; }
    void point(double step, int at, bool &changed, bool &nonzero) {
        t = step;
        const T ts = (T)(sign * step);
        bool ch = false, nz = false;
        for (int i = 0; i < Q.n; ++i) {
            y[i] = std::fma(ts, Q.dir[i], Q.x[i]);
            ch |= Q.x[i] != y[i];
            nz |= Q.dir[i] != (T)0;
        }
        if (at <= kPhiAtTinyDouble) { changed = ch; unchanged += !ch; }
        if (at == kPhiAtT0) nonzero = nz;
    }
    double objective(bool *feasible) {
        for (int i = 0; i < Q.n; ++i) {
            if (Q.cons == 1) y[i] = y[i] < Q.lo ? Q.lo : (y[i] > Q.hi ? Q.hi : y[i]);
            if (Q.cons == 2 && !(y[i] >= Q.lo && y[i] <= Q.hi)) { *feasible = false; infeasible += 1; last_f = phi_typemax(dt); return 0; }
        }
        const double f = (double)::objective(Q, y);
        char buf[64];
        snprintf(buf, sizeof buf, " %llx %llx", bits(t), bits(f));
        trace += buf;
        for (int i = 0; i < Q.n; ++i) { snprintf(buf, sizeof buf, " %llx", bits((double)y[i])); trace += buf; }
        evaluated += 1;
        return last_f = f;
    }
    bool same(const T *a, const T *b) const {                    // Julia's isequal: the same bits, or both NaN
        for (int i = 0; i < Q.n; ++i)
            if (!(a[i] != a[i] && b[i] != b[i]) && memcmp(&a[i], &b[i], sizeof(T)) != 0) return false;
        return true;
    }
    bool same_as_x() { at_x = same(y, Q.x); return at_x != 0; }
    bool same_as_reference() { compared += 1; return same(y, ref); }
    void keep_reference() { memcpy(ref, y, sizeof ref); }
};

// --sequential: phi_sequential_run over the Evaluator.  One answer per line:
//     state increases quadratic_asked evaluated unchanged infeasible at_x compared t_best f_best f0 x1 f1 x2 f2 last_f
//     then per evaluated point, in order:  t f point[n]
template <typename T>
static int run_sequential(int32_t dt, const Query<T> &Q, bool f0_given, double f0, double t0, int32_t max_increases, double sign) {
    if (!f0_given) f0 = (double)objective(Q, Q.x);
    Evaluator<T> ev{Q, dt, sign};
    PhiMachine q;
    phi_sequential_run(dt, max_increases, ev, f0, t0, q);
    double t_best, f_best;
    int grad_index;
    phi_result(q, 0, &t_best, &f_best, &grad_index);
    double xq;
    const bool quadratic_asked = phi_quadratic_request(dt, q.f0, q.x1, q.f1, q.x2, q.f2, &xq);   // (a function of the bracket alone)
    printf("%d %d %d %d %d %d %d %d %llx %llx %llx %llx %llx %llx %llx %llx%s\n", q.state, q.increases, (int)quadratic_asked, ev.evaluated, ev.unchanged,
           ev.infeasible, ev.at_x, ev.compared, bits(t_best), bits(f_best), bits(f0), bits(q.x1), bits(q.f1), bits(q.x2), bits(q.f2), bits(ev.last_f),
           ev.trace.c_str());
    return 0;
}

template <typename T> static int answer(int32_t dt, int kind, int n, const char *rest, bool sequential) {
    Query<T> Q;
    Q.kind = kind; Q.n = n;
    T *fields[4] = {Q.x, Q.dir, Q.c, Q.m};
    int used = 0;
    for (T *field : fields)
        for (int i = 0; i < kMaxN; ++i) {
            field[i] = 0;
            if (i >= n) continue;
            double v;
            if (sscanf(rest, "%la%n", &v, &used) != 1) return 2;
            rest += used;
            field[i] = (T)v;
            if ((double)field[i] != v && v == v) return 3;       // (the query's reals are exact in its dtype)
        }
    int f0_given, max_increases;
    double f0, t0, sign;
    double lo = 0, hi = 0;
    const int got = sscanf(rest, "%d %la %la %d %la %d %la %la", &f0_given, &f0, &t0, &max_increases, &sign, &Q.cons, &lo, &hi);
    if (got != 5 && got != 8) return 2;
    Q.lo = (T)lo; Q.hi = (T)hi;
    if (sequential) return run_sequential<T>(dt, Q, f0_given != 0, f0, t0, max_increases, sign);
    if (Q.cons) return 5;                                        // (the speculative drivers serve no constraint)
    return run<T>(dt, Q, f0_given != 0, f0, t0, max_increases, sign);
}

int main(int argc, char **argv) {
    const bool sequential = argc == 3 && !strcmp(argv[1], "--sequential");
    if (argc != 2 && !sequential) { fprintf(stderr, "usage: phi_search_table [--sequential] FILE\n"); return 1; }
    FILE *in = fopen(argv[argc - 1], "r");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[argc - 1]); return 1; }
    char line[1024];
    int rc = 0;
    while (!rc && fgets(line, sizeof line, in)) {
        int dt, kind, n, used = 0;
        if (sscanf(line, "%d %d %d%n", &dt, &kind, &n, &used) != 3) continue;
        if (n < 1 || n > kMaxN || kind < 0 || kind > 2) rc = 2;
        else rc = dt == kPhiF32 ? answer<float>(dt, kind, n, line + used, sequential) : answer<double>(dt, kind, n, line + used, sequential);
    }
    fclose(in);
    return rc;
}
