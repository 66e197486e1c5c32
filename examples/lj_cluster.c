/* lj_cluster.c -- relax a 38-atom Lennard-Jones cluster with L-BFGS on the device, plain C against include/dzo.h.
 *
 * What the reference is written for (src/ExampleFunctions.jl + src/DZOptimization.jl): the pairwise radial objective
 * with lj_energy / lj_first_derivative as a built-in problem (DZO_PROBLEM_PAIRWISE_LJ, point = [x | y | z]), and
 *
 *     opt = LBFGSOptimizer(nothing, f, g!, x0, 0.01, 10)
 *     while !opt.is_stuck[]; step!(opt); end
 *
 * Start: the truncated octahedron (the fcc fragment of 38 integer points with odd coordinate sum, |a| + |b| + |c| <= 3,
 * max <= 2, scaled to nearest-neighbour distance 1.09) with every coordinate jittered by +-0.05.  Its minimum is the
 * global minimum of LJ38, -173.928427 in the Cambridge Cluster Database.
 *
 *   gcc -O2 -Iinclude examples/lj_cluster.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_cluster && ./lj_cluster
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dzo.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int32_t rc_ = (call);                                                        \
        if (rc_ != DZO_OK) {                                                         \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dzo_last_error());   \
            return 1;                                                                \
        }                                                                            \
    } while (0)

#define N 38

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform_pm(double a) {                       /* uniform in (-a, a) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return a * (2.0 * (double)(lcg_state >> 11) / 9007199254740992.0 - 1.0);
}

int main(void) {
    double p[3 * N];
    int count = 0;
    const double scale = 1.09 / sqrt(2.0);
    for (int a = -3; a <= 3; ++a)
        for (int b = -3; b <= 3; ++b)
            for (int c = -3; c <= 3; ++c) {
                const int m = abs(a) > abs(b) ? (abs(a) > abs(c) ? abs(a) : abs(c)) : (abs(b) > abs(c) ? abs(b) : abs(c));
                if (((a + b + c) & 1) == 0 || abs(a) + abs(b) + abs(c) > 3 || m > 2) continue;
                if (count == N) { fprintf(stderr, "more than %d lattice points\n", N); return 2; }
                p[count] = scale * a + uniform_pm(0.05);
                p[N + count] = scale * b + uniform_pm(0.05);
                p[2 * N + count] = scale * c + uniform_pm(0.05);
                ++count;
            }
    if (count != N) { fprintf(stderr, "%d lattice points, expected %d\n", count, N); return 2; }

    CHECK(dzo_init(0));
    void *x_dev = NULL;
    CHECK(dzo_malloc(&x_dev, (int64_t)sizeof p));
    CHECK(dzo_memcpy_h2d(x_dev, p, (int64_t)sizeof p));

    /* the handle-less form of the same objective: accelerated_pairwise_radial_energy(lj_energy, x, y, z) */
    double e0 = 0;
    CHECK(dzo_pairwise_energy(DZO_RADIAL_LENNARD_JONES, N, DZO_F64, x_dev, (const double *)x_dev + N, (const double *)x_dev + 2 * N, &e0));

    dzo_problem_t prob = NULL;
    CHECK(dzo_problem_create(DZO_PROBLEM_PAIRWISE_LJ, 3 * N, DZO_F64, NULL, NULL, 0.0, &prob));
    dzo_lbfgs_t opt = NULL;
    CHECK(dzo_lbfgs_create_problem(prob, 10, x_dev, 0.01, &opt));   /* aliases x_dev as current_point */
    int64_t stuck = 0, iters = 0;
    while (!stuck && iters < 20000) {
        CHECK(dzo_lbfgs_step(opt));
        CHECK(dzo_lbfgs_get_i(opt, 0, &stuck));                     /* opt.is_stuck[] */
        ++iters;
    }
    double f = 0;
    CHECK(dzo_lbfgs_get_s(opt, 0, &f));                             /* opt.current_objective_value[] */
    printf("LJ38 truncated octahedron, jitter 0.05: E = %.9f -> %.9f after %lld L-BFGS steps (is_stuck = %lld)\n", e0, f,
           (long long)iters, (long long)stuck);
    CHECK(dzo_lbfgs_destroy(opt));
    CHECK(dzo_problem_destroy(prob));
    CHECK(dzo_free(x_dev));
    CHECK(dzo_shutdown());
    if (!(fabs(f - (-173.928427)) <= 5e-7)) { fprintf(stderr, "FAILED: expected -173.928427\n"); return 3; }
    printf("OK\n");
    return 0;
}
