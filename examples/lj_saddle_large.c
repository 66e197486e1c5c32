/* lj_saddle_large.c -- temper, quench, and search a transition state from every replica of a cluster too large for a dense
 * Hessian on the device.  Plain C against include/dzo.h: REPLICAS random N-atom Lennard-Jones clusters (N = 150 by default;
 * the dense search of examples/lj_saddle.c stops at 128) are tempered (scripts/MonteCarlo.jl), relaxed by one batched
 * LBFGSOptimizer (src/DZOptimization.jl:321-509, step 0.01, history 10), and asked for their lowest mode
 * (dzo_pairwise_batch_lowest_mode).  Every replica is then displaced by 0.05 along that mode and followed uphill by hybrid
 * eigenvector following (dzo_hybridef_batch_*): Hessian-vector products and gradients only.  It prints, for every search that
 * ended on a stationary point with a negative lowest eigenvalue, the barrier above the quenched replica.  (A barrier can be
 * negative: a search may cross into a lower basin and end on a saddle below its start.)
 *
 *   gcc -O2 -Iinclude examples/lj_saddle_large.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_saddle_large && ./lj_saddle_large [n_particles [replicas]]
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

#define STEPS_PER_LAUNCH 50
#define MAX_QUENCH_STEPS 20000
#define MAX_SEARCH_STEPS 600
#define ZERO_TOL 1e-4

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 150, replicas = argc > 2 ? atoi(argv[2]) : 8;
    if (n < 3 || n > DZO_HYBRIDEF_MAX_PARTICLES || replicas < 2) { fprintf(stderr, "usage: lj_saddle_large [n_particles >= 3 [replicas >= 2]]\n"); return 2; }
    const int n3 = 3 * n;
    /* a sphere with room for n atoms at the density of a cluster */
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *e_min = malloc(sizeof(double) * replicas), *e_top = malloc(sizeof(double) * replicas),
           *lowest = malloc(sizeof(double) * replicas);
    int32_t *status = malloc(sizeof(int32_t) * replicas);
    int64_t *counts = malloc(sizeof(int64_t) * 3 * replicas);
    if (!points || !inv_temps || !radii || !e_min || !e_top || !lowest || !status || !counts) { fprintf(stderr, "out of host memory\n"); return 1; }
    for (int k = 0; k < replicas; ++k) {
        for (int i = 0; i < n; ++i)
            for (;;) {
                const double s = 0.5 * constraining_radius, x = s * normal(), y = s * normal(), z = s * normal();
                if (x * x + y * y + z * z < constraining_radius * constraining_radius) {
                    points[(size_t)k * n3 + i] = x; points[(size_t)k * n3 + n + i] = y; points[(size_t)k * n3 + 2 * n + i] = z;
                    break;
                }
            }
        inv_temps[k] = exp(-log(min_temp) + (-log(max_temp) + log(min_temp)) * (double)k / (double)(replicas - 1));
        radii[k] = 0.05;
    }

    CHECK(dzo_init(0));
    const int64_t point_bytes = (int64_t)sizeof(double) * n3 * replicas;
    void *points_dev = NULL, *vectors_dev = NULL, *lowest_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes));
    CHECK(dzo_malloc(&vectors_dev, point_bytes));
    CHECK(dzo_malloc(&lowest_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_memcpy_h2d(points_dev, points, point_bytes));

    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, 500, 20, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_tempering_destroy(pt));

    dzo_lbfgs_batch_t q = NULL;                             /* aliases points_dev */
    CHECK(dzo_lbfgs_batch_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_QUENCH_STEPS) {
        CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    CHECK(dzo_lbfgs_batch_read(q, DZO_LBFGS_BATCH_OBJECTIVES, e_min));
    CHECK(dzo_lbfgs_batch_destroy(q));

    /* the lowest mode of every quenched replica, loosely: the search refines it at every step */
    CHECK(dzo_pairwise_batch_lowest_mode(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, 1, DZO_LOWMODE_MAX_KRYLOV, 40, 1e-6, 7, NULL,
                                         lowest_dev, vectors_dev, NULL, NULL));
    CHECK(dzo_axpy((int64_t)n3 * replicas, DZO_F64, 0.05, vectors_dev, points_dev));   /* the kick */

    /* uphill steps of at most 0.1; 10 tangent steps (2 while the mode is still convex), capped at 0.05, the first 0.01 long;
     * 8 Lanczos vectors and one refinement cycle per step, left early at a relative residual of 1e-3 */
    dzo_hybridef_batch_t search = NULL;                     /* aliases points_dev, copies vectors_dev */
    CHECK(dzo_hybridef_batch_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, vectors_dev, 0.1, 10, 2, 0.05, 0.01, 8, 1, 1e-3,
                                    ZERO_TOL, 1e-10, 7, &search));
    int32_t all_done = 0;
    int steps = 0;
    while (!all_done && steps < MAX_SEARCH_STEPS) {
        CHECK(dzo_hybridef_batch_step(search, STEPS_PER_LAUNCH, &all_done));
        steps += STEPS_PER_LAUNCH;
    }
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_STATUS, status));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_ENERGIES, e_top));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_EIGENVALUES, lowest));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_ITERATION_COUNTS, counts));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_PRODUCTS, counts + replicas));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_EVALUATIONS, counts + 2 * replicas));
    CHECK(dzo_hybridef_batch_destroy(search));

    int saddles = 0, failed = 0;
    for (int k = 0; k < replicas; ++k) {
        if (status[k] == DZO_HYBRIDEF_FAILED) ++failed;
        if (status[k] != DZO_HYBRIDEF_CONVERGED || !(lowest[k] < -ZERO_TOL)) continue;
        ++saddles;
        printf("replica %d: saddle at E = %.6f, barrier %.6f above its quenched start, lowest eigenvalue %.4f, %lld steps, %lld products, %lld gradients\n",
               k, e_top[k], e_top[k] - e_min[k], lowest[k], (long long)counts[k], (long long)counts[replicas + k], (long long)counts[2 * replicas + k]);
    }
    printf("%d replicas of %d atoms: %d searches ended on a saddle within %d steps, %d failed\n", replicas, n, saddles, steps, failed);

    CHECK(dzo_free(lowest_dev));
    CHECK(dzo_free(vectors_dev));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(counts); free(status); free(lowest); free(e_top); free(e_min); free(radii); free(inv_temps); free(points);
    if (saddles == 0 || failed > 0) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
