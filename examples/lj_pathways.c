/* lj_pathways.c -- from random clusters to a list of (minimum, saddle, minimum) triples with barrier heights, without leaving
 * the device for anything but the final table.  Plain C against include/dzo.h: REPLICAS random N-atom Lennard-Jones clusters
 * (N = 38 by default) are tempered (scripts/MonteCarlo.jl), relaxed by one batched LBFGSOptimizer
 * (src/DZOptimization.jl:321-509, step 0.01, history 10), asked for their lowest mode (dzo_pairwise_batch_lowest_mode),
 * displaced along it and followed uphill by hybrid eigenvector following (dzo_hybridef_batch_*).  Then the connection: every
 * search's end point is displaced by +-DISPLACEMENT along its mode, the 2 REPLICAS points are quenched together by batched
 * LBFGSOptimizers (restarted until none moves: quench() below says why), their fingerprints (dzo_structure_batch_fingerprint) are classified (dzo_structure_batch_classify), and the
 * labels say which two minima each transition state joins.
 *
 *   gcc -O2 -Iinclude examples/lj_pathways.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_pathways && ./lj_pathways [n_particles [replicas]]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
#define DISPLACEMENT 0.03      /* off the saddle's flat top; README.md, the structure block, has the sweep */
#define MATCH_TOL 1e-5         /* above what a stuck fp64 quench leaves between copies, far below two different minima */

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

/* Batched LBFGSOptimizers on `count` points until all are at rest.  "Stuck" alone does not say that: next to a saddle the
 * first pair (s, y) has s.y < 0, the L-BFGS direction points uphill and the backtracking search halves the step to nothing
 * on a slope.  So a fresh handle (empty history: a plain gradient step first) takes over until one leaves every energy as it
 * was, to the bit.  stuck[k] = instance k is stuck and at rest.  e and e_before: `count` doubles of scratch. */
static int quench(void *points_dev, int n, int count, int32_t *stuck, double *e, double *e_before) {
    int64_t launched = 0;
    for (int round = 0; launched < MAX_QUENCH_STEPS; ++round) {
        dzo_lbfgs_batch_t q = NULL;                         /* aliases points_dev */
        CHECK(dzo_lbfgs_batch_create(DZO_RADIAL_LENNARD_JONES, n, count, DZO_F64, points_dev, 0.01, 10, &q));
        int32_t all_stuck = 0;
        while (!all_stuck && launched < MAX_QUENCH_STEPS) {
            CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
            launched += STEPS_PER_LAUNCH;
        }
        CHECK(dzo_lbfgs_batch_read(q, DZO_LBFGS_BATCH_IS_STUCK, stuck));
        CHECK(dzo_lbfgs_batch_read(q, DZO_LBFGS_BATCH_OBJECTIVES, e));
        CHECK(dzo_lbfgs_batch_destroy(q));
        int moving = 0;
        for (int k = 0; k < count; ++k) {
            if (round == 0 || !stuck[k] || memcmp(&e[k], &e_before[k], sizeof(double)) != 0) { stuck[k] = 0; ++moving; }
            e_before[k] = e[k];
        }
        if (!moving) break;
    }
    return 0;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 38, replicas = argc > 2 ? atoi(argv[2]) : 16;
    if (n < 3 || n > DZO_STRUCTURE_MAX_PARTICLES || replicas < 2 || 2 * replicas > DZO_STRUCTURE_MAX_BATCH) {
        fprintf(stderr, "usage: lj_pathways [n_particles >= 3 [replicas >= 2]]\n");
        return 2;
    }
    const int n3 = 3 * n, ends = 2 * replicas;
    /* a sphere with room for n atoms at the density of a cluster */
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *e_top = malloc(sizeof(double) * replicas), *lowest = malloc(sizeof(double) * replicas),
           *e_end = malloc(sizeof(double) * ends), *e_scratch = malloc(sizeof(double) * ends);
    int32_t *status = malloc(sizeof(int32_t) * replicas), *stuck = malloc(sizeof(int32_t) * ends), *labels = malloc(sizeof(int32_t) * ends);
    if (!points || !inv_temps || !radii || !e_top || !lowest || !e_end || !e_scratch || !status || !stuck || !labels) { fprintf(stderr, "out of host memory\n"); return 1; }
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
    void *points_dev = NULL, *vectors_dev = NULL, *lowest_dev = NULL, *ends_dev = NULL, *prints_dev = NULL, *e_end_dev = NULL, *labels_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes));
    CHECK(dzo_malloc(&vectors_dev, point_bytes));
    CHECK(dzo_malloc(&lowest_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_malloc(&ends_dev, 2 * point_bytes));
    CHECK(dzo_malloc(&prints_dev, (int64_t)sizeof(double) * 2 * n * ends));
    CHECK(dzo_malloc(&e_end_dev, (int64_t)sizeof(double) * ends));
    CHECK(dzo_malloc(&labels_dev, (int64_t)sizeof(int32_t) * ends));
    CHECK(dzo_memcpy_h2d(points_dev, points, point_bytes));

    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, 500, 20, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_tempering_destroy(pt));
    if (quench(points_dev, n, replicas, stuck, e_end, e_scratch)) return 1;

    /* the lowest mode of every quenched replica, loosely: the search refines it at every step */
    CHECK(dzo_pairwise_batch_lowest_mode(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, 1, DZO_LOWMODE_MAX_KRYLOV, 40, 1e-6, 7, NULL,
                                         lowest_dev, vectors_dev, NULL, NULL));
    CHECK(dzo_axpy((int64_t)n3 * replicas, DZO_F64, 0.05, vectors_dev, points_dev));   /* the kick */
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
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_EIGENVALUES, lowest));
    void *modes_dev = NULL;                                 /* the handle's: the mode of every search's last step */
    CHECK(dzo_hybridef_batch_get_ptr(search, DZO_HYBRIDEF_MODES, &modes_dev));

    /* the connection: saddle +- DISPLACEMENT * mode, the + ends first, quenched in one handle */
    for (int side = 0; side < 2; ++side) {
        void *end = (char *)ends_dev + side * point_bytes;
        CHECK(dzo_memcpy_d2d(end, points_dev, point_bytes));
        CHECK(dzo_axpy((int64_t)n3 * replicas, DZO_F64, side ? -DISPLACEMENT : DISPLACEMENT, modes_dev, end));
    }
    CHECK(dzo_hybridef_batch_destroy(search));
    CHECK(dzo_pairwise_batch_energy_gradient(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, lowest_dev, NULL));
    CHECK(dzo_memcpy_d2h(e_top, lowest_dev, (int64_t)sizeof(double) * replicas));
    if (quench(ends_dev, n, ends, stuck, e_end, e_scratch)) return 1;
    CHECK(dzo_structure_batch_fingerprint(DZO_RADIAL_LENNARD_JONES, n, ends, DZO_F64, ends_dev, prints_dev, e_end_dev));
    for (int k = 0; k < ends; ++k)                          /* an end that is still moving names no minimum */
        if (!stuck[k]) CHECK(dzo_fill(1, DZO_F64, NAN, (char *)prints_dev + sizeof(double) * 2 * n * (size_t)k));
    int32_t n_minima = 0;
    CHECK(dzo_structure_batch_classify(2 * n, ends, DZO_F64, prints_dev, MATCH_TOL, labels_dev, &n_minima));
    CHECK(dzo_memcpy_d2h(labels, labels_dev, (int64_t)sizeof(int32_t) * ends));
    CHECK(dzo_memcpy_d2h(e_end, e_end_dev, (int64_t)sizeof(double) * ends));

    int triples = 0, degenerate = 0;
    printf("%d distinct minima below %d searches of %d atoms\n", n_minima, replicas, n);
    printf("%8s %14s %8s %14s %8s %14s %10s %10s\n", "minimum", "E", "saddle", "E", "minimum", "E", "barrier+", "barrier-");
    for (int k = 0; k < replicas; ++k) {
        if (status[k] != DZO_HYBRIDEF_CONVERGED || !(lowest[k] < -ZERO_TOL)) continue;   /* not a saddle */
        const int32_t a = labels[k], b = labels[replicas + k];
        if (a < 0 || b < 0) continue;                       /* an end did not arrive */
        ++triples;
        if (a == b) ++degenerate;
        printf("%8d %14.6f %8d %14.6f %8d %14.6f %10.6f %10.6f%s\n", a, e_end[a], k, e_top[k], b, e_end[b], e_top[k] - e_end[a], e_top[k] - e_end[b],
               a == b ? "  (both ends in one minimum)" : "");
    }
    printf("%d triples, %d of them with both ends in one minimum\n", triples, degenerate);

    CHECK(dzo_free(labels_dev)); CHECK(dzo_free(e_end_dev)); CHECK(dzo_free(prints_dev)); CHECK(dzo_free(ends_dev));
    CHECK(dzo_free(lowest_dev)); CHECK(dzo_free(vectors_dev)); CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(labels); free(stuck); free(status); free(e_scratch); free(e_end); free(lowest); free(e_top); free(radii); free(inv_temps); free(points);
    if (triples == 0) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
