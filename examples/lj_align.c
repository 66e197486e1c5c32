/* lj_align.c -- a band between two minima that nothing relates: what the double-ended search needs the alignment for.  Plain C
 * against include/dzo.h: REPLICAS random N-atom Lennard-Jones clusters (N = 13 by default) are tempered (scripts/MonteCarlo.jl)
 * and relaxed by batched LBFGSOptimizers (src/DZOptimization.jl:321-509, step 0.01, history 10): one minimum per replica, each
 * in the frame and with the particle labels its own walk left it.  Replica k is paired with replica k + 1.  Every pair is
 * aligned (dzo_align_batch_pairs: the identity, the four principal-axis starts and RANDOM_TRIALS random ones, each alternating
 * the optimal assignment of the particles with the best rotation), a straight band of IMAGES images is strung between a and
 * the aligned b (dzo_neb_batch_interpolate) and relaxed by the nudged elastic band with a climbing image (dzo_neb_batch_*).
 * Per pair it prints the distance of the centred points as they came, the aligned distance, and how the band ended with its
 * barrier from either end.
 *
 *   gcc -O2 -Iinclude examples/lj_align.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_align && ./lj_align [n_particles [replicas]]
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

#define IMAGES 9
#define STEPS_PER_LAUNCH 50
#define BAND_STEPS_PER_LAUNCH 200
#define MAX_QUENCH_STEPS 20000
#define MAX_BAND_ITERATIONS 20000
#define FORCE_TOL 1e-6
#define RANDOM_TRIALS 8
#define MAX_CYCLES 20

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

/* Batched LBFGSOptimizers on `count` points until all are at rest: a fresh handle takes over until one leaves every energy
 * as it was, to the bit (examples/lj_pathways.c says why).  e and e_before: `count` doubles of scratch. */
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

/* the distance of two points of n particles with their centroids removed, labels as they are */
static double centred_distance(const double *a, const double *b, int n) {
    double d2 = 0;
    for (int c = 0; c < 3; ++c) {
        double ca = 0, cb = 0;
        for (int i = 0; i < n; ++i) { ca += a[c * n + i]; cb += b[c * n + i]; }
        ca /= n; cb /= n;
        for (int i = 0; i < n; ++i) { const double d = (a[c * n + i] - ca) - (b[c * n + i] - cb); d2 += d * d; }
    }
    return sqrt(d2);
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 13, replicas = argc > 2 ? atoi(argv[2]) : 8;
    if (n < 3 || n > DZO_ALIGN_MAX_PARTICLES || replicas < 2) {
        fprintf(stderr, "usage: lj_align [n_particles >= 3 [replicas >= 2]]\n");
        return 2;
    }
    const int n3 = 3 * n, pairs = replicas - 1;
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *e_scratch = malloc(sizeof(double) * 2 * replicas),
           *distance = malloc(sizeof(double) * pairs), *profile = malloc(sizeof(double) * IMAGES * pairs), *residual = malloc(sizeof(double) * pairs);
    int32_t *stuck = malloc(sizeof(int32_t) * replicas), *align_status = malloc(sizeof(int32_t) * pairs), *best = malloc(sizeof(int32_t) * pairs),
            *cycles = malloc(sizeof(int32_t) * pairs), *band_status = malloc(sizeof(int32_t) * pairs), *climbing = malloc(sizeof(int32_t) * pairs);
    int64_t *iterations = malloc(sizeof(int64_t) * pairs);
    if (!points || !inv_temps || !radii || !e_scratch || !distance || !profile || !residual || !stuck || !align_status || !best || !cycles || !band_status ||
        !climbing || !iterations) {
        fprintf(stderr, "out of host memory\n");
        return 1;
    }
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
    const int64_t point_bytes = (int64_t)sizeof(double) * n3 * replicas, pair_bytes = (int64_t)sizeof(double) * n3 * pairs;
    void *points_dev = NULL, *aligned_dev = NULL, *band_dev = NULL, *perm_dev = NULL, *rotation_dev = NULL, *distance_dev = NULL, *int_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes));
    CHECK(dzo_malloc(&aligned_dev, pair_bytes));
    CHECK(dzo_malloc(&band_dev, IMAGES * pair_bytes));
    CHECK(dzo_malloc(&perm_dev, (int64_t)sizeof(int32_t) * n * pairs));
    CHECK(dzo_malloc(&rotation_dev, (int64_t)sizeof(double) * 9 * pairs));
    CHECK(dzo_malloc(&distance_dev, (int64_t)sizeof(double) * pairs));
    CHECK(dzo_malloc(&int_dev, (int64_t)sizeof(int32_t) * 3 * pairs));
    CHECK(dzo_memcpy_h2d(points_dev, points, point_bytes));

    /* 1. temper, 2. quench: one minimum per replica */
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, 500, 20, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_tempering_destroy(pt));
    if (quench(points_dev, n, replicas, stuck, e_scratch, e_scratch + replicas)) return 1;
    CHECK(dzo_memcpy_d2h(points, points_dev, point_bytes));

    /* 3. pair replica k with replica k + 1: a = points[0 .. pairs), b = points[1 .. pairs]; 4. align */
    const void *a_dev = points_dev, *b_dev = (const char *)points_dev + sizeof(double) * n3;
    int32_t *best_dev = int_dev, *cycles_dev = best_dev + pairs, *status_dev = cycles_dev + pairs;
    CHECK(dzo_align_batch_pairs(n, pairs, DZO_F64, a_dev, b_dev, DZO_ALIGN_TRIAL_IDENTITY | DZO_ALIGN_TRIAL_PRINCIPAL, RANDOM_TRIALS, MAX_CYCLES, 0, 1,
                                aligned_dev, perm_dev, rotation_dev, distance_dev, best_dev, cycles_dev, status_dev, NULL));
    CHECK(dzo_memcpy_d2h(distance, distance_dev, (int64_t)sizeof(double) * pairs));
    CHECK(dzo_memcpy_d2h(best, best_dev, (int64_t)sizeof(int32_t) * pairs));
    CHECK(dzo_memcpy_d2h(cycles, cycles_dev, (int64_t)sizeof(int32_t) * pairs));
    CHECK(dzo_memcpy_d2h(align_status, status_dev, (int64_t)sizeof(int32_t) * pairs));

    /* 5. a band between a and the aligned b */
    CHECK(dzo_neb_batch_interpolate(n, IMAGES, pairs, DZO_F64, a_dev, aligned_dev, band_dev));
    dzo_neb_batch_t band = NULL;                            /* aliases band_dev */
    CHECK(dzo_neb_batch_create(DZO_RADIAL_LENNARD_JONES, n, IMAGES, pairs, DZO_F64, band_dev, 1.0, 0.02, 0.1, FORCE_TOL, 1, 50, &band));
    int32_t all_done = 0;
    for (int it = 0; !all_done && it < MAX_BAND_ITERATIONS; it += BAND_STEPS_PER_LAUNCH) CHECK(dzo_neb_batch_step(band, BAND_STEPS_PER_LAUNCH, &all_done));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_STATUS, band_status));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_ENERGIES, profile));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_CLIMBING_IMAGES, climbing));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_RESIDUALS, residual));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_ITERATION_COUNTS, iterations));
    CHECK(dzo_neb_batch_destroy(band));

    /* 6. the barrier of every pair */
    int shorter = 0, aligned_ok = 0;
    for (int k = 0; k < pairs; ++k) {
        const double *e = profile + (size_t)IMAGES * k;
        const double raw = centred_distance(points + (size_t)k * n3, points + (size_t)(k + 1) * n3, n);
        printf("pair %d: raw centred distance %.6f, aligned distance %.6f (start %d, %d cycles, %s); band %s after %lld iterations, residual %.2e\n", k,
               raw, distance[k], best[k], cycles[k],
               align_status[k] == DZO_ALIGN_CONVERGED ? "converged" : align_status[k] == DZO_ALIGN_CYCLE_LIMIT ? "cycle limit" : "failed",
               band_status[k] == DZO_NEB_CONVERGED ? "converged" : band_status[k] == DZO_NEB_FAILED ? "failed" : "still active", (long long)iterations[k],
               residual[k]);
        if (align_status[k] != DZO_ALIGN_FAILED) ++aligned_ok;
        if (distance[k] <= raw * (1.0 + 1e-12)) ++shorter;   /* the identity start cannot do worse than the labels as they came */
        if (band_status[k] == DZO_NEB_CONVERGED && climbing[k] >= 1) {
            const double top = e[climbing[k]];
            printf("  barrier %.6f from image 0, %.6f from image %d\n", top - e[0], top - e[IMAGES - 1], IMAGES - 1);
        }
    }
    printf("%d of %d pairs aligned, %d no farther apart than they came\n", aligned_ok, pairs, shorter);

    CHECK(dzo_free(int_dev)); CHECK(dzo_free(distance_dev)); CHECK(dzo_free(rotation_dev)); CHECK(dzo_free(perm_dev)); CHECK(dzo_free(band_dev));
    CHECK(dzo_free(aligned_dev)); CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(iterations); free(climbing); free(band_status); free(cycles); free(best); free(align_status); free(stuck); free(residual); free(profile);
    free(distance); free(e_scratch); free(radii); free(inv_temps); free(points);
    if (aligned_ok != pairs || shorter != pairs) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
