/* lj_connect.c -- the first half of a connect cycle (Carr, Trygubenko & Wales 2005) in plain C against include/dzo.h:
 * band -> candidates -> refinement.  REPLICAS random N-atom Lennard-Jones clusters (N = 13 by default) are tempered
 * (scripts/MonteCarlo.jl) and relaxed by batched LBFGSOptimizers (src/DZOptimization.jl:321-509, step 0.01, history 10): a
 * handful of minima, in whatever frames they ended in.  Minimum k and minimum k + 1 make pair k.  Such a pair is usually several
 * elementary steps apart, so its band will not converge, and is not asked to: the second end is aligned onto the first
 * (dzo_align_batch_pairs), a straight band of IMAGES images is strung between them (dzo_neb_batch_interpolate) and iterated
 * BAND_ITERATIONS times (dzo_neb_batch_*), whatever its status.  Then every local maximum of every band's energy profile is taken
 * as a transition-state candidate with the band's tangent there (dzo_pathway_batch_candidates) and refined by hybrid eigenvector
 * following from that tangent (dzo_hybridef_batch_*).  The table has one line per candidate: its band, its image, its energy on
 * the band, and what the refinement made of it.  The rest of the cycle (which minima a saddle joins, the database, the choice
 * of the next pairs) is connect_pathways of the Python module.
 *
 *   gcc -O2 -Iinclude examples/lj_connect.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_connect && ./lj_connect [n_particles [replicas]]
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
#define BAND_ITERATIONS 600
#define BAND_STEPS_PER_LAUNCH 200
#define MAX_QUENCH_STEPS 20000
#define MAX_SEARCH_STEPS 600
#define ZERO_TOL 1e-4

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

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 13, replicas = argc > 2 ? atoi(argv[2]) : 8;
    if (n < 3 || n > DZO_PATHWAY_MAX_PARTICLES || replicas < 2) {
        fprintf(stderr, "usage: lj_connect [n_particles >= 3 [replicas >= 2]]\n");
        return 2;
    }
    const int n3 = 3 * n, pairs = replicas - 1, capacity = pairs * ((IMAGES - 1) / 2);   /* the most the bands can hold */
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *e_scratch = malloc(sizeof(double) * 2 * replicas),
           *profile = malloc(sizeof(double) * IMAGES * pairs), *distance = malloc(sizeof(double) * pairs),
           *cand_e = malloc(sizeof(double) * capacity), *refined_e = malloc(sizeof(double) * capacity),
           *lowest = malloc(sizeof(double) * capacity), *grms = malloc(sizeof(double) * capacity);
    int32_t *stuck = malloc(sizeof(int32_t) * replicas), *band_status = malloc(sizeof(int32_t) * pairs),
            *band_index = malloc(sizeof(int32_t) * capacity), *image_index = malloc(sizeof(int32_t) * capacity),
            *offsets = malloc(sizeof(int32_t) * (pairs + 1)), *status = malloc(sizeof(int32_t) * capacity);
    if (!points || !inv_temps || !radii || !e_scratch || !profile || !distance || !cand_e || !refined_e || !lowest || !grms || !stuck ||
        !band_status || !band_index || !image_index || !offsets || !status) {
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
    const int64_t point_bytes = (int64_t)sizeof(double) * n3, pair_bytes = point_bytes * pairs, cand_bytes = point_bytes * capacity;
    void *points_dev = NULL, *aligned_dev = NULL, *band_dev = NULL, *cand_dev = NULL, *tangent_dev = NULL, *cand_e_dev = NULL, *int_dev = NULL,
         *align_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes * replicas));
    CHECK(dzo_malloc(&aligned_dev, pair_bytes));
    CHECK(dzo_malloc(&band_dev, IMAGES * pair_bytes));
    CHECK(dzo_malloc(&cand_dev, cand_bytes));
    CHECK(dzo_malloc(&tangent_dev, cand_bytes));
    CHECK(dzo_malloc(&cand_e_dev, (int64_t)sizeof(double) * capacity));
    CHECK(dzo_malloc(&int_dev, (int64_t)sizeof(int32_t) * (2 * capacity + pairs + 1)));      /* band_index | image_index | offsets */
    /* the alignment's records: permutations, rotations, distances, best trial, cycles, status */
    const int64_t perm_bytes = ((int64_t)sizeof(int32_t) * n * pairs + 7) / 8 * 8;      /* the doubles behind them stay aligned */
    CHECK(dzo_malloc(&align_dev, perm_bytes + (int64_t)sizeof(double) * 10 * pairs + (int64_t)sizeof(int32_t) * 3 * pairs));
    CHECK(dzo_memcpy_h2d(points_dev, points, point_bytes * replicas));

    /* temper -> quench: the minima */
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, 500, 20, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_tempering_destroy(pt));
    if (quench(points_dev, n, replicas, stuck, e_scratch, e_scratch + replicas)) return 1;

    /* pair k: minimum k and minimum k + 1, the second one brought onto the first */
    void *second_dev = (char *)points_dev + point_bytes;
    double *rotation_dev = (double *)((char *)align_dev + perm_bytes), *distance_dev = rotation_dev + 9 * pairs;
    int32_t *best_dev = (int32_t *)(distance_dev + pairs), *cycles_dev = best_dev + pairs, *align_status_dev = cycles_dev + pairs;
    CHECK(dzo_align_batch_pairs(n, pairs, DZO_F64, points_dev, second_dev, DZO_ALIGN_TRIAL_IDENTITY | DZO_ALIGN_TRIAL_PRINCIPAL, 8, 20, 0, 1,
                                aligned_dev, (int32_t *)align_dev, rotation_dev, distance_dev, best_dev, cycles_dev, align_status_dev, NULL));
    CHECK(dzo_memcpy_d2h(distance, distance_dev, (int64_t)sizeof(double) * pairs));

    /* the bands: BAND_ITERATIONS iterations, converged or not (force_tol 0: none stops early) */
    CHECK(dzo_neb_batch_interpolate(n, IMAGES, pairs, DZO_F64, points_dev, aligned_dev, band_dev));
    dzo_neb_batch_t band = NULL;                            /* aliases band_dev */
    CHECK(dzo_neb_batch_create(DZO_RADIAL_LENNARD_JONES, n, IMAGES, pairs, DZO_F64, band_dev, 1.0, 0.02, 0.1, 0.0, 1, 50, &band));
    for (int it = 0; it < BAND_ITERATIONS; it += BAND_STEPS_PER_LAUNCH) CHECK(dzo_neb_batch_step(band, BAND_STEPS_PER_LAUNCH, NULL));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_STATUS, band_status));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_ENERGIES, profile));

    /* the candidates: every local maximum of every profile, with the band's tangent there.  The profile is the handle's record
     * (the band before the move of its last iteration); the images are the band's as it stands. */
    void *energies_dev = NULL;
    CHECK(dzo_neb_batch_get_ptr(band, DZO_NEB_ENERGIES, &energies_dev));
    int32_t *band_index_dev = (int32_t *)int_dev, *image_index_dev = band_index_dev + capacity, *offsets_dev = image_index_dev + capacity;
    int64_t count = 0;
    CHECK(dzo_pathway_batch_candidates(n, IMAGES, pairs, DZO_F64, band_dev, energies_dev, capacity, cand_dev, tangent_dev, cand_e_dev,
                                       band_index_dev, image_index_dev, offsets_dev, &count));
    CHECK(dzo_neb_batch_destroy(band));
    CHECK(dzo_memcpy_d2h(cand_e, cand_e_dev, (int64_t)sizeof(double) * capacity));
    CHECK(dzo_memcpy_d2h(band_index, band_index_dev, (int64_t)sizeof(int32_t) * capacity));
    CHECK(dzo_memcpy_d2h(image_index, image_index_dev, (int64_t)sizeof(int32_t) * capacity));
    CHECK(dzo_memcpy_d2h(offsets, offsets_dev, (int64_t)sizeof(int32_t) * (pairs + 1)));
    for (int k = 0; k < pairs; ++k) {
        const double *e = profile + (size_t)IMAGES * k;
        printf("band %d (minima %d and %d, %.4f apart once aligned): %s, %d candidates; profile", k, k, k + 1, distance[k],
               band_status[k] == DZO_NEB_FAILED ? "failed" : "still active", (int)(offsets[k + 1] - offsets[k]));
        for (int m = 0; m < IMAGES; ++m) printf(" %.4f", e[m]);
        printf("\n");
    }

    /* the refinement: hybrid eigenvector following from every candidate, its tangent as the first mode */
    int saddles = 0;
    if (count > 0) {
        dzo_hybridef_batch_t search = NULL;                 /* aliases cand_dev, copies tangent_dev */
        CHECK(dzo_hybridef_batch_create(DZO_RADIAL_LENNARD_JONES, n, count, DZO_F64, cand_dev, tangent_dev, 0.1, 10, 2, 0.05, 0.01, 8, 1, 1e-3,
                                        ZERO_TOL, 1e-10, 7, &search));
        int32_t all_done = 0;
        for (int steps = 0; !all_done && steps < MAX_SEARCH_STEPS; steps += STEPS_PER_LAUNCH) CHECK(dzo_hybridef_batch_step(search, STEPS_PER_LAUNCH, &all_done));
        CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_STATUS, status));
        CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_ENERGIES, refined_e));
        CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_EIGENVALUES, lowest));
        CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_GRMS, grms));
        CHECK(dzo_hybridef_batch_destroy(search));
        printf("candidate  band  image  E on the band    E refined      lowest mode   grms      result\n");
        for (int c = 0; c < count; ++c) {
            const int saddle = status[c] == DZO_HYBRIDEF_CONVERGED && lowest[c] < -ZERO_TOL;
            saddles += saddle;
            printf("%9d  %4d  %5d  %14.8f  %14.8f  %11.5f  %8.1e  %s\n", c, band_index[c], image_index[c], cand_e[c], refined_e[c], lowest[c], grms[c],
                   saddle ? "a saddle" : status[c] == DZO_HYBRIDEF_CONVERGED ? "stationary, no negative mode" : "not converged");
        }
    }
    printf("%lld candidates from %d bands, %d refined to a stationary point with a negative mode\n", (long long)count, pairs, saddles);

    CHECK(dzo_free(align_dev)); CHECK(dzo_free(int_dev)); CHECK(dzo_free(cand_e_dev)); CHECK(dzo_free(tangent_dev)); CHECK(dzo_free(cand_dev));
    CHECK(dzo_free(band_dev)); CHECK(dzo_free(aligned_dev)); CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(status); free(offsets); free(image_index); free(band_index); free(band_status); free(stuck); free(grms); free(lowest); free(refined_e);
    free(cand_e); free(distance); free(profile); free(e_scratch); free(radii); free(inv_temps); free(points);
    if (saddles == 0) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
