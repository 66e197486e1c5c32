/* lj_band.c -- the double-ended search: what joins minimum A to minimum B, and how high is the barrier.  Plain C against
 * include/dzo.h: REPLICAS random N-atom Lennard-Jones clusters (N = 13 by default) are tempered (scripts/MonteCarlo.jl),
 * relaxed by batched LBFGSOptimizers (src/DZOptimization.jl:321-509, step 0.01, history 10), kicked along their lowest mode and
 * followed uphill by hybrid eigenvector following (dzo_hybridef_batch_*): one saddle per replica.  Each saddle is displaced by
 * +-DISPLACEMENT along its mode and the two sides are quenched: its two minima, in one frame.  Then the saddles are forgotten:
 * a straight band of IMAGES images is strung between every pair of minima (dzo_neb_batch_interpolate) and relaxed by the nudged
 * elastic band with a climbing image (dzo_neb_batch_*), all bands in one handle, STEPS_PER_LAUNCH iterations per launch.  The
 * energy profile of every converged band is printed with its barrier from either end, next to the energy of the saddle the
 * pair came from.
 *
 *   gcc -O2 -Iinclude examples/lj_band.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_band && ./lj_band [n_particles [replicas]]
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
#define MAX_SEARCH_STEPS 600
#define MAX_BAND_ITERATIONS 20000
#define ZERO_TOL 1e-4
#define DISPLACEMENT 0.03
#define FORCE_TOL 1e-6

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
    if (n < 3 || n > DZO_NEB_MAX_PARTICLES || replicas < 2) {
        fprintf(stderr, "usage: lj_band [n_particles >= 3 [replicas >= 2]]\n");
        return 2;
    }
    const int n3 = 3 * n, ends = 2 * replicas;
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *e_top = malloc(sizeof(double) * replicas), *lowest = malloc(sizeof(double) * replicas),
           *e_scratch = malloc(sizeof(double) * 2 * ends), *profile = malloc(sizeof(double) * IMAGES * replicas),
           *residual = malloc(sizeof(double) * replicas);
    int32_t *status = malloc(sizeof(int32_t) * replicas), *stuck = malloc(sizeof(int32_t) * ends), *band_status = malloc(sizeof(int32_t) * replicas),
            *climbing = malloc(sizeof(int32_t) * replicas);
    int64_t *iterations = malloc(sizeof(int64_t) * replicas);
    if (!points || !inv_temps || !radii || !e_top || !lowest || !e_scratch || !profile || !residual || !status || !stuck || !band_status || !climbing ||
        !iterations) {
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
    const int64_t point_bytes = (int64_t)sizeof(double) * n3 * replicas;
    void *points_dev = NULL, *vectors_dev = NULL, *lowest_dev = NULL, *ends_dev = NULL, *band_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes));
    CHECK(dzo_malloc(&vectors_dev, point_bytes));
    CHECK(dzo_malloc(&lowest_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_malloc(&ends_dev, 2 * point_bytes));
    CHECK(dzo_malloc(&band_dev, IMAGES * point_bytes));
    CHECK(dzo_memcpy_h2d(points_dev, points, point_bytes));

    /* temper -> quench -> one saddle per replica */
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, 500, 20, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_tempering_destroy(pt));
    if (quench(points_dev, n, replicas, stuck, e_scratch, e_scratch + ends)) return 1;
    CHECK(dzo_pairwise_batch_lowest_mode(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, 1, DZO_LOWMODE_MAX_KRYLOV, 40, 1e-6, 7, NULL,
                                         lowest_dev, vectors_dev, NULL, NULL));
    CHECK(dzo_axpy((int64_t)n3 * replicas, DZO_F64, 0.05, vectors_dev, points_dev));   /* the kick */
    dzo_hybridef_batch_t search = NULL;                     /* aliases points_dev, copies vectors_dev */
    CHECK(dzo_hybridef_batch_create(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, vectors_dev, 0.1, 10, 2, 0.05, 0.01, 8, 1, 1e-3,
                                    ZERO_TOL, 1e-10, 7, &search));
    int32_t all_done = 0;
    for (int steps = 0; !all_done && steps < MAX_SEARCH_STEPS; steps += STEPS_PER_LAUNCH) CHECK(dzo_hybridef_batch_step(search, STEPS_PER_LAUNCH, &all_done));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_STATUS, status));
    CHECK(dzo_hybridef_batch_read(search, DZO_HYBRIDEF_EIGENVALUES, lowest));
    void *modes_dev = NULL;                                 /* the handle's: the mode of every search's last step */
    CHECK(dzo_hybridef_batch_get_ptr(search, DZO_HYBRIDEF_MODES, &modes_dev));

    /* its two minima: saddle +- DISPLACEMENT * mode, the + sides first, quenched in one handle */
    for (int side = 0; side < 2; ++side) {
        void *end = (char *)ends_dev + side * point_bytes;
        CHECK(dzo_memcpy_d2d(end, points_dev, point_bytes));
        CHECK(dzo_axpy((int64_t)n3 * replicas, DZO_F64, side ? -DISPLACEMENT : DISPLACEMENT, modes_dev, end));
    }
    CHECK(dzo_hybridef_batch_destroy(search));
    CHECK(dzo_pairwise_batch_energy_gradient(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, lowest_dev, NULL));
    CHECK(dzo_memcpy_d2h(e_top, lowest_dev, (int64_t)sizeof(double) * replicas));
    if (quench(ends_dev, n, ends, stuck, e_scratch, e_scratch + ends)) return 1;

    /* a band between every pair of minima: the quench moved both sides in the saddle's frame, so no alignment is needed */
    CHECK(dzo_neb_batch_interpolate(n, IMAGES, replicas, DZO_F64, ends_dev, (char *)ends_dev + point_bytes, band_dev));
    dzo_neb_batch_t band = NULL;                            /* aliases band_dev */
    CHECK(dzo_neb_batch_create(DZO_RADIAL_LENNARD_JONES, n, IMAGES, replicas, DZO_F64, band_dev, 1.0, 0.02, 0.1, FORCE_TOL, 1, 50, &band));
    all_done = 0;
    for (int it = 0; !all_done && it < MAX_BAND_ITERATIONS; it += BAND_STEPS_PER_LAUNCH) CHECK(dzo_neb_batch_step(band, BAND_STEPS_PER_LAUNCH, &all_done));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_STATUS, band_status));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_ENERGIES, profile));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_CLIMBING_IMAGES, climbing));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_RESIDUALS, residual));
    CHECK(dzo_neb_batch_read(band, DZO_NEB_ITERATION_COUNTS, iterations));
    CHECK(dzo_neb_batch_destroy(band));

    int good = 0;
    for (int k = 0; k < replicas; ++k) {
        const double *e = profile + (size_t)IMAGES * k;
        const int saddle_found = status[k] == DZO_HYBRIDEF_CONVERGED && lowest[k] < -ZERO_TOL;
        printf("band %d: %s after %lld iterations, residual %.2e; its pair came from %s\n", k,
               band_status[k] == DZO_NEB_CONVERGED ? "converged" : band_status[k] == DZO_NEB_FAILED ? "failed" : "still active",
               (long long)iterations[k], residual[k], saddle_found ? "a saddle" : "a search that found no saddle");
        printf("  profile");
        for (int m = 0; m < IMAGES; ++m) printf(" %.6f%s", e[m], m == climbing[k] ? "*" : "");
        printf("\n");
        if (band_status[k] != DZO_NEB_CONVERGED || climbing[k] < 1) continue;
        const double top = e[climbing[k]];
        printf("  barrier %.6f from image 0, %.6f from image %d; top %.9f, the saddle searched for %.9f\n", top - e[0], top - e[IMAGES - 1], IMAGES - 1, top,
               e_top[k]);
        if (saddle_found && top > e[0] && top > e[IMAGES - 1]) ++good;
    }
    printf("%d of %d bands converged on a barrier between their two minima\n", good, replicas);

    CHECK(dzo_free(band_dev)); CHECK(dzo_free(ends_dev)); CHECK(dzo_free(lowest_dev)); CHECK(dzo_free(vectors_dev)); CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(iterations); free(climbing); free(band_status); free(stuck); free(status); free(residual); free(profile); free(e_scratch); free(lowest);
    free(e_top); free(radii); free(inv_temps); free(points);
    if (good == 0) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
