/* lj_lowest_mode.c -- temper, quench, and ask every replica "is this a minimum, and if not, which way is down?" without a
 * dense Hessian.  Plain C against include/dzo.h: REPLICAS random N-atom Lennard-Jones clusters are tempered
 * (scripts/MonteCarlo.jl), relaxed by one batched LBFGSOptimizer (src/DZOptimization.jl:321-509, step 0.01, history 10), and
 * dzo_pairwise_batch_lowest_mode finds the lowest eigenpair of every Hessian with the rigid-body motions projected out, by
 * restarted Lanczos on Hessian-vector products inside one launch.  It prints how many replicas are minima.  With N = 38 (the
 * default) the dense route still exists: the largest difference from eigenvalue 6 of dzo_symmetric_batch_eigen (the lowest
 * vibration, after the six rigid-body zeros) over the replicas that are minima is printed as well.  N up to 1024 works; the dense route stops at 128.
 *
 *   gcc -O2 -Iinclude examples/lj_lowest_mode.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_lowest_mode && ./lj_lowest_mode [n_particles [replicas]]
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
#define MAX_STEPS 20000

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 38, replicas = argc > 2 ? atoi(argv[2]) : 64;
    if (n < 3 || n > DZO_LOWMODE_MAX_PARTICLES || replicas < 2) { fprintf(stderr, "usage: lj_lowest_mode [n_particles >= 3 [replicas >= 2]]\n"); return 2; }
    const int n3 = 3 * n;
    /* a sphere with room for n atoms at the density of a cluster */
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 0.75 * cbrt((double)n) + 0.5;
    double *points = malloc(sizeof(double) * (size_t)n3 * replicas), *inv_temps = malloc(sizeof(double) * replicas),
           *radii = malloc(sizeof(double) * replicas), *lowest = malloc(sizeof(double) * replicas), *residuals = malloc(sizeof(double) * replicas);
    int32_t *info = malloc(sizeof(int32_t) * 3 * replicas);
    if (!points || !inv_temps || !radii || !lowest || !residuals || !info) { fprintf(stderr, "out of host memory\n"); return 1; }
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
    void *points_dev = NULL, *lowest_dev = NULL, *vectors_dev = NULL, *residuals_dev = NULL, *info_dev = NULL;
    CHECK(dzo_malloc(&points_dev, point_bytes));
    CHECK(dzo_malloc(&vectors_dev, point_bytes));
    CHECK(dzo_malloc(&lowest_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_malloc(&residuals_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_malloc(&info_dev, (int64_t)sizeof(int32_t) * 3 * replicas));
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
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    CHECK(dzo_lbfgs_batch_destroy(q));

    /* the lowest mode of every quenched replica: 32 Lanczos vectors per cycle, relative residual 1e-8, starts drawn in the kernel */
    CHECK(dzo_pairwise_batch_lowest_mode(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, 1, DZO_LOWMODE_MAX_KRYLOV, 100, 1e-8, 7, NULL,
                                         lowest_dev, vectors_dev, (double *)residuals_dev, (int32_t *)info_dev));
    CHECK(dzo_memcpy_d2h(lowest, lowest_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_memcpy_d2h(residuals, residuals_dev, (int64_t)sizeof(double) * replicas));
    CHECK(dzo_memcpy_d2h(info, info_dev, (int64_t)sizeof(int32_t) * 3 * replicas));
    int minima = 0, converged = 0;
    int64_t products = 0;
    double worst = 0;
    for (int k = 0; k < replicas; ++k) {
        if (info[3 * k] == DZO_LOWMODE_CONVERGED) ++converged;
        if (info[3 * k] == DZO_LOWMODE_CONVERGED && lowest[k] > 0) ++minima;
        products += info[3 * k + 2];
        if (residuals[k] > worst) worst = residuals[k];
    }
    printf("%d replicas of %d atoms: %d converged, %d are minima (lowest vibration > 0), %.1f products per replica, largest residual %.2e\n",
           replicas, n, converged, minima, (double)products / replicas, worst);
    int ok = converged == replicas;

    if (n == 38) {                                          /* the dense route, for comparison */
        void *hessians_dev = NULL, *spectrum_dev = NULL;
        double *spectrum = malloc(sizeof(double) * (size_t)n3 * replicas);
        if (!spectrum) { fprintf(stderr, "out of host memory\n"); return 1; }
        CHECK(dzo_malloc(&hessians_dev, (int64_t)sizeof(double) * n3 * n3 * replicas));
        CHECK(dzo_malloc(&spectrum_dev, point_bytes));
        CHECK(dzo_pairwise_batch_hessian(DZO_RADIAL_LENNARD_JONES, n, replicas, DZO_F64, points_dev, hessians_dev));
        CHECK(dzo_symmetric_batch_eigen(n3, replicas, DZO_F64, hessians_dev, spectrum_dev, NULL, NULL, 0));
        CHECK(dzo_memcpy_d2h(spectrum, spectrum_dev, point_bytes));
        /* where the dense spectrum says "minimum" (nothing below the six rigid-body zeros), eigenvalue 6 is the lowest vibration */
        double diff = 0;
        int compared = 0;
        for (int k = 0; k < replicas; ++k) {
            const double *ev = spectrum + (size_t)k * n3;
            if (ev[0] < -1e-5 * ev[n3 - 1]) continue;
            const double d = fabs(lowest[k] - ev[6]);
            if (d > diff) diff = d;
            ++compared;
        }
        printf("largest difference from eigenvalue 6 of dzo_symmetric_batch_eigen over the %d minima of the dense spectrum: %.3e\n", compared, diff);
        CHECK(dzo_free(spectrum_dev));
        CHECK(dzo_free(hessians_dev));
        free(spectrum);
    }

    CHECK(dzo_free(info_dev));
    CHECK(dzo_free(residuals_dev));
    CHECK(dzo_free(lowest_dev));
    CHECK(dzo_free(vectors_dev));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    free(info); free(residuals); free(lowest); free(radii); free(inv_temps); free(points);
    if (!ok) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
