/* lj_saddle.c -- from a Markov chain to transition states, plain C against include/dzo.h: replicas of the 38-atom
 * Lennard-Jones cluster are tempered (scripts/MonteCarlo.jl:183-260), a copy of them is quenched by one batched LBFGSOptimizer
 * (src/DZOptimization.jl:321-509) until every instance is stuck, the minima are polished by eigenvector following of target
 * index 0 until the gradient is at rounding level, every polished minimum is displaced by 0.05 along its lowest non-zero
 * normal mode, and eigenvector following of target index 1 walks that mode uphill to a transition state.  Hessians,
 * eigenvalues, eigenvectors and steps stay on the device; the host reads the modes once, for the displacement.
 *
 *   gcc -O2 -Iinclude examples/lj_saddle.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_saddle && ./lj_saddle [num_steps [num_batches]]
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
#define N3 (3 * N)
#define REPLICAS 32
#define ZERO_TOL 1e-4
#define GRAD_TOL 1e-10
#define KICK 0.05

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

/* steps of a mode-following handle until no instance is ACTIVE, at most max_steps */
static int32_t follow(dzo_modefollow_batch_t h, int max_steps) {
    int32_t done = 0;
    for (int taken = 0; !done && taken < max_steps; taken += 10) {
        const int32_t rc = dzo_modefollow_batch_step(h, 10, &done);
        if (rc != DZO_OK) return rc;
    }
    return DZO_OK;
}

int main(int argc, char **argv) {
    const int64_t num_steps = argc > 1 ? atoll(argv[1]) : 500;
    const int64_t num_batches = argc > 2 ? atoll(argv[2]) : 4;
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 2.25;
    if (num_steps < 1 || num_batches < 1) { fprintf(stderr, "usage: lj_saddle [num_steps [num_batches]]\n"); return 2; }

    static double replicas[REPLICAS][N3];
    for (int k = 0; k < REPLICAS; ++k)
        for (int i = 0; i < N; ++i)
            for (;;) {
                const double x = normal(), y = normal(), z = normal();
                if (x * x + y * y + z * z < constraining_radius * constraining_radius) {
                    replicas[k][i] = x; replicas[k][N + i] = y; replicas[k][2 * N + i] = z;
                    break;
                }
            }
    double inv_temps[REPLICAS], radii[REPLICAS];
    for (int k = 0; k < REPLICAS; ++k) {
        inv_temps[k] = exp(-log(min_temp) + (-log(max_temp) + log(min_temp)) * (double)k / (double)(REPLICAS - 1));
        radii[k] = ldexp(1.0, -4);
    }

    CHECK(dzo_init(0));
    void *replicas_dev = NULL, *points_dev = NULL, *dirs_dev = NULL;
    CHECK(dzo_malloc(&replicas_dev, (int64_t)sizeof replicas));
    CHECK(dzo_malloc(&points_dev, (int64_t)sizeof replicas));
    CHECK(dzo_malloc(&dirs_dev, (int64_t)sizeof replicas));
    CHECK(dzo_memcpy_h2d(replicas_dev, replicas, (int64_t)sizeof replicas));

    /* temper; the chain keeps its own array, the rest works on a copy */
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, replicas_dev, inv_temps, radii, constraining_radius, 1, &pt));
    CHECK(dzo_tempering_run(pt, num_steps, num_batches, NULL, 0));
    CHECK(dzo_synchronize());
    CHECK(dzo_memcpy_d2d(points_dev, replicas_dev, (int64_t)sizeof replicas));
    CHECK(dzo_tempering_destroy(pt));

    /* quench until every instance is stuck */
    dzo_lbfgs_batch_t q = NULL;
    CHECK(dzo_lbfgs_batch_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, points_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    for (int launched = 0; !all_stuck && launched < 20000; launched += 50) CHECK(dzo_lbfgs_batch_step(q, 50, &all_stuck));
    CHECK(dzo_lbfgs_batch_destroy(q));

    /* polish: target index 0 */
    dzo_modefollow_batch_t polish = NULL;
    CHECK(dzo_modefollow_batch_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, points_dev, 0, 0.2, ZERO_TOL, GRAD_TOL, &polish));
    CHECK(follow(polish, 100));
    static double minimum_energy[REPLICAS], minimum_grms[REPLICAS], lam[REPLICAS][N3], points[REPLICAS][N3], dirs[REPLICAS][N3];
    static double modes[REPLICAS][N3][N3];                 /* [instance][mode][component] */
    static int32_t minimum_index[REPLICAS], minimum_status[REPLICAS];
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_ENERGIES, minimum_energy));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_GRMS, minimum_grms));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_INDEX, minimum_index));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_STATUS, minimum_status));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_EIGENVALUES, lam));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_EIGENVECTORS, modes));
    CHECK(dzo_modefollow_batch_read(polish, DZO_MODEFOLLOW_POINTS, points));
    CHECK(dzo_modefollow_batch_destroy(polish));

    /* the kick along the lowest non-zero mode, which is also the vector to follow */
    for (int k = 0; k < REPLICAS; ++k) {
        int m = 0;
        while (m < N3 - 1 && fabs(lam[k][m]) <= ZERO_TOL) ++m;
        for (int e = 0; e < N3; ++e) {
            dirs[k][e] = modes[k][m][e];
            points[k][e] += KICK * dirs[k][e];
        }
    }
    CHECK(dzo_memcpy_h2d(points_dev, points, (int64_t)sizeof points));
    CHECK(dzo_memcpy_h2d(dirs_dev, dirs, (int64_t)sizeof dirs));

    /* saddles: target index 1 */
    dzo_modefollow_batch_t saddle = NULL;
    CHECK(dzo_modefollow_batch_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, points_dev, 1, 0.1, ZERO_TOL, GRAD_TOL, &saddle));
    CHECK(dzo_modefollow_batch_set_directions(saddle, dirs_dev));
    CHECK(follow(saddle, 400));
    static double energy[REPLICAS], grms[REPLICAS];
    static int32_t index[REPLICAS], zeros[REPLICAS], status[REPLICAS];
    static int64_t iterations[REPLICAS];
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_ENERGIES, energy));
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_GRMS, grms));
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_INDEX, index));
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_ZEROS, zeros));
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_STATUS, status));
    CHECK(dzo_modefollow_batch_read(saddle, DZO_MODEFOLLOW_ITERATION_COUNTS, iterations));
    CHECK(dzo_modefollow_batch_destroy(saddle));

    int minima = 0, saddles = 0;
    printf("#        k      E(minimum)    grms   index      E(saddle)       grms  index zeros  steps   barrier\n");
    for (int k = 0; k < REPLICAS; ++k) {
        const int is_minimum = minimum_status[k] == DZO_MODEFOLLOW_CONVERGED && minimum_index[k] == 0;
        const int is_saddle = status[k] == DZO_MODEFOLLOW_CONVERGED && index[k] == 1 && zeros[k] == 6;
        minima += is_minimum;
        saddles += is_saddle;
        printf("instance %d %.9f %.2e %d   %.9f %.2e %d %d %lld %.6f %s\n", k, minimum_energy[k], minimum_grms[k], minimum_index[k], energy[k],
               grms[k], index[k], zeros[k], (long long)iterations[k], energy[k] - minimum_energy[k],
               is_saddle ? "transition state" : (status[k] == DZO_MODEFOLLOW_CONVERGED ? "another stationary point" : "not converged"));
    }
    printf("polished minima: %d of %d; index-1 saddles: %d of %d\n", minima, REPLICAS, saddles, REPLICAS);

    CHECK(dzo_free(dirs_dev));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_free(replicas_dev));
    CHECK(dzo_shutdown());
    if (minima == 0 || saddles == 0) { printf("FAILED: no polished minimum or no transition state\n"); return 1; }
    printf("OK\n");
    return 0;
}
