/* thomson_quench.c -- the Thomson problem through the C ABI, plain C against include/dzo.h: 64 random configurations of 12 unit
 * charges are projected onto the unit sphere and quenched by one sphere-constrained batched LBFGSOptimizer (Riesz energy
 * sum 1 / r, step 0.01, history 10, 25 calls of step!() per launch) until every instance is stuck.  Prints the lowest and the
 * highest energy found and how many configurations reached the icosahedron, the minimum for 12 charges (49.16525305763).
 *
 *   gcc -O2 -Iinclude examples/thomson_quench.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o thomson_quench && ./thomson_quench
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

#define N 12
#define BATCH 64
#define STEPS_PER_LAUNCH 25
#define MAX_STEPS 5000
#define ICOSAHEDRON 49.16525305763
#define AT_ICOSAHEDRON 1e-9

static uint64_t lcg_state = 0x9E3779B97F4A7C16ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

int main(void) {
    /* instance k is [x | y | z]; every coordinate uniform in (-1, 1): the constructor projects each charge onto the sphere */
    static double points[BATCH][3][N], energies[BATCH];
    for (int k = 0; k < BATCH; ++k)
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < N; ++i) points[k][c][i] = 2.0 * uniform01() - 1.0;

    CHECK(dzo_init(0));
    void *points_dev = NULL, *e_dev = NULL;
    CHECK(dzo_malloc(&points_dev, (int64_t)sizeof points));
    CHECK(dzo_malloc(&e_dev, (int64_t)sizeof energies));
    CHECK(dzo_memcpy_h2d(points_dev, points, (int64_t)sizeof points));

    dzo_sphere_lbfgs_batch_t q = NULL;
    CHECK(dzo_sphere_lbfgs_batch_create(DZO_SPHERE_ENERGY_RIESZ1, N, BATCH, DZO_F64, points_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_sphere_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    CHECK(dzo_sphere_lbfgs_batch_read(q, DZO_LBFGS_BATCH_OBJECTIVES, energies));
    CHECK(dzo_sphere_lbfgs_batch_destroy(q));

    /* the points the handle left behind are on the sphere: projecting them again moves them by rounding only, and their energy,
     * evaluated apart from the optimizer, is the stored objective */
    CHECK(dzo_memcpy_d2h(points, points_dev, (int64_t)sizeof points));
    double off_sphere = 0.0;
    for (int k = 0; k < BATCH; ++k)
        for (int i = 0; i < N; ++i) {
            const double r2 = points[k][0][i] * points[k][0][i] + points[k][1][i] * points[k][1][i] + points[k][2][i] * points[k][2][i];
            if (!(fabs(r2 - 1.0) <= off_sphere)) off_sphere = fabs(r2 - 1.0);
        }
    static double again[BATCH];
    CHECK(dzo_sphere_batch_energy_gradient(DZO_SPHERE_ENERGY_RIESZ1, N, BATCH, DZO_F64, points_dev, e_dev, NULL, 1));
    CHECK(dzo_memcpy_d2h(again, e_dev, (int64_t)sizeof again));
    static double projected[BATCH][3][N];
    CHECK(dzo_sphere_batch_project(N, BATCH, DZO_F64, points_dev));
    CHECK(dzo_memcpy_d2h(projected, points_dev, (int64_t)sizeof projected));
    double moved = 0.0;
    for (int k = 0; k < BATCH; ++k)
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < N; ++i)
                if (!(fabs(projected[k][c][i] - points[k][c][i]) <= moved)) moved = fabs(projected[k][c][i] - points[k][c][i]);
    CHECK(dzo_free(e_dev));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());

    double lowest = energies[0], highest = energies[0];
    int reached = 0, differ = 0;
    for (int k = 0; k < BATCH; ++k) {
        if (energies[k] < lowest) lowest = energies[k];
        if (energies[k] > highest) highest = energies[k];
        if (fabs(energies[k] - ICOSAHEDRON) <= AT_ICOSAHEDRON) ++reached;
        if (again[k] != energies[k]) ++differ;
    }
    printf("lowest energy %.11f, highest energy %.11f, %d of %d at the icosahedron, %s after %lld steps per configuration\n", lowest, highest,
           reached, BATCH, all_stuck ? "all at rest" : "NOT all at rest", (long long)launched);
    if (!all_stuck) { printf("FAILED: configurations still moving after %d steps\n", MAX_STEPS); return 1; }
    if (!(off_sphere <= 2e-15)) { printf("FAILED: a charge is off the sphere by %.3e\n", off_sphere); return 1; }
    if (!(moved <= 1e-15)) { printf("FAILED: projecting the final points again moved a coordinate by %.3e\n", moved); return 1; }
    if (differ) { printf("FAILED: %d stored objectives are not the energies of the stored points\n", differ); return 1; }
    if (!(lowest >= ICOSAHEDRON - AT_ICOSAHEDRON)) { printf("FAILED: an energy below the icosahedron's\n"); return 1; }
    printf("OK\n");
    return 0;
}
