/* lj_adgd_quench.c -- the counterpart of examples/lj_quench.c with the second live optimizer, plain C against include/dzo.h:
 * 256 replicas of the 38-atom Lennard-Jones cluster are tempered as in examples/lj_tempering.c (the `main` of
 * scripts/MonteCarlo.jl:183-260), then a COPY of all of them is quenched to local minima by one batched AdGDOptimizer
 * (src/DZOptimization.jl:179-312, step 0.01): every launch runs 50 calls of step!() of every replica, until all are stuck.  The
 * Markov chain's own array is not touched.
 *
 *   gcc -O2 -Iinclude examples/lj_adgd_quench.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_adgd_quench && ./lj_adgd_quench [num_steps [num_batches [radius]]]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

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
#define REPLICAS 256
#define STEPS_PER_LAUNCH 50
#define MAX_STEPS 200000
#define LJ38 (-173.928427)

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal(void) { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int by_value(const void *a, const void *b) {
    const double x = *(const double *)a, y = *(const double *)b;
    return x < y ? -1 : x > y ? 1 : 0;
}

int main(int argc, char **argv) {
    const int64_t num_steps = argc > 1 ? atoll(argv[1]) : 500;
    const int64_t num_batches = argc > 2 ? atoll(argv[2]) : 20;
    const double radius0 = argc > 3 ? atof(argv[3]) : 0.05;
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 2.25;
    if (num_steps < 1 || num_batches < 1 || !(radius0 > 0.0)) { fprintf(stderr, "usage: lj_adgd_quench [num_steps [num_batches [radius]]]\n"); return 2; }

    static double replicas[REPLICAS][3][N];
    for (int k = 0; k < REPLICAS; ++k)
        for (int i = 0; i < N; ++i)
            for (;;) {
                const double x = normal(), y = normal(), z = normal();
                if (x * x + y * y + z * z < constraining_radius * constraining_radius) {
                    replicas[k][0][i] = x; replicas[k][1][i] = y; replicas[k][2][i] = z;
                    break;
                }
            }
    double inv_temps[REPLICAS], radii[REPLICAS];
    for (int k = 0; k < REPLICAS; ++k) {
        inv_temps[k] = exp(-log(min_temp) + (-log(max_temp) + log(min_temp)) * (double)k / (double)(REPLICAS - 1));
        radii[k] = radius0;
    }

    CHECK(dzo_init(0));
    void *replicas_dev = NULL, *minima_dev = NULL;
    CHECK(dzo_malloc(&replicas_dev, (int64_t)sizeof replicas));
    CHECK(dzo_malloc(&minima_dev, (int64_t)sizeof replicas));
    CHECK(dzo_memcpy_h2d(replicas_dev, replicas, (int64_t)sizeof replicas));
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, replicas_dev, inv_temps, radii, constraining_radius, 1,
                               &pt));
    CHECK(dzo_tempering_run(pt, num_steps, num_batches, NULL, 0));

    /* the quench works on a copy: dzo_memcpy_d2d waits for the tempering first */
    CHECK(dzo_memcpy_d2d(minima_dev, replicas_dev, (int64_t)sizeof replicas));
    const double start = now();
    dzo_adgd_batch_t q = NULL;
    CHECK(dzo_adgd_batch_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, minima_dev, 0.01, &q));
    static double before[REPLICAS], after[REPLICAS];
    CHECK(dzo_adgd_batch_read(q, DZO_ADGD_BATCH_OBJECTIVES, before));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_adgd_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    const double duration = now() - start;
    static int64_t counts[REPLICAS];
    CHECK(dzo_adgd_batch_read(q, DZO_ADGD_BATCH_OBJECTIVES, after));
    CHECK(dzo_adgd_batch_read(q, DZO_ADGD_BATCH_ITERATION_COUNTS, counts));
    int64_t active = 0;
    CHECK(dzo_adgd_batch_count_active(q, &active));

    int ok = 1;
    int64_t total = 0, most = 0, least = counts[0];
    for (int k = 0; k < REPLICAS; ++k) {
        if (!(after[k] <= before[k]) || !isfinite(after[k])) ok = 0;
        total += counts[k];
        if (counts[k] > most) most = counts[k];
        if (counts[k] < least) least = counts[k];
    }
    static double sorted[REPLICAS];
    for (int k = 0; k < REPLICAS; ++k) sorted[k] = after[k];
    qsort(sorted, REPLICAS, sizeof(double), by_value);
    int distinct = 1;
    for (int k = 1; k < REPLICAS; ++k)
        if (sorted[k] - sorted[k - 1] > 1e-6) ++distinct;
    printf("lowest minimum: %.6f (literature %.6f)\n", sorted[0], LJ38);
    printf("highest minimum: %.6f\n", sorted[REPLICAS - 1]);
    printf("distinct minima: %d of %d\n", distinct, REPLICAS);
    printf("steps per replica: min %lld, mean %.1f, max %lld; %lld steps per replica launched\n", (long long)least,
           (double)total / REPLICAS, (long long)most, (long long)launched);
    printf("instances not stuck: %lld\n", (long long)active);
    printf("quench: %.3f ms, %.6e step!() calls per second\n", 1e3 * duration, (double)total / duration);

    CHECK(dzo_adgd_batch_destroy(q));
    CHECK(dzo_tempering_destroy(pt));
    CHECK(dzo_free(minima_dev));
    CHECK(dzo_free(replicas_dev));
    CHECK(dzo_shutdown());
    if (!ok) { printf("FAILED: a quench did not lower its replica's energy\n"); return 1; }
    if (active != 0) { printf("FAILED: %lld instances still moving after %d steps\n", (long long)active, MAX_STEPS); return 1; }
    if (sorted[0] < LJ38 - 5e-7) { printf("FAILED: a minimum below the global one\n"); return 1; }
    printf("OK\n");
    return 0;
}
