/* lj_basin_hopping.c -- basin hopping (Wales & Doye 1997) over Lennard-Jones clusters, plain C against include/dzo.h: walkers
 * start from random points inside the constraining sphere; a hop perturbs every particle, quenches the trial with the batched
 * L-BFGS (step 0.01, history 10, at most 400 steps) and applies the Metropolis test to the quenched energies.  Every launch
 * runs HOPS_PER_LAUNCH hops of every walker at the walker's own pace.  The 13-atom cluster must reach the icosahedron,
 * -44.326801; for any other N (38: the literature's -173.928427) the best energy is only reported.
 *
 *   gcc -O2 -Iinclude examples/lj_basin_hopping.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_basin_hopping && ./lj_basin_hopping [N [walkers [hops [seed]]]]
 *
 * Defaults (N = 13): 64 walkers, 16 hops.  They come from a run on an MI355X (2026-10-19): with 64 walkers and seeds 1 .. 5 the best
 * energy, looked at after every launch of 4 hops, was first within 1e-6 of -44.326801 after 0, 0, 4, 4 and 4 hops (0: one of the
 * 64 quenched starts already is the icosahedron); 16 is four times the worst of the five.  After 64 hops 63 or 64 of the 64 walkers
 * had it as their best.
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

#define MAX_N 64
#define MAX_WALKERS 1024
#define HOPS_PER_LAUNCH 4
#define LJ13 (-44.326801)
#define LJ38 (-173.928427)

static uint64_t lcg_state;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 13;
    const int walkers = argc > 2 ? atoi(argv[2]) : 64;
    const int64_t hops = argc > 3 ? atoll(argv[3]) : 16;
    const uint64_t seed = argc > 4 ? strtoull(argv[4], NULL, 10) : 1;
    if (n < 2 || n > MAX_N || walkers < 1 || walkers > MAX_WALKERS || hops < 0) {
        fprintf(stderr, "usage: lj_basin_hopping [N (2..%d) [walkers (1..%d) [hops [seed]]]]\n", MAX_N, MAX_WALKERS);
        return 2;
    }
    /* a sphere that holds the cluster at its bulk density with room to spare; temperature 0.8, radius 0.35 (Wales & Doye) */
    const double constraining_radius = 1.0 + 0.75 * cbrt((double)n), temperature = 0.8, radius0 = 0.35;
    lcg_state = 0x9E3779B97F4A7C15ull + seed;

    static double points[MAX_WALKERS * 3 * MAX_N];           /* walker k: [x | y | z] at 3 n k */
    for (int k = 0; k < walkers; ++k)
        for (int i = 0; i < n; ++i)
            for (;;) {
                const double x = constraining_radius * (2.0 * uniform01() - 1.0), y = constraining_radius * (2.0 * uniform01() - 1.0),
                             z = constraining_radius * (2.0 * uniform01() - 1.0);
                if (x * x + y * y + z * z < constraining_radius * constraining_radius) {
                    double *p = points + (size_t)3 * n * k;
                    p[i] = x; p[n + i] = y; p[2 * n + i] = z;
                    break;
                }
            }
    static double inv_temps[MAX_WALKERS], radii[MAX_WALKERS];
    for (int k = 0; k < walkers; ++k) { inv_temps[k] = 1.0 / temperature; radii[k] = radius0; }

    CHECK(dzo_init(0));
    const int64_t bytes = (int64_t)sizeof(double) * 3 * n * walkers;
    void *points_dev = NULL;
    CHECK(dzo_malloc(&points_dev, bytes));
    CHECK(dzo_memcpy_h2d(points_dev, points, bytes));
    dzo_basin_hopping_t bh = NULL;
    CHECK(dzo_basin_hopping_create(DZO_RADIAL_LENNARD_JONES, n, walkers, DZO_F64, points_dev, inv_temps, radii, constraining_radius, 0.01, 10,
                                   400, seed, &bh));
    static double best[MAX_WALKERS];
    static int64_t accepted[MAX_WALKERS], iterations[MAX_WALKERS], unfinished[MAX_WALKERS];
    const double target = n == 13 ? LJ13 : n == 38 ? LJ38 : 0.0;
    const double start = now();
    int64_t done = 0, first_hit = -1, total_accepted = 0;
    double lowest = INFINITY;
    for (;;) {
        CHECK(dzo_basin_hopping_read(bh, DZO_BASIN_HOPPING_BEST_ENERGIES, best));   /* waits for the launches so far */
        for (int k = 0; k < walkers; ++k)
            if (best[k] < lowest) lowest = best[k];
        if (first_hit < 0 && target != 0.0 && fabs(lowest - target) <= 1e-6) first_hit = done;
        if (done >= hops) break;
        const int64_t k = hops - done < HOPS_PER_LAUNCH ? hops - done : HOPS_PER_LAUNCH;
        CHECK(dzo_basin_hopping_hop(bh, k, 1));
        CHECK(dzo_basin_hopping_read(bh, DZO_BASIN_HOPPING_NUM_ACCEPT, accepted));
        for (int w = 0; w < walkers; ++w) total_accepted += accepted[w];
        done += k;
    }
    const double duration = now() - start;
    CHECK(dzo_basin_hopping_read(bh, DZO_BASIN_HOPPING_QUENCH_ITERATIONS, iterations));
    CHECK(dzo_basin_hopping_read(bh, DZO_BASIN_HOPPING_QUENCH_UNFINISHED, unfinished));
    int64_t total_iterations = 0, total_unfinished = 0;
    int at_lowest = 0;
    for (int k = 0; k < walkers; ++k) {
        total_iterations += iterations[k];
        total_unfinished += unfinished[k];
        if (best[k] - lowest <= 1e-6) ++at_lowest;
    }
    printf("N = %d, %d walkers, %lld hops each, seed %llu\n", n, walkers, (long long)done, (unsigned long long)seed);
    printf("best energy: %.6f", lowest);
    if (target != 0.0) printf(" (literature %.6f)", target);
    printf("\nwalkers whose best is within 1e-6 of it: %d\n", at_lowest);
    if (target != 0.0) printf("first reached after hops: %lld\n", (long long)first_hit);
    printf("accepted hops: %lld of %lld; L-BFGS iterations: %lld; quenches cut off at 400 steps: %lld\n", (long long)total_accepted,
           (long long)(done * walkers), (long long)total_iterations, (long long)total_unfinished);
    printf("hopping: %.3f ms, %.6e hops per second\n", 1e3 * duration, duration > 0 ? (double)(done * walkers) / duration : 0.0);

    CHECK(dzo_basin_hopping_destroy(bh));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    if (target != 0.0 && lowest < target - 5e-7) { printf("FAILED: a minimum below the global one\n"); return 1; }
    if (n == 13) {
        if (fabs(lowest - LJ13) > 1e-6) { printf("FAILED: the icosahedron was not reached\n"); return 1; }
        printf("OK\n");
    }
    return 0;
}
