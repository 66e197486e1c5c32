/* lj_tempering.c -- parallel tempering of 256 replicas of the 38-atom Lennard-Jones cluster on the device, plain C against
 * include/dzo.h: the `main` of the reference's driver script (scripts/MonteCarlo.jl:183-260).
 *
 *     main(num_particles=38, num_replicas=256, min_temp=0.05, max_temp=0.35, constraining_radius=2.25,
 *          num_steps=500, num_batches=1000)
 *
 * Start (:198-213): every particle a standard-normal point, redrawn until it lies inside the constraining sphere; here from
 * a seeded host generator (Box-Muller over a 64-bit LCG).  Inverse temperatures (:215): geometric from 1 / min_temp to
 * 1 / max_temp.  Perturbation radii (:216): 2^-12, or the third argument.  One pass of the script's outer loop (:222-231) is
 * dzo_tempering_run; the script repeats it for ever and plots, this program runs it twice -- the first pass untimed, to leave
 * the start behind -- and prints the reference's own metric and the heat-capacity curve of the second pass as numbers.
 *
 *   gcc -O2 -Iinclude examples/lj_tempering.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_tempering && ./lj_tempering [num_steps [num_batches [radius]]]
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

int main(int argc, char **argv) {
    const int64_t num_steps = argc > 1 ? atoll(argv[1]) : 500;
    const int64_t num_batches = argc > 2 ? atoll(argv[2]) : 20;
    const double radius0 = argc > 3 ? atof(argv[3]) : ldexp(1.0, -12);
    const double min_temp = 0.05, max_temp = 0.35, constraining_radius = 2.25;
    if (num_steps < 1 || num_batches < 1 || !(radius0 > 0.0)) { fprintf(stderr, "usage: lj_tempering [num_steps [num_batches [radius]]]\n"); return 2; }

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
    const int64_t rows = 2 * num_steps * num_batches;
    void *replicas_dev = NULL, *energies_dev = NULL;
    CHECK(dzo_malloc(&replicas_dev, (int64_t)sizeof replicas));
    CHECK(dzo_malloc(&energies_dev, (int64_t)sizeof(double) * rows * REPLICAS));
    CHECK(dzo_memcpy_h2d(replicas_dev, replicas, (int64_t)sizeof replicas));
    dzo_tempering_t pt = NULL;
    CHECK(dzo_tempering_create(DZO_RADIAL_LENNARD_JONES, N, REPLICAS, DZO_F64, replicas_dev, inv_temps, radii, constraining_radius, 1,
                               &pt));

    CHECK(dzo_tempering_run(pt, num_steps, num_batches, energies_dev, rows));
    CHECK(dzo_synchronize());
    const double start = now();
    CHECK(dzo_tempering_run(pt, num_steps, num_batches, energies_dev, rows));
    CHECK(dzo_synchronize());
    const double duration = now() - start;
    const double num_trials = 2.0 * (double)num_steps * (double)num_batches * REPLICAS;

    static double cv[REPLICAS], cv_prime[REPLICAS], moments[3 * REPLICAS];
    CHECK(dzo_tempering_analyze(pt, rows, energies_dev, rows, cv, cv_prime, moments));
    CHECK(dzo_tempering_read(pt, DZO_TEMPERING_RADII, radii));
    printf("#       k        T          <E>           cv     cv_prime   (R(T) in the last column of the radii line)\n");
    int finite = 1;
    for (int k = 0; k < REPLICAS; ++k) {
        printf("replica %d %.6f %.6f %.6e %.6e\n", k, 1.0 / inv_temps[k], moments[3 * k], cv[k], cv_prime[k]);
        if (!isfinite(moments[3 * k]) || !isfinite(cv[k]) || !isfinite(cv_prime[k])) finite = 0;
    }
    printf("radii: R(%.2f) = %.6f ... R(%.2f) = %.6f\n", min_temp, radii[0], max_temp, radii[REPLICAS - 1]);
    printf("Monte Carlo steps per second: %.6e\n", num_trials / duration);

    CHECK(dzo_tempering_destroy(pt));
    CHECK(dzo_free(energies_dev));
    CHECK(dzo_free(replicas_dev));
    CHECK(dzo_shutdown());
    if (!finite) { printf("FAILED: a moment or a heat capacity is not finite\n"); return 1; }
    printf("OK\n");
    return 0;
}
