/* lj_spectrum.c -- minimum or saddle?  Plain C against include/dzo.h, and nothing leaves the device before the answer: four
 * jittered copies of the 13-atom Lennard-Jones icosahedron are relaxed by one batched LBFGSOptimizer
 * (src/DZOptimization.jl:321-509, step 0.01, history 10), dzo_pairwise_batch_hessian forms their dense 39 x 39 Hessians, and
 * dzo_symmetric_batch_eigen diagonalises all of them in one launch.  Per instance: the Morse index (eigenvalues below -tol),
 * the zero modes (|lambda| <= tol: six for a cluster in free space) and the lowest vibration.
 *
 *   gcc -O2 -Iinclude examples/lj_spectrum.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_spectrum && ./lj_spectrum
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "dzo.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int32_t rc_ = (call);                                                        \
        if (rc_ != DZO_OK) {                                                         \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, dzo_last_error());   \
            return 1;                                                                \
        }                                                                            \
    } while (0)

#define N 13
#define N3 (3 * N)
#define BATCH 4
#define STEPS_PER_LAUNCH 50
#define MAX_STEPS 5000
#define LJ13 (-44.326801)

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

int main(void) {
    /* centre + the 12 cyclic permutations of (0, +-1, +-phi), vertices 1.08 from the centre; a point is [x | y | z] */
    const double phi = (1.0 + sqrt(5.0)) / 2.0, scale = 1.08 / sqrt(1.0 + phi * phi);
    double ideal[N3] = {0};
    int n = 1;
    for (int sa = -1; sa <= 1; sa += 2)
        for (int sb = -1; sb <= 1; sb += 2) {
            const double a = sa * scale, b = sb * phi * scale;
            ideal[n] = 0; ideal[N + n] = a; ideal[2 * N + n] = b; ++n;
            ideal[n] = a; ideal[N + n] = b; ideal[2 * N + n] = 0; ++n;
            ideal[n] = b; ideal[N + n] = 0; ideal[2 * N + n] = a; ++n;
        }
    static double points[BATCH][N3];
    for (int k = 0; k < BATCH; ++k)
        for (int e = 0; e < N3; ++e) points[k][e] = ideal[e] + 0.03 * (2.0 * uniform01() - 1.0);

    CHECK(dzo_init(0));
    int32_t storage = -1;
    int64_t ld = 0, lds_bytes = 0;
    CHECK(dzo_symeig_plan(N3, DZO_F64, &storage, &ld, &lds_bytes));
    printf("plan: n = %d in fp64 on %s storage, leading dimension %lld, %lld bytes of LDS\n", N3,
           storage == DZO_SYMEIG_STORAGE_LDS ? "LDS" : "memory", (long long)ld, (long long)lds_bytes);
    void *points_dev = NULL, *hessians_dev = NULL, *eigenvalues_dev = NULL, *sweeps_dev = NULL;
    CHECK(dzo_malloc(&points_dev, (int64_t)sizeof points));
    CHECK(dzo_malloc(&hessians_dev, (int64_t)(BATCH * N3 * N3 * sizeof(double))));
    CHECK(dzo_malloc(&eigenvalues_dev, (int64_t)(BATCH * N3 * sizeof(double))));
    CHECK(dzo_malloc(&sweeps_dev, (int64_t)(BATCH * sizeof(int32_t))));
    CHECK(dzo_memcpy_h2d(points_dev, points, (int64_t)sizeof points));

    /* quench: the handle aliases points_dev */
    dzo_lbfgs_batch_t q = NULL;
    CHECK(dzo_lbfgs_batch_create(DZO_RADIAL_LENNARD_JONES, N, BATCH, DZO_F64, points_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    double energies[BATCH];
    CHECK(dzo_lbfgs_batch_read(q, DZO_LBFGS_BATCH_OBJECTIVES, energies));
    CHECK(dzo_lbfgs_batch_destroy(q));

    /* Hessians and their spectra, device to device; eigenvectors are not asked for */
    CHECK(dzo_pairwise_batch_hessian(DZO_RADIAL_LENNARD_JONES, N, BATCH, DZO_F64, points_dev, hessians_dev));
    CHECK(dzo_symmetric_batch_eigen(N3, BATCH, DZO_F64, hessians_dev, eigenvalues_dev, NULL, (int32_t *)sweeps_dev, 0));
    static double eigenvalues[BATCH][N3];
    int32_t sweeps[BATCH];
    CHECK(dzo_memcpy_d2h(eigenvalues, eigenvalues_dev, (int64_t)sizeof eigenvalues));
    CHECK(dzo_memcpy_d2h(sweeps, sweeps_dev, (int64_t)sizeof sweeps));

    int ok = 1;
    for (int k = 0; k < BATCH; ++k) {
        /* the quench leaves a residual gradient, which moves the rigid-body zeros: 1e-5 of the stiffest mode separates them from
         * the softest vibration */
        const double tol = 1e-5 * eigenvalues[k][N3 - 1];
        int index = 0, zeros = 0;
        for (int e = 0; e < N3; ++e) {
            if (eigenvalues[k][e] < -tol) ++index;
            else if (fabs(eigenvalues[k][e]) <= tol) ++zeros;
        }
        printf("instance %d: index %d zeros %d sweeps %d energy %.6f lowest vibration %.6f stiffest %.6f\n", k, index, zeros, (int)sweeps[k],
               energies[k], eigenvalues[k][index + zeros < N3 ? index + zeros : N3 - 1], eigenvalues[k][N3 - 1]);
        if (index != 0 || zeros != 6 || sweeps[k] < 1 || !(fabs(energies[k] - LJ13) <= 5e-7)) ok = 0;
    }

    CHECK(dzo_free(sweeps_dev));
    CHECK(dzo_free(eigenvalues_dev));
    CHECK(dzo_free(hessians_dev));
    CHECK(dzo_free(points_dev));
    CHECK(dzo_shutdown());
    if (!ok) { printf("FAILED: a quenched icosahedron is not a minimum with six zero modes\n"); return 1; }
    printf("OK\n");
    return 0;
}
