/* morse_quench.c -- the Morse pair potential through the C ABI, plain C against include/dzo.h: 64 jittered 13-atom icosahedra are
 * quenched by one batched LBFGSOptimizer (step 0.01, history 10, 50 calls of step!() per launch) under rho = 6 and again under
 * rho = 14.  For each range: the lowest energy found, the gradient norm there, and the Morse index (negative and zero Hessian
 * eigenvalues, from one dense-Hessian launch and the batched eigensolver).  Lengths are in units of the pair distance (pair
 * minimum at r = 1, depth 1): the rho = 6 icosahedron is -42.439863 in the Cambridge Cluster Database.
 *
 *   gcc -O2 -Iinclude examples/morse_quench.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o morse_quench && ./morse_quench
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

#define N 13
#define DIM (3 * N)
#define BATCH 64
#define STEPS_PER_LAUNCH 50
#define MAX_STEPS 20000
#define MORSE13_RHO6 (-42.439863)

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double uniform01(void) {                            /* in (0, 1) */
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

static int run(int32_t radial, int rho, double *lowest_out) {
    /* centre + the 12 cyclic permutations of (0, +-1, +-phi), vertices one pair distance from the centre, each coordinate
     * jittered by +-0.05 */
    const double phi = 0.5 * (1.0 + sqrt(5.0)), scale = 1.0 / sqrt(1.0 + phi * phi);
    double ico[N][3] = {{0.0, 0.0, 0.0}};
    int n = 1;
    for (int a = -1; a <= 1; a += 2)
        for (int b = -1; b <= 1; b += 2) {
            const double p = a * scale, q = b * phi * scale;
            ico[n][0] = 0.0; ico[n][1] = p; ico[n][2] = q; ++n;
            ico[n][0] = p; ico[n][1] = q; ico[n][2] = 0.0; ++n;
            ico[n][0] = q; ico[n][1] = 0.0; ico[n][2] = p; ++n;
        }
    static double points[BATCH][3][N];
    for (int k = 0; k < BATCH; ++k)
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < N; ++i) points[k][c][i] = ico[i][c] + 0.1 * (uniform01() - 0.5);

    void *points_dev = NULL, *grad_dev = NULL, *e_dev = NULL, *hess_dev = NULL, *lam_dev = NULL;
    CHECK(dzo_malloc(&points_dev, (int64_t)sizeof points));
    CHECK(dzo_malloc(&grad_dev, (int64_t)sizeof points));
    CHECK(dzo_malloc(&e_dev, (int64_t)(BATCH * sizeof(double))));
    CHECK(dzo_malloc(&hess_dev, (int64_t)(BATCH * DIM * DIM * sizeof(double))));
    CHECK(dzo_malloc(&lam_dev, (int64_t)(BATCH * DIM * sizeof(double))));
    CHECK(dzo_memcpy_h2d(points_dev, points, (int64_t)sizeof points));

    dzo_lbfgs_batch_t q = NULL;
    CHECK(dzo_lbfgs_batch_create(radial, N, BATCH, DZO_F64, points_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    CHECK(dzo_lbfgs_batch_destroy(q));

    static double energies[BATCH], grads[BATCH][DIM], lam[BATCH][DIM];
    CHECK(dzo_pairwise_batch_energy_gradient(radial, N, BATCH, DZO_F64, points_dev, e_dev, grad_dev));
    CHECK(dzo_pairwise_batch_hessian(radial, N, BATCH, DZO_F64, points_dev, hess_dev));
    CHECK(dzo_symmetric_batch_eigen(DIM, BATCH, DZO_F64, hess_dev, lam_dev, NULL, NULL, 0));
    CHECK(dzo_memcpy_d2h(energies, e_dev, (int64_t)sizeof energies));
    CHECK(dzo_memcpy_d2h(grads, grad_dev, (int64_t)sizeof grads));
    CHECK(dzo_memcpy_d2h(lam, lam_dev, (int64_t)sizeof lam));

    int best = 0;
    for (int k = 1; k < BATCH; ++k)
        if (energies[k] < energies[best]) best = k;
    double gg = 0.0;
    for (int e = 0; e < DIM; ++e) gg += grads[best][e] * grads[best][e];
    const double tol = 1e-6 * lam[best][DIM - 1];            /* between the six rigid-body modes and the softest vibration */
    int negatives = 0, zeros = 0;
    for (int e = 0; e < DIM; ++e) {
        if (lam[best][e] < -tol) ++negatives;
        else if (fabs(lam[best][e]) <= tol) ++zeros;
    }
    printf("rho = %2d: lowest energy %.6f, gradient norm %.2e, Morse index %d (%d zero modes), %s after %lld steps per cluster\n", rho,
           energies[best], sqrt(gg), negatives, zeros, all_stuck ? "all at rest" : "NOT all at rest", (long long)launched);
    *lowest_out = energies[best];

    CHECK(dzo_free(lam_dev));
    CHECK(dzo_free(hess_dev));
    CHECK(dzo_free(e_dev));
    CHECK(dzo_free(grad_dev));
    CHECK(dzo_free(points_dev));
    if (!all_stuck) { printf("FAILED: clusters still moving after %d steps\n", MAX_STEPS); return 1; }
    if (negatives != 0 || zeros != 6) { printf("FAILED: the lowest structure is not a minimum with six zero modes\n"); return 1; }
    if (!(sqrt(gg) <= 1e-5)) { printf("FAILED: the gradient has not vanished\n"); return 1; }
    return 0;
}

int main(void) {
    CHECK(dzo_init(0));
    double e6 = 0.0, e14 = 0.0;
    if (run(DZO_RADIAL_MORSE_RHO6, 6, &e6) != 0) return 1;
    if (run(DZO_RADIAL_MORSE_RHO14, 14, &e14) != 0) return 1;
    CHECK(dzo_shutdown());
    if (fabs(e6 - MORSE13_RHO6) > 5e-6) { printf("FAILED: rho = 6 ends at %.6f, the literature icosahedron is %.6f\n", e6, MORSE13_RHO6); return 1; }
    printf("OK\n");
    return 0;
}
