/* lj_hessian.c -- second-order information on a quenched cluster, plain C against include/dzo.h: the 13-atom Lennard-Jones
 * icosahedron is relaxed to its minimum by a batched LBFGSOptimizer (src/DZOptimization.jl:321-509, step 0.01, history 10), its
 * dense 39 x 39 Hessian is formed by dzo_pairwise_batch_hessian, and dzo_pairwise_batch_hvp applies four directions to the
 * minimum in one launch (point_stride = 0): the three translations, along which the curvature vanishes, and the gradient of a
 * jittered copy of the minimum, along which it does not.  The Rayleigh quotients come from `curvatures` (u.Hu and u.u in fp64).
 *
 *   gcc -O2 -Iinclude examples/lj_hessian.c -Ldzoptimization.jl_amd -ldzo_hip \
 *       -Wl,-rpath,$PWD/dzoptimization.jl_amd -lm -o lj_hessian && ./lj_hessian
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
#define DIRECTIONS 4
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
    double point[N3] = {0};
    int n = 1;
    for (int sa = -1; sa <= 1; sa += 2)
        for (int sb = -1; sb <= 1; sb += 2) {
            const double a = sa * scale, b = sb * phi * scale;
            point[n] = 0; point[N + n] = a; point[2 * N + n] = b; ++n;
            point[n] = a; point[N + n] = b; point[2 * N + n] = 0; ++n;
            point[n] = b; point[N + n] = 0; point[2 * N + n] = a; ++n;
        }

    CHECK(dzo_init(0));
    void *point_dev = NULL, *hessian_dev = NULL, *jittered_dev = NULL, *energy_dev = NULL, *directions_dev = NULL, *products_dev = NULL,
         *curvatures_dev = NULL;
    CHECK(dzo_malloc(&point_dev, (int64_t)sizeof point));
    CHECK(dzo_malloc(&jittered_dev, (int64_t)sizeof point));
    CHECK(dzo_malloc(&energy_dev, (int64_t)sizeof(double)));
    CHECK(dzo_malloc(&hessian_dev, (int64_t)(N3 * N3 * sizeof(double))));
    CHECK(dzo_malloc(&directions_dev, (int64_t)(DIRECTIONS * N3 * sizeof(double))));
    CHECK(dzo_malloc(&products_dev, (int64_t)(DIRECTIONS * N3 * sizeof(double))));
    CHECK(dzo_malloc(&curvatures_dev, (int64_t)(2 * DIRECTIONS * sizeof(double))));
    CHECK(dzo_memcpy_h2d(point_dev, point, (int64_t)sizeof point));

    /* quench: one instance of the batched optimizer; the handle aliases point_dev */
    dzo_lbfgs_batch_t q = NULL;
    CHECK(dzo_lbfgs_batch_create(DZO_RADIAL_LENNARD_JONES, N, 1, DZO_F64, point_dev, 0.01, 10, &q));
    int32_t all_stuck = 0;
    int64_t launched = 0;
    while (!all_stuck && launched < MAX_STEPS) {
        CHECK(dzo_lbfgs_batch_step(q, STEPS_PER_LAUNCH, &all_stuck));
        launched += STEPS_PER_LAUNCH;
    }
    double energy = 0;
    CHECK(dzo_lbfgs_batch_read(q, DZO_LBFGS_BATCH_OBJECTIVES, &energy));
    CHECK(dzo_lbfgs_batch_destroy(q));
    CHECK(dzo_memcpy_d2h(point, point_dev, (int64_t)sizeof point));
    printf("energy: %.9f (literature %.6f)\n", energy, LJ13);
    printf("point:");
    for (int e = 0; e < N3; ++e) printf(" %.17g", point[e]);
    printf("\n");

    /* the dense Hessian, column-major: element r + N3 c */
    static double hessian[N3 * N3];
    CHECK(dzo_pairwise_batch_hessian(DZO_RADIAL_LENNARD_JONES, N, 1, DZO_F64, point_dev, hessian_dev));
    CHECK(dzo_memcpy_d2h(hessian, hessian_dev, (int64_t)sizeof hessian));
    double trace = 0, asymmetry = 0, largest = 0;
    for (int c = 0; c < N3; ++c) {
        trace += hessian[c + N3 * c];
        for (int r = 0; r < N3; ++r) {
            asymmetry = fmax(asymmetry, fabs(hessian[r + N3 * c] - hessian[c + N3 * r]));
            largest = fmax(largest, fabs(hessian[r + N3 * c]));
        }
    }
    printf("trace: %.17g\n", trace);
    printf("largest |H[r, c] - H[c, r]|: %.3e (largest entry %.3f)\n", asymmetry, largest);

    /* four directions applied to the one point: the translations and the gradient of a jittered copy */
    static double directions[DIRECTIONS][N3], jittered[N3], curvatures[DIRECTIONS][2];
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < N; ++i) directions[a][a * N + i] = 1.0;
    for (int e = 0; e < N3; ++e) jittered[e] = point[e] + 0.05 * (2.0 * uniform01() - 1.0);
    CHECK(dzo_memcpy_h2d(jittered_dev, jittered, (int64_t)sizeof jittered));
    CHECK(dzo_pairwise_batch_energy_gradient(DZO_RADIAL_LENNARD_JONES, N, 1, DZO_F64, jittered_dev, energy_dev,
                                             (char *)directions_dev + 3 * N3 * sizeof(double)));
    CHECK(dzo_memcpy_h2d(directions_dev, directions, (int64_t)(3 * N3 * sizeof(double))));
    CHECK(dzo_pairwise_batch_hvp(DZO_RADIAL_LENNARD_JONES, N, DIRECTIONS, DZO_F64, point_dev, 0, directions_dev, products_dev,
                                 (double *)curvatures_dev));
    CHECK(dzo_memcpy_d2h(curvatures, curvatures_dev, (int64_t)sizeof curvatures));
    const char *names[DIRECTIONS] = {"translation x", "translation y", "translation z", "gradient of a jittered copy"};
    int ok = isfinite(trace) && fabs(energy - LJ13) <= 5e-7;
    for (int k = 0; k < DIRECTIONS; ++k) {
        const double rayleigh = curvatures[k][0] / curvatures[k][1];
        printf("Rayleigh quotient along the %s: %.6e (u.Hu = %.6e, u.u = %.6e)\n", names[k], rayleigh, curvatures[k][0], curvatures[k][1]);
        /* a translation's rows are sums of N terms that cancel: rounding of the order N u trace; at a minimum every other mode is stiff */
        if (k < 3 ? !(fabs(rayleigh) <= 1e-9 * trace) : !(rayleigh > 1.0)) ok = 0;
    }

    CHECK(dzo_free(curvatures_dev));
    CHECK(dzo_free(products_dev));
    CHECK(dzo_free(directions_dev));
    CHECK(dzo_free(hessian_dev));
    CHECK(dzo_free(energy_dev));
    CHECK(dzo_free(jittered_dev));
    CHECK(dzo_free(point_dev));
    CHECK(dzo_shutdown());
    if (!ok) { printf("FAILED: the minimum's energy, a translation's curvature or the gradient direction's curvature is off\n"); return 1; }
    printf("OK\n");
    return 0;
}
