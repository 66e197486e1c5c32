// dzo_hybridef.hip -- hybrid eigenvector following (Munro & Wales 1999) over MANY Lennard-Jones clusters on gfx950:
// dzo_hybridef_batch_*.  A transition-state search that never forms a Hessian: per step the lowest mode is refined from the
// previous step's vector by a few Lanczos products (dzo_lowmode.hip through dzo_chain.h), then the step kernel of this file
// walks uphill along that mode and relaxes in the subspace orthogonal to it by a few Barzilai-Borwein gradient steps.  So the
// unit serves the 1024 particles of every other cluster unit where the dense one (dzo_modefollow.hip) stops at 128.
// include/dzo.h, "Batched hybrid eigenvector following", states the step operation by operation (tests/hybridef_twin.py
// replays it on the CPU); the numbers 1 .. 5 below are its items.
//
// A step of the handle is two launches on the library's stream with no host wait between them.  The step kernel has the two
// launch shapes of every cluster unit and ONE body (he_run):
//
//   * WAVE shape (N <= 64): one wave per instance, lane i holds particle i: its coordinates, its entries of the mode, of the
//     gradient and of the previous tangent point and projected gradient, all in registers.
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per instance, thread t owns particles t, t + 256, ... in registers
//     likewise; the point is staged in LDS for the pair loop of cl_block_eval.
//
// Energies and gradients are cl_wave_eval / cl_block_eval, so they carry the bits of dzo_pairwise_batch_energy_gradient.  Sums
// over the particles are fp64 in the order of the sums of dzo_lowmode.hip: cl_dot3 per particle, the wave tree, then the four
// wave sums in wave order (cl_block_sum).  Every decision is taken from such a sum, which every thread holds: the control
// flow is block-uniform.  One writer per element; every loop is bounded by an argument.
#include "dzo_chain.h"
#include "dzo_cluster.h"

#include <cmath>
#include <new>

namespace dzo {

static_assert(DZO_HYBRIDEF_MAX_PARTICLES == kClMaxN, "the argument checks of dzo_cluster.h state the particle bound");
static_assert(DZO_HYBRIDEF_MAX_PARTICLES == DZO_LOWMODE_MAX_PARTICLES, "the mode launch serves every size the step kernel does");

template <typename T> struct HybridefArgs {
    int N, tangent_steps, tangent_steps_convex;
    T zero_tol;
    double max_step, tangent_cap, tangent_first, grad_tol;
    T *x;                      // (3N, batch) points, moved
    const T *lam_in;           // (batch) the mode launch's eigenvalues
    const T *u_in;             // (3N, batch) its vectors
    const double *res_in;      // (batch) its residuals, or null
    const int32_t *info;       // (3, batch) its status, cycles, products, or null
    T *E, *g, *lam, *u, *F, *h;   // records: (batch), (3N, batch), (batch), (3N, batch), (batch), (batch); each may be null
    double *grms, *res;        // (batch); may be null
    int32_t *status;           // (batch): an instance that is not ACTIVE is left alone
    int32_t *tangent;          // (batch); may be null
    int64_t *iters, *products, *evals;   // (batch); may be null
};

// X: 3N elements of LDS (BLOCK; unused by WAVE); red: 2 * kWaves doubles of LDS (BLOCK)
template <typename T, typename RF, bool BLOCK> __device__ __forceinline__ void he_run(const HybridefArgs<T> &a, T *X, double *red) {
    constexpr int PER = BLOCK ? kClPer : 1;
    const int64_t b = blockIdx.x;
    if (a.status[b] != DZO_HYBRIDEF_ACTIVE) return;          // frozen: the whole block
    const int tid = threadIdx.x, N = a.N, n = 3 * N;
    const int64_t base = (int64_t)n * b;
    int par = 0;

    bool live[PER];
    T x[3][PER], u[3][PER], g[3][PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + kBlock * q;
        live[q] = i < N;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c][q] = live[q] ? a.x[base + c * N + i] : T(0);
            u[c][q] = live[q] ? a.u_in[base + c * N + i] : T(0);
        }
    }
    // E and g at x.  BLOCK: every earlier read of X lies before a barrier every thread has passed (the sum that ends
    // cl_block_eval), so the point can be staged at once.
    auto eval = [&](T &E) {
        if constexpr (BLOCK) {
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int i = tid + kBlock * q;
                if (live[q]) { X[i] = x[0][q]; X[N + i] = x[1][q]; X[2 * N + i] = x[2][q]; }
            }
            __syncthreads();
            cl_block_eval<T, RF>(N, tid, X, red, par, E, g[0], g[1], g[2]);
        } else {
            cl_wave_eval<T, RF>(N, tid, x[0][0], x[1][0], x[2][0], E, g[0][0], g[1][0], g[2][0]);
        }
    };
    // a sum over the particles in every thread, in the order of the sums
    auto sum = [&](double v) -> double {
        if constexpr (BLOCK) return cl_block_sum(v, red, par);
        else return 0.0 + wave_sum_all(v);
    };
    auto dot = [&](const T (&s)[3][PER], const T (&t)[3][PER]) -> double {
        double r = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) r += cl_dot3(s[0][q], s[1][q], s[2][q], t[0][q], t[1][q], t[2][q]);
        return sum(r);
    };

    // 1. evaluate; the records of the point before the move
    T E;
    eval(E);
    const double grms = __builtin_sqrt(dot(g, g) / (double)n);
    const T lam = a.lam_in[b], zt = a.zero_tol;
    const int mode_status = a.info ? a.info[3 * b] : (int)DZO_LOWMODE_CONVERGED;
    int64_t evals = 1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + kBlock * q;
        if (live[q]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.g) a.g[base + c * N + i] = g[c][q];
                if (a.u) a.u[base + c * N + i] = u[c][q];
            }
        }
    }
    // 2. the freeze check.  A non-finite g makes g.g, a sum of squares, non-finite.
    const bool bad = !cl_finite(E) || !(grms < __builtin_inf()) || !cl_finite(lam) || mode_status == DZO_LOWMODE_FAILED;
    const int status = bad ? DZO_HYBRIDEF_FAILED : (grms <= a.grad_tol ? DZO_HYBRIDEF_CONVERGED : DZO_HYBRIDEF_ACTIVE);
    T F = T(0), h = T(0);
    int made = 0;
    if (status == DZO_HYBRIDEF_ACTIVE) {                     // the same in every thread
        // 3. the uphill step
        F = (T)dot(u, g);
        const T al = cl_abs(lam);
        const T q0 = (F + F) / al;
        const T hq = q0 / (T(1) + cl_sqrt(T(1) + q0 * q0));
        h = al <= zt ? T(0) : hq;
        if ((double)cl_abs(h) > a.max_step) h = h < T(0) ? -(T)a.max_step : (T)a.max_step;
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c][q] = dfma<T>(h, u[c][q], x[c][q]);

        // 4. the tangent relaxation
        const int tmax = lam < -zt ? a.tangent_steps : a.tangent_steps_convex;
        T xp[3][PER], p[3][PER], pp[3][PER];
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) xp[c][q] = pp[c][q] = T(0);
        for (int t = 0; t < tmax; ++t) {
            T Et;
            eval(Et);
            evals += 1;
            const double cg = dot(u, g);
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c][q] = (T)((double)g[c][q] - cg * (double)u[c][q]);
            const double p2 = dot(p, p);
            if (__builtin_sqrt(p2 / (double)n) <= a.grad_tol) break;
            double alpha = a.tangent_first;
            if (t > 0) {
                double ss = 0, sy = 0;
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const T sx = x[0][q] - xp[0][q], sy_ = x[1][q] - xp[1][q], sz = x[2][q] - xp[2][q];
                    const T yx = p[0][q] - pp[0][q], yy = p[1][q] - pp[1][q], yz = p[2][q] - pp[2][q];
                    ss += cl_dot3(sx, sy_, sz, sx, sy_, sz);
                    sy += cl_dot3(sx, sy_, sz, yx, yy, yz);
                }
                ss = sum(ss);
                sy = sum(sy);
                if (sy > 0) alpha = ss / sy;
            }
            const double dn = alpha * __builtin_sqrt(p2);
            if (dn > a.tangent_cap) alpha = alpha * (a.tangent_cap / dn);
            const T na = -(T)alpha;
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xp[c][q] = x[c][q];
                    pp[c][q] = p[c][q];
                    x[c][q] = dfma<T>(na, p[c][q], x[c][q]);
                }
            made = t + 1;
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = tid + kBlock * q;
            if (live[q]) { a.x[base + i] = x[0][q]; a.x[base + N + i] = x[1][q]; a.x[base + 2 * N + i] = x[2][q]; }
        }
    }
    // 5. the records
    if (tid == 0) {
        if (a.E) a.E[b] = E;
        if (a.grms) a.grms[b] = grms;
        if (a.lam) a.lam[b] = lam;
        if (a.res) a.res[b] = a.res_in ? a.res_in[b] : 0.0;
        if (a.F) a.F[b] = F;
        if (a.h) a.h[b] = h;
        if (a.tangent) a.tangent[b] = made;
        if (a.products) a.products[b] += a.info ? (int64_t)a.info[3 * b + 2] : 0;
        if (a.evals) a.evals[b] += evals;
        if (a.iters && status == DZO_HYBRIDEF_ACTIVE) a.iters[b] += 1;
        a.status[b] = status;
    }
}

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
template <typename T, typename RF> __global__ __launch_bounds__(64) void hybridef_wave_step_kernel(HybridefArgs<T> a) { he_run<T, RF, false>(a, nullptr, nullptr); }

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
template <typename T, typename RF> __global__ __launch_bounds__(kBlock) void hybridef_block_step_kernel(HybridefArgs<T> a) {
    __shared__ T X[3 * kClMaxN];
    __shared__ double red[2 * kWaves];
    he_run<T, RF, true>(a, X, red);
}

template <typename T, typename RF> static void he_launch(hipStream_t s, int64_t batch, const HybridefArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((hybridef_wave_step_kernel<T, RF>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hybridef_block_step_kernel<T, RF>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

// the argument checks of apply and create
static int32_t he_check_args(int32_t radial, int64_t N, int64_t batch, int32_t dtype, double max_step, int32_t tangent_steps, int32_t tangent_steps_convex,
                             double tangent_cap, double tangent_first, double zero_tol, double grad_tol) {
    DZO_TRY(cl_check_args(radial, N, batch, dtype));
    DZO_REQUIRE(N >= 3, DZO_ERR_INVALID, "hybrid eigenvector following needs at least 3 particles (got %lld): fewer have no rotation-free subspace",
                (long long)N);
    DZO_REQUIRE(max_step > 0, DZO_ERR_INVALID, "max_step must be positive (got %g)", max_step);
    DZO_REQUIRE(tangent_steps >= 0 && tangent_steps_convex >= 0, DZO_ERR_INVALID, "tangent_steps and tangent_steps_convex must not be negative (got %d, %d)",
                tangent_steps, tangent_steps_convex);
    DZO_REQUIRE(tangent_cap > 0 && tangent_first > 0, DZO_ERR_INVALID, "tangent_cap and tangent_first must be positive (got %g, %g)", tangent_cap,
                tangent_first);
    DZO_REQUIRE(zero_tol >= 0 && grad_tol >= 0, DZO_ERR_INVALID, "zero_tol and grad_tol must not be negative (got %g, %g)", zero_tol, grad_tol);
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

struct dzo_hybridef_batch_s {
    ClCore core;                     // x, g, f; stuck = the status (ACTIVE is 0); iters
    // u: the modes of record, the start of the next refinement; u_new, lam_new, res_new, info: what the mode launch writes
    void *u = nullptr, *u_new = nullptr, *lam = nullptr, *lam_new = nullptr, *F = nullptr, *hup = nullptr, *basis = nullptr;
    double *grms = nullptr, *res = nullptr, *res_new = nullptr;
    int32_t *info = nullptr, *tangent = nullptr;
    int64_t *products = nullptr, *evals = nullptr;
    bool have_modes = false;         // false: the first refinement draws its start
    int32_t tangent_steps = 0, tangent_steps_convex = 0, krylov = 0, mode_cycles = 0;
    double max_step = 0, tangent_cap = 0, tangent_first = 0, mode_tol = 0, zero_tol = 0, grad_tol = 0;
    uint64_t base_seed = 0;
};

namespace dzo {

static void he_free(dzo_hybridef_batch_s *h) {
    cl_free(h, {h->u, h->u_new, h->lam, h->lam_new, h->F, h->hup, h->basis, h->grms, h->res, h->res_new, h->info, h->tangent, h->products, h->evals});
}

template <typename T> static HybridefArgs<T> he_args(const dzo_hybridef_batch_s *h) {
    const ClCore &c = h->core;
    HybridefArgs<T> a;
    a.N = c.N; a.tangent_steps = h->tangent_steps; a.tangent_steps_convex = h->tangent_steps_convex;
    a.zero_tol = (T)h->zero_tol; a.max_step = h->max_step; a.tangent_cap = h->tangent_cap; a.tangent_first = h->tangent_first; a.grad_tol = h->grad_tol;
    a.x = (T *)c.x; a.lam_in = (const T *)h->lam_new; a.u_in = (const T *)h->u_new; a.res_in = h->res_new; a.info = h->info;
    a.E = (T *)c.f; a.g = (T *)c.g; a.lam = (T *)h->lam; a.u = (T *)h->u; a.F = (T *)h->F; a.h = (T *)h->hup;
    a.grms = h->grms; a.res = h->res; a.status = c.stuck; a.tangent = h->tangent;
    a.iters = c.iters; a.products = h->products; a.evals = h->evals;
    return a;
}

// `what` -> device address, bytes
static int32_t he_array(dzo_hybridef_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const ClCore &c = h->core;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, n3 = 3 * (size_t)c.N;
    switch (what) {
    case DZO_HYBRIDEF_POINTS: *p = c.x; *bytes = es * n3 * B; break;
    case DZO_HYBRIDEF_GRADIENTS: *p = c.g; *bytes = es * n3 * B; break;
    case DZO_HYBRIDEF_ENERGIES: *p = c.f; *bytes = es * B; break;
    case DZO_HYBRIDEF_GRMS: *p = h->grms; *bytes = 8 * B; break;
    case DZO_HYBRIDEF_STATUS: *p = c.stuck; *bytes = 4 * B; break;
    case DZO_HYBRIDEF_EIGENVALUES: *p = h->lam; *bytes = es * B; break;
    case DZO_HYBRIDEF_MODES: *p = h->u; *bytes = es * n3 * B; break;
    case DZO_HYBRIDEF_MODE_RESIDUALS: *p = h->res; *bytes = 8 * B; break;
    case DZO_HYBRIDEF_PROJECTIONS: *p = h->F; *bytes = es * B; break;
    case DZO_HYBRIDEF_UPHILL_STEPS: *p = h->hup; *bytes = es * B; break;
    case DZO_HYBRIDEF_TANGENT_STEPS: *p = h->tangent; *bytes = 4 * B; break;
    case DZO_HYBRIDEF_ITERATION_COUNTS: *p = c.iters; *bytes = 8 * B; break;
    case DZO_HYBRIDEF_PRODUCTS: *p = h->products; *bytes = 8 * B; break;
    case DZO_HYBRIDEF_EVALUATIONS: *p = h->evals; *bytes = 8 * B; break;
    default: set_error("unknown hybrid eigenvector-following array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

// the step of include/dzo.h, once, from the caller's modes
int32_t dzo_hybridef_batch_apply(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, const void *eigenvalues_dev,
                                 const void *modes_dev, double max_step, int32_t tangent_steps, int32_t tangent_steps_convex, double tangent_cap,
                                 double tangent_first, double zero_tol, double grad_tol, void *energies_dev, void *gradients_dev, void *projections_dev,
                                 void *uphill_steps_dev, double *grms_dev, int32_t *status_dev, int32_t *tangent_counts_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && eigenvalues_dev && modes_dev && status_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(he_check_args(radial, n_particles, batch, dtype, max_step, tangent_steps, tangent_steps_convex, tangent_cap, tangent_first, zero_tol, grad_tol));
    const char *where = "dzo_hybridef_batch_apply", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", eigenvalues_dev, "eigenvalues"));
    DZO_TRY(require_same_backend(where, cite, modes_dev, "modes", status_dev, "status"));
    DZO_TRY(require_same_backend(where, cite, energies_dev, "energies", gradients_dev, "gradients"));
    DZO_TRY(require_same_backend(where, cite, projections_dev, "projections", uphill_steps_dev, "uphill_steps"));
    DZO_TRY(require_same_backend(where, cite, grms_dev, "grms", tangent_counts_dev, "tangent_counts"));
    Context &c = ctx();
    {
        DZO_TIMED("hybridef_step", c.stream);
        DZO_HIP(hipMemsetAsync(status_dev, 0, 4 * (size_t)batch, c.stream));   // every instance ACTIVE
        DZO_DISPATCH_RADIAL(radial, dtype, HybridefArgs<T> a{};
                     a.N = (int)n_particles; a.tangent_steps = tangent_steps; a.tangent_steps_convex = tangent_steps_convex;
                     a.zero_tol = (T)zero_tol; a.max_step = max_step; a.tangent_cap = tangent_cap; a.tangent_first = tangent_first; a.grad_tol = grad_tol;
                     a.x = (T *)points_dev; a.lam_in = (const T *)eigenvalues_dev; a.u_in = (const T *)modes_dev;
                     a.E = (T *)energies_dev; a.g = (T *)gradients_dev; a.F = (T *)projections_dev; a.h = (T *)uphill_steps_dev;
                     a.grms = grms_dev; a.status = status_dev; a.tangent = tangent_counts_dev;
                     (he_launch<T, F>(c.stream, batch, a)));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

int32_t dzo_hybridef_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, const void *dirs_dev,
                                  double max_step, int32_t tangent_steps, int32_t tangent_steps_convex, double tangent_cap, double tangent_first,
                                  int32_t krylov, int32_t mode_cycles, double mode_tol, double zero_tol, double grad_tol, uint64_t base_seed,
                                  dzo_hybridef_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(he_check_args(radial, n_particles, batch, dtype, max_step, tangent_steps, tangent_steps_convex, tangent_cap, tangent_first, zero_tol, grad_tol));
    DZO_REQUIRE(krylov >= 2 && krylov <= DZO_LOWMODE_MAX_KRYLOV, DZO_ERR_INVALID, "krylov must be in 2 .. %d (got %d)", DZO_LOWMODE_MAX_KRYLOV, krylov);
    DZO_REQUIRE(mode_cycles >= 1 && mode_cycles < INT32_MAX, DZO_ERR_INVALID, "mode_cycles must be at least 1 (got %d)", mode_cycles);
    DZO_REQUIRE(mode_tol >= 0 && std::isfinite(mode_tol), DZO_ERR_INVALID, "mode_tol must be finite and not negative (got %g)", mode_tol);
    DZO_TRY(require_same_backend("dzo_hybridef_batch_create", "every array of a handle lives on one device", points_dev, "points", dirs_dev, "directions"));
    dzo_hybridef_batch_s *h = new (std::nothrow) dzo_hybridef_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.radial = radial; c.N = (int)n_particles; c.B = batch; c.x = points_dev;
    h->max_step = max_step; h->tangent_steps = tangent_steps; h->tangent_steps_convex = tangent_steps_convex; h->tangent_cap = tangent_cap;
    h->tangent_first = tangent_first; h->krylov = krylov; h->mode_cycles = mode_cycles; h->mode_tol = mode_tol; h->zero_tol = zero_tol;
    h->grad_tol = grad_tol; h->base_seed = base_seed; h->have_modes = dirs_dev != nullptr;
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles;
    int32_t rc = cl_alloc({{&c.g, es * n3 * B}, {&c.f, es * B}, {(void **)&c.stuck, 4 * B}, {(void **)&c.iters, 8 * B}, {(void **)&c.active_dev, 8},
                           {&h->u, es * n3 * B}, {&h->u_new, es * n3 * B}, {&h->lam, es * B}, {&h->lam_new, es * B}, {&h->F, es * B}, {&h->hup, es * B},
                           {c.N > 64 ? &h->basis : nullptr, es * n3 * (size_t)krylov * B}, {(void **)&h->grms, 8 * B}, {(void **)&h->res, 8 * B},
                           {(void **)&h->res_new, 8 * B}, {(void **)&h->info, 12 * B}, {(void **)&h->tangent, 4 * B}, {(void **)&h->products, 8 * B},
                           {(void **)&h->evals, 8 * B}},
                          "the hybrid eigenvector-following state");
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, nullptr, "hybrid eigenvector-following state", "hybrid eigenvector-following constructor", [&](hipStream_t s) -> int32_t {
            DZO_TRY(lm_prepare(radial, dtype, c.N, krylov, 1));
            DZO_TIMED("hybridef_init", s);
            if (dirs_dev) { DZO_HIP(hipMemcpyAsync(h->u, dirs_dev, es * n3 * B, hipMemcpyDeviceToDevice, s)); }
            // the energies and gradients of the points as given; every other record is zero until the first step
            DZO_DISPATCH(dtype, DZO_TRY(cl_launch_eval<T>(s, radial, c.N, batch, (const T *)c.x, (T *)c.f, (T *)c.g)));
            return DZO_OK;
        });
    if (rc != DZO_OK) { he_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_hybridef_batch_destroy(dzo_hybridef_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    he_free(h);
    return DZO_OK;
}

int32_t dzo_hybridef_batch_set_directions(dzo_hybridef_batch_t h, const void *dirs_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && dirs_dev, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->core.device);
    DZO_TRY(require_same_backend("dzo_hybridef_batch_set_directions", "every array of a handle lives on one device", dirs_dev, "directions", nullptr, ""));
    const ClCore &c = h->core;
    DZO_HIP(hipMemcpyAsync(h->u, dirs_dev, dtype_size(c.dtype) * 3 * (size_t)c.N * (size_t)c.B, hipMemcpyDeviceToDevice, ctx().stream));
    h->have_modes = true;
    return DZO_OK;
}

// per step: the mode refinement from the modes of record, then the step kernel; nothing waits in between
int32_t dzo_hybridef_batch_step(dzo_hybridef_batch_t h, int32_t steps, int32_t *all_done) {
    return cl_step(h, steps, all_done, [&](hipStream_t s) -> int32_t {
        const ClCore &c = h->core;
        for (int32_t k = 0; k < steps; ++k) {
            {
                DZO_TIMED("hybridef_mode", s);
                // mode_cycles cycles refine the vector; the first product of one more measures its eigenvalue and residual
                DZO_TRY(lm_enqueue(s, c.radial, c.dtype, c.N, c.B, c.x, 1, h->krylov, h->mode_cycles + 1, h->mode_tol, h->base_seed, h->have_modes ? h->u : nullptr,
                                   h->basis, h->lam_new, h->u_new, h->res_new, h->info));
            }
            h->have_modes = true;
            DZO_TIMED("hybridef_step", s);
            DZO_DISPATCH_RADIAL(c.radial, c.dtype, (he_launch<T, F>(s, c.B, he_args<T>(h))));
            DZO_HIP(hipGetLastError());
        }
        return DZO_OK;
    });
}

int32_t dzo_hybridef_batch_count_active(dzo_hybridef_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_hybridef_batch_get_ptr(dzo_hybridef_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, he_array, what, ptr_dev); }

int32_t dzo_hybridef_batch_read(dzo_hybridef_batch_t h, int32_t what, void *out_host) { return cl_read(h, he_array, what, out_host); }

}  // extern "C"
