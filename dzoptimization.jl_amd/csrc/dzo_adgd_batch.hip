// dzo_adgd_batch.hip -- the live AdGDOptimizer (src/DZOptimization.jl:179-312, constraint_function! = nothing) over MANY small
// Lennard-Jones clusters on gfx950: dzo_adgd_batch_*.
//
// The second live optimizer on the launch shapes of dzo_cluster.h, next to dzo_lbfgs_batch.hip.  It keeps no history, so an
// instance is four vectors (point, gradient, delta_point, delta_gradient), two step sizes and a few scalars.  The trial's
// energy and gradient, the block sums and the sums of squares are dzo_cluster.h's: one definition with the quench, the same
// bits.  The backtracking loop is written out in both step kernels, as in the quench's: shared, it compiled to slower kernels.  The step-size rule (:285-299) is evaluated in T, operation by operation as adgd_next_state of
// dzo_adgd.hip does; it is the only arithmetic of this file.
//
//   * WAVE (N <= 64): point, gradient, both deltas, the trial and its gradient are registers; no LDS beyond the sums'.
//   * BLOCK (65 <= N <= 1024): dynamic LDS red[2 kWaves] | X | G | DX | DG | XT (the trial point, which the pair loop reads as
//     a broadcast); the trial gradient in registers.  5 * 3N elements: 120 KiB at N = 1024 in fp64.
#include "dzo_cluster.h"

#include <cmath>
#include <new>

namespace dzo {

constexpr int kAdgdBatchMaxN = DZO_ADGD_BATCH_MAX_PARTICLES;
static_assert(kAdgdBatchMaxN == kClMaxN, "the batched AdGD kernels use the evaluation routines of dzo_cluster.h and their particle bound");

template <typename T> struct AdgdBatchArgs {
    int N, steps;
    int64_t max_halvings;
    T step_length;
    T *x, *g, *dx, *dg;        // (3N, batch)
    T *f, *df, *cur, *prev;    // batch
    int32_t *stuck, *halv;
    int64_t *iters;
};

__device__ __forceinline__ double ab_sqrt(double v) { return ::sqrt(v); }
__device__ __forceinline__ float ab_sqrt(float v) { return ::sqrtf(v); }

// next_step_size of :290-295 from the sums of squares of delta_point and delta_gradient (fp64); every operation in T
template <typename T> __device__ __forceinline__ T ab_next_step_size(T current, T previous, double dx2, double dg2) {
    const T theta = current / previous;                      // :290
    T next = current * ab_sqrt(T(1) + theta);                // :291
    const T dgn = ab_sqrt((T)dg2);                           // :292
    if (dgn != T(0)) {                                       // :293
        const T inv_L = ab_sqrt((T)dx2) / dgn;               // :294
        const T cap = ab_sqrt(T(0.5)) * inv_L;
        next = next < cap ? next : cap;                      // :295
    }
    return next;
}

// the rest of the constructor (:229-241) behind the evaluation kernel, which left f0 and g0: grid batch, block 256
template <typename T> __global__ __launch_bounds__(kBlock) void adgd_batch_init_kernel(AdgdBatchArgs<T> a) {
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    double part = 0;
    for (int i = tid; i < N; i += kBlock) {
        const T gx = a.g[base + i], gy = a.g[base + N + i], gz = a.g[base + 2 * N + i];
        part += cl_dot3(gx, gy, gz, gx, gy, gz);
    }
    int par = 0;
    const double ss = cl_block_sum(part, red, par);          // :230
    if (tid == 0) {
        const bool stuck = ss == 0.0;                        // :231
        const T s0 = stuck ? T(0) : a.step_length / (T)::sqrt(ss);   // :232-233
        a.cur[b] = s0; a.prev[b] = s0;                       // :241
        a.stuck[b] = stuck ? 1 : 0;
    }
}

// (a step kernel is its body as a __device__ function and the entry point that calls it: written into the __global__ function
// itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
template <typename T, typename F> __device__ __forceinline__ void adgd_batch_wave_step_body(AdgdBatchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // :276, the whole wave
    const int lane = threadIdx.x, N = a.N;
    const int64_t base = (int64_t)3 * N * b;
    const bool live = lane < N;
    auto ld = [&](const T *p, int c) { return live ? p[base + c * N + lane] : T(0); };
    T x = ld(a.x, 0), y = ld(a.x, 1), z = ld(a.x, 2);
    T gx = ld(a.g, 0), gy = ld(a.g, 1), gz = ld(a.g, 2);
    T sx = ld(a.dx, 0), sy = ld(a.dx, 1), sz = ld(a.dx, 2);
    T yx = ld(a.dg, 0), yy = ld(a.dg, 1), yz = ld(a.dg, 2);
    T E = a.f[b], dE = a.df[b], cur = a.cur[b], prev = a.prev[b];
    int64_t it = a.iters[b];
    int halv = a.halv[b];
    bool stuck = false;
    for (int s = 0; s < a.steps && !stuck; ++s) {
        T next = cur;                                        // :287
        if (it > 0) {                                        // :288
            const double dg2 = wave_sum_all(cl_dot3(yx, yy, yz, yx, yy, yz));
            const double dx2 = wave_sum_all(cl_dot3(sx, sy, sz, sx, sy, sz));
            next = ab_next_step_size<T>(cur, prev, dx2, dg2);
        }
        prev = cur; cur = next;                              // :298-299
        // take_backtracking_step!(opt, -next, current_gradient), :107-154
        const T x0 = x, y0 = y, z0 = z;                      // :118
        T t = next;
        int h = 0;
        for (;;) {
            const T xt = dfma<T>(-t, gx, x0), yt = dfma<T>(-t, gy, y0), zt = dfma<T>(-t, gz, z0);   // :124
            if (__all(is_equal(xt, x0) && is_equal(yt, y0) && is_equal(zt, z0))) { stuck = true; break; }   // :128
            T Et, tx, ty, tz;
            cl_wave_eval<T, F>(N, lane, xt, yt, zt, Et, tx, ty, tz);
            if (Et < E) {                                    // :139
                dE = Et - E; E = Et;                         // :142-144
                sx = xt - x0; sy = yt - y0; sz = zt - z0;    // :145
                yx = tx - gx; yy = ty - gy; yz = tz - gz;    // :306-308
                x = xt; y = yt; z = zt;
                gx = tx; gy = ty; gz = tz;
                break;
            }
            t *= T(0.5);                                     // :152 (the point was never overwritten: :151)
            if (++h >= a.max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (stuck) { sx = x0; sy = y0; sz = z0; break; }     // delta_point keeps the copy of :118
        ++it;                                                // :310
    }
    if (live) {
        auto st = [&](T *p, int c, T v) { p[base + c * N + lane] = v; };
        st(a.x, 0, x); st(a.x, 1, y); st(a.x, 2, z);
        st(a.g, 0, gx); st(a.g, 1, gy); st(a.g, 2, gz);
        st(a.dx, 0, sx); st(a.dx, 1, sy); st(a.dx, 2, sz);
        st(a.dg, 0, yx); st(a.dg, 1, yy); st(a.dg, 2, yz);
    }
    if (lane == 0) {
        a.f[b] = E; a.df[b] = dE;
        a.cur[b] = cur; a.prev[b] = prev;
        a.stuck[b] = stuck ? 1 : 0;
        a.iters[b] = it;
        a.halv[b] = halv;
    }
}
template <typename T, typename F> __global__ __launch_bounds__(64) void adgd_batch_wave_step_kernel(AdgdBatchArgs<T> a) { adgd_batch_wave_step_body<T, F>(a); }

extern __shared__ __attribute__((aligned(16))) double adgd_batch_smem[];

template <typename T, typename F> __device__ __forceinline__ void adgd_batch_block_step_body(AdgdBatchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // the whole block
    const int tid = threadIdx.x, N = a.N, n3 = 3 * N;
    const int64_t base = (int64_t)n3 * b;
    // LDS: red[2 kWaves] | X | G | DX | DG | XT
    double *red = adgd_batch_smem;
    T *X = reinterpret_cast<T *>(red + 2 * kWaves), *G = X + n3, *DX = G + n3, *DG = DX + n3, *XT = DG + n3;
    T *const gx_ = pw_pin_ptr(a.x + base), *const gg_ = pw_pin_ptr(a.g + base), *const gdx_ = pw_pin_ptr(a.dx + base);
    T *const gdg_ = pw_pin_ptr(a.dg + base), *const gf_ = pw_pin_ptr(a.f + b), *const gdf_ = pw_pin_ptr(a.df + b);
    T *const gcur_ = pw_pin_ptr(a.cur + b), *const gprev_ = pw_pin_ptr(a.prev + b);
    int32_t *const gstuck_ = pw_pin_ptr(a.stuck + b), *const ghalv_ = pw_pin_ptr(a.halv + b);
    int64_t *const git_ = pw_pin_ptr(a.iters + b);
    int halv = *ghalv_, par = 0;
    int64_t it = *git_;
    T E = *gf_, dE = *gdf_, cur = *gcur_, prev = *gprev_;
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        X[e] = gx_[e]; G[e] = gg_[e]; DX[e] = gdx_[e]; DG[e] = gdg_[e];
    })
    bool stuck = false;
    for (int s = 0; s < a.steps && !stuck; ++s) {
        T next = cur;                                        // :287
        if (it > 0) {                                        // :288
            double pg = 0, px = 0;
            CL_FOR_OWN(i, pg += cl_dot3(DG[i], DG[N + i], DG[2 * N + i], DG[i], DG[N + i], DG[2 * N + i]);
                       px += cl_dot3(DX[i], DX[N + i], DX[2 * N + i], DX[i], DX[N + i], DX[2 * N + i]);)
            const double dg2 = cl_block_sum(pg, red, par);
            const double dx2 = cl_block_sum(px, red, par);
            next = ab_next_step_size<T>(cur, prev, dx2, dg2);
        }
        prev = cur; cur = next;                              // :298-299
        // take_backtracking_step!(opt, -next, current_gradient), :107-154: X keeps the old point, XT is the trial (:124)
        T t = next;
        int h = 0;
        bool accepted = false;
        T tx[kClPer], ty[kClPer], tz[kClPer];
        for (;;) {
            bool same = true;
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
                const T v = dfma<T>(-t, G[c * N + i], X[c * N + i]);
                XT[c * N + i] = v;
                same = same && is_equal(v, X[c * N + i]);
            })
            if (__syncthreads_and(same ? 1 : 0)) { stuck = true; break; }   // :128; the barrier also publishes the trial point
            T Et;
            cl_block_eval<T, F>(N, tid, XT, red, par, Et, tx, ty, tz);      // its barrier: every thread has read XT
            if (Et < E) { dE = Et - E; E = Et; accepted = true; break; }   // :139-144
            t *= T(0.5);                                                    // :152
            if (++h >= a.max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (!accepted) {                                     // delta_point keeps the copy of :118
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) DX[c * N + i] = X[c * N + i];)
            break;
        }
#pragma unroll
        for (int q = 0; q < kClPer; ++q) {
            const int i = tid + kBlock * q;
            if (i < N) {
                const T tg[3] = {tx[q], ty[q], tz[q]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = c * N + i;
                    DX[e] = XT[e] - X[e]; DG[e] = tg[c] - G[e];   // :145, :306-308
                    X[e] = XT[e]; G[e] = tg[c];
                }
            }
        }
        ++it;                                                // :310
    }
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        gx_[e] = X[e]; gg_[e] = G[e]; gdx_[e] = DX[e]; gdg_[e] = DG[e];
    })
    if (tid == 0) {
        *gf_ = E; *gdf_ = dE;
        *gcur_ = cur; *gprev_ = prev;
        *gstuck_ = stuck ? 1 : 0;
        *git_ = it;
        *ghalv_ = halv;
    }
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void adgd_batch_block_step_kernel(AdgdBatchArgs<T> a) { adgd_batch_block_step_body<T, F>(a); }

}  // namespace dzo

using namespace dzo;

struct dzo_adgd_batch_s {
    ClCore core;                     // lds_bytes: BLOCK shape only
    void *cur = nullptr, *prev = nullptr;
};

namespace dzo {

static void ab_free(dzo_adgd_batch_s *h) { cl_free(h, {h->cur, h->prev}); }

template <typename T> static AdgdBatchArgs<T> ab_args(const dzo_adgd_batch_s *h, int steps, double step_length) {
    const ClCore &c = h->core;
    AdgdBatchArgs<T> a;
    a.N = c.N; a.steps = steps;
    a.max_halvings = c.max_halvings;
    a.step_length = (T)step_length;
    a.x = (T *)c.x; a.g = (T *)c.g; a.dx = (T *)c.dx; a.dg = (T *)c.dg;
    a.f = (T *)c.f; a.df = (T *)c.df; a.cur = (T *)h->cur; a.prev = (T *)h->prev;
    a.stuck = c.stuck; a.halv = c.halv; a.iters = c.iters;
    return a;
}

template <typename T, typename F> static void ab_launch_step(hipStream_t s, const dzo_adgd_batch_s *h, int steps) {
    const AdgdBatchArgs<T> a = ab_args<T>(h, steps, 0.0);
    const dim3 grid((unsigned)h->core.B);
    if (a.N <= 64) hipLaunchKernelGGL((adgd_batch_wave_step_kernel<T, F>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((adgd_batch_block_step_kernel<T, F>), grid, dim3(kBlock), h->core.lds_bytes, s, a);
}

// `what` -> device address, bytes
static int32_t ab_array(dzo_adgd_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const ClCore &c = h->core;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, n3 = 3 * (size_t)c.N;
    switch (what) {
    case DZO_ADGD_BATCH_POINTS: *p = c.x; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_GRADIENTS: *p = c.g; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_DELTA_POINTS: *p = c.dx; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_DELTA_GRADIENTS: *p = c.dg; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_OBJECTIVES: *p = c.f; *bytes = es * B; break;
    case DZO_ADGD_BATCH_DELTA_OBJECTIVES: *p = c.df; *bytes = es * B; break;
    case DZO_ADGD_BATCH_IS_STUCK: *p = c.stuck; *bytes = 4 * B; break;
    case DZO_ADGD_BATCH_ITERATION_COUNTS: *p = c.iters; *bytes = 8 * B; break;
    case DZO_ADGD_BATCH_CURRENT_STEP_SIZES: *p = h->cur; *bytes = es * B; break;
    case DZO_ADGD_BATCH_PREVIOUS_STEP_SIZES: *p = h->prev; *bytes = es * B; break;
    case DZO_ADGD_BATCH_LAST_HALVINGS: *p = c.halv; *bytes = 4 * B; break;
    default: set_error("unknown batched AdGD array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

// AdGDOptimizer(constraint_function! = nothing, ...), src/DZOptimization.jl:245-271 and :201-242, per instance
int32_t dzo_adgd_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, double initial_step_length,
                              dzo_adgd_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:229)");
    DZO_TRY(require_same_backend("AdGDOptimizer", "src/DZOptimization.jl:216-217", points_dev, "initial_point", nullptr, ""));
    dzo_adgd_batch_s *h = new (std::nothrow) dzo_adgd_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.radial = radial; c.N = (int)n_particles; c.B = batch; c.x = points_dev;
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles;
    if (n_particles > 64) c.lds_bytes = 16 * kWaves + 5 * n3 * es;
    int32_t rc = cl_alloc({{&c.g, es * n3 * B}, {&c.dx, es * n3 * B}, {&c.dg, es * n3 * B}, {&c.f, es * B}, {&c.df, es * B}, {&h->cur, es * B},
                           {&h->prev, es * B}, {(void **)&c.stuck, 4 * B}, {(void **)&c.halv, 4 * B}, {(void **)&c.iters, 8 * B},
                           {(void **)&c.active_dev, 8}},
                          "the batched AdGD state");
    const void *k = nullptr;                                  // the block step kernel of the handle's radial and element type
    if (rc == DZO_OK) rc = [&]() -> int32_t { DZO_DISPATCH_RADIAL(radial, dtype, k = (const void *)adgd_batch_block_step_kernel<T, F>); return DZO_OK; }();
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, k, "batched AdGD state", "batched AdGD constructor", [&](hipStream_t s) -> int32_t {
            DZO_TIMED("adgd_batch_init", s);
            // f0 and g0 by the evaluation kernels of dzo_pairwise_batch_energy_gradient, then the step sizes and is_stuck
            DZO_DISPATCH(dtype, DZO_TRY(cl_launch_eval<T>(s, radial, c.N, batch, (const T *)c.x, (T *)c.f, (T *)c.g)));
            DZO_DISPATCH(dtype, hipLaunchKernelGGL((adgd_batch_init_kernel<T>), dim3((unsigned)batch), dim3(kBlock), 0, s, ab_args<T>(h, 0, initial_step_length)));
            return DZO_OK;
        });
    if (rc != DZO_OK) { ab_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_adgd_batch_destroy(dzo_adgd_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    ab_free(h);
    return DZO_OK;
}

int32_t dzo_adgd_batch_set_max_halvings(dzo_adgd_batch_t h, int64_t max_halvings) { return cl_set_max_halvings(h, max_halvings); }

// step!(::AdGDOptimizer), src/DZOptimization.jl:274-312, `steps` times per instance
int32_t dzo_adgd_batch_step(dzo_adgd_batch_t h, int32_t steps, int32_t *all_stuck) {
    return cl_step(h, steps, all_stuck, [&](hipStream_t s) -> int32_t {
        DZO_TIMED("adgd_batch_step", s);
        DZO_DISPATCH_RADIAL(h->core.radial, h->core.dtype, (ab_launch_step<T, F>(s, h, steps)));
        DZO_HIP(hipGetLastError());
        return DZO_OK;
    });
}

int32_t dzo_adgd_batch_count_active(dzo_adgd_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_adgd_batch_get_ptr(dzo_adgd_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, ab_array, what, ptr_dev); }

int32_t dzo_adgd_batch_read(dzo_adgd_batch_t h, int32_t what, void *out_host) { return cl_read(h, ab_array, what, out_host); }

}  // extern "C"
