// dzo_cluster.h -- what the units that run MANY small Lennard-Jones clusters at once share: dzo_lbfgs_batch.hip, dzo_adgd_batch.hip,
// dzo_hessian_batch.hip, dzo_tempering.hip and dzo_basin_hopping.hip.  One definition each, the same bits in all of them.  Every name here starts with
// cl_ (functions), Cl (types), kCl (constants) or CL_ (the one macro).  The two launch shapes, WAVE (N <= 64, one wave per
// instance) and BLOCK (up to 1024 particles, one 256-thread block per instance), are described in dzo_lbfgs_batch.hip.
// A .hip that uses dynamic LDS declares its own `extern __shared__` array.
#pragma once
#include "dzo_pairwise.h"

#include <initializer_list>

namespace dzo {

constexpr int kClMaxN = DZO_LBFGS_BATCH_MAX_PARTICLES;
constexpr int kClPer = kClMaxN / kBlock;                     // particles a thread of the BLOCK shape owns at most
constexpr size_t kClLdsMax = 160 * 1024 - 1024;              // dynamic LDS of a step launch: the CU's 160 KiB less room for the static part

// ------------------------------------------------------------------------------ sums
// a lane's / thread's share of a dot over one particle, in fp64
template <typename T> __device__ __forceinline__ double cl_dot3(T ax, T ay, T az, T bx, T by, T bz) {
    double p = (double)ax * (double)bx;
    p = __builtin_fma((double)ay, (double)by, p);
    return __builtin_fma((double)az, (double)bz, p);
}

// |v|, the IEEE square root, and "neither infinite nor NaN" in the element type (the mode-following units)
template <typename T> __device__ __forceinline__ T cl_abs(T v);
template <> __device__ __forceinline__ double cl_abs<double>(double v) { return __builtin_fabs(v); }
template <> __device__ __forceinline__ float cl_abs<float>(float v) { return __builtin_fabsf(v); }
template <typename T> __device__ __forceinline__ T cl_sqrt(T v);
template <> __device__ __forceinline__ double cl_sqrt<double>(double v) { return __builtin_sqrt(v); }
template <> __device__ __forceinline__ float cl_sqrt<float>(float v) { return __builtin_sqrtf(v); }
template <typename T> __device__ __forceinline__ bool cl_finite(T v) { return cl_abs(v) < (T)__builtin_inf(); }   // false for NaN

// a block-wide sum in EVERY thread, fixed order (wave trees, then the four waves in wave order).  `red` holds 2 * kWaves doubles
// used alternately, so that one barrier per sum is enough (a wave can be at most one sum ahead of the slowest).
__device__ __forceinline__ double cl_block_sum(double v, double *red, int &par) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double w = wave_sum_all(v);
    if (lane == 0) red[par * kWaves + wv] = w;
    __syncthreads();
    double r = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) r += red[par * kWaves + k];
    par ^= 1;
    return r;
}

// two block-wide sums behind one barrier, in EVERY thread, in the same fixed order; `red` holds 2 * kWaves doubles.  The caller
// puts a barrier between the reads of one call and the next call.
__device__ __forceinline__ void cl_block_sum2(double &v0, double &v1, double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double w0 = wave_sum_all(v0), w1 = wave_sum_all(v1);
    if (lane == 0) { red[wv] = w0; red[kWaves + wv] = w1; }
    __syncthreads();
    double r0 = 0, r1 = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { r0 += red[k]; r1 += red[kWaves + k]; }
    v0 = r0; v1 = r1;
}

// The body for every particle i = tid + 256 q the thread owns in the BLOCK shape (`tid` and `N` are the caller's).  A macro: as
// a function template that takes a lambda, the block evaluation kernel and the step kernels compile to other code.
#define CL_FOR_OWN(i, ...)                                  \
    _Pragma("unroll") for (int q = 0; q < kClPer; ++q) { \
        const int i = tid + kBlock * q;                     \
        if (i < N) { __VA_ARGS__ }                          \
    }

// ------------------------------------------------------------------------------ energy and gradient of one point
// one (i, j) term: energy (:137-146) and gradient (:245-257) from the same r2 (dzo_pairwise.h); `drop` = self term or padding
template <typename T, typename F>
__device__ __forceinline__ void cl_pair(bool drop, T xi, T yi, T zi, T xj, T yj, T zj, T &row, T &ax, T &ay, T &az) {
    pw_pair<T, F, kPwEnergyGradient>(drop, PwPoint<T>{xi, yi, zi}, PwPoint<T>{xj, yj, zj}, ax, ay, az, &row);
}

// WAVE: energy in every lane, gradient of particle `lane` (zero in the lanes without a particle)
template <typename T, typename F>
__device__ __forceinline__ void cl_wave_eval(int N, int lane, T x, T y, T z, T &E, T &gx, T &gy, T &gz) {
    T row = T(0), ax = T(0), ay = T(0), az = T(0);
    // four independent pairs per trip; j4 + k <= 63 is a lane of the wave, the padding is dropped like the self term
    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j4 + k;
            cl_pair<T, F>(j == lane || j >= N, x, y, z, lane_read(x, j), lane_read(y, j), lane_read(z, j), row, ax, ay, az);
        }
    }
    const bool live = lane < N;
    E = (T)(0.5 * wave_sum_all(live ? (double)row : 0.0));
    gx = live ? pw_twice(ax) : T(0);
    gy = live ? pw_twice(ay) : T(0);
    gz = live ? pw_twice(az) : T(0);
}

// BLOCK: energy in every thread and the gradients of the thread's own particles, from the point X = [x | y | z] in LDS (complete
// and visible: the caller's barrier)
template <typename T, typename F>
__device__ __forceinline__ void cl_block_eval(int N, int tid, const T *X, double *red, int &par, T &E, T (&gx)[kClPer], T (&gy)[kClPer],
                                              T (&gz)[kClPer]) {
    double rows = 0;
#pragma unroll
    for (int q = 0; q < kClPer; ++q) {
        const int i = tid + kBlock * q;
        gx[q] = gy[q] = gz[q] = T(0);
        if (i < N) {
            const T xi = X[i], yi = X[N + i], zi = X[2 * N + i];
            T row = T(0), ax = T(0), ay = T(0), az = T(0);
            for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j4 + k, jc = j < N ? j : N - 1;   // the padding re-reads the last particle and is dropped
                    cl_pair<T, F>(j == i || j >= N, xi, yi, zi, X[jc], X[N + jc], X[2 * N + jc], row, ax, ay, az);
                }
            }
            rows += (double)row;
            gx[q] = pw_twice(ax); gy[q] = pw_twice(ay); gz[q] = pw_twice(az);
        }
    }
    E = (T)(0.5 * cl_block_sum(rows, red, par));
}

// ------------------------------------------------------------------------------ host side
// the argument checks of every entry point that takes `batch` clusters of N particles
inline int32_t cl_check_args(int32_t radial, int64_t N, int64_t batch, int32_t dtype) {
    return pw_check_args(radial, dtype, N, batch, "batch", kClMaxN, DZO_ERR_UNSUPPORTED, "the batched kernels hold an instance in one block");
}

// energy (f, one per instance) and, where g is not null, gradient of `batch` points on s: the evaluation kernels of
// dzo_lbfgs_batch.hip, which also defines the count below
template <typename T> int32_t cl_launch_eval(hipStream_t s, int32_t radial, int N, int64_t batch, const T *x, T *f, T *g);

// What the handles of the batched optimizers share; each embeds one as `core`.
struct ClCore {
    int device = -1;
    int32_t dtype = DZO_F64, radial = DZO_RADIAL_LENNARD_JONES;   // the radial of every later launch is the constructor's
    int N = 0;
    int64_t B = 0, max_halvings = 4096;
    void *x = nullptr;               // the caller's
    void *g = nullptr, *dx = nullptr, *dg = nullptr, *f = nullptr, *df = nullptr;
    int32_t *stuck = nullptr, *halv = nullptr;
    int64_t *iters = nullptr, *active_dev = nullptr, *active_host = nullptr;
    size_t lds_bytes = 0;
};

// instances that are not stuck; waits for the stream
int32_t cl_count_active(ClCore *c, hipStream_t s, int64_t *active);

struct ClPiece { void **p; size_t bytes; };

// every piece (but one with p null), cleared, in order; stops at the first that fails (the caller then frees the handle)
inline int32_t cl_alloc(std::initializer_list<ClPiece> pieces, const char *what_for) {
    for (const ClPiece &q : pieces)
        if (q.p) DZO_TRY(device_alloc(q.p, q.bytes, what_for, true));
    return DZO_OK;
}

// the core's arrays and the handle's own (`more`), then the handle
template <typename H> void cl_free(H *h, std::initializer_list<void *> more) {
    ClCore &c = h->core;
    for (void *q : {c.g, c.dx, c.dg, c.f, c.df, (void *)c.stuck, (void *)c.halv, (void *)c.iters, (void *)c.active_dev})
        if (q) (void)hipFree(q);
    for (void *q : more)
        if (q) (void)hipFree(q);
    if (c.active_host) (void)hipHostFree(c.active_host);
    delete h;
}

// The constructor behind the allocations: the pinned word of the count, the LDS attribute of `step_kernel`, then `init` (f0, g0
// and the rest of the reference's constructor, enqueued under the caller's timer) and a wait.  `state` and `ctor` name the two
// stages in a HIP failure's message.
template <typename Init> int32_t cl_finish_create(ClCore *c, const void *step_kernel, const char *state, const char *ctor, Init init) {
    hipStream_t s = ctx().stream;
    hipError_t e = hipHostMalloc((void **)&c->active_host, sizeof(int64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipDeviceSynchronize();          // the memsets of cl_alloc ran on the null stream
    // gfx950 has 160 KiB of LDS per CU; dynamic requests above the default need the attribute.  It belongs to the kernel, not
    // to the handle: it is raised to the limit, so that a later handle with a smaller request does not lower it for this one
    if (e == hipSuccess && c->lds_bytes > 48 * 1024) e = hipFuncSetAttribute(step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClLdsMax);
    if (e != hipSuccess) return hip_fail(e, state, __FILE__, __LINE__);
    DZO_TRY(init(s));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, ctor, __FILE__, __LINE__);
    return DZO_OK;
}

// the project's bounded-halvings escape of the loop of :121-153 (dzo_lbfgs_set_max_halvings); at least 1 here
template <typename H> int32_t cl_set_max_halvings(H *h, int64_t max_halvings) {
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(max_halvings >= 1, DZO_ERR_INVALID, "max_halvings must be at least 1 (got %lld): a launch cannot search without bound", (long long)max_halvings);
    h->core.max_halvings = max_halvings;
    return DZO_OK;
}

// `steps` calls of step!() per instance through launch(stream) (the caller's timer and kernels), then the count where asked for
template <typename H, typename Launch> int32_t cl_step(H *h, int32_t steps, int32_t *all_stuck, Launch launch) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(steps >= 0, DZO_ERR_INVALID, "steps must not be negative (got %d)", steps);
    DeviceScope scope(h->core.device);
    hipStream_t s = ctx().stream;
    if (steps > 0) DZO_TRY(launch(s));
    if (all_stuck) {
        int64_t active = 0;
        DZO_TRY(cl_count_active(&h->core, s, &active));
        *all_stuck = active == 0 ? 1 : 0;
    }
    return DZO_OK;
}

template <typename H> int32_t cl_count(H *h, int64_t *active) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && active, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->core.device);
    return cl_count_active(&h->core, ctx().stream, active);
}

// array(h, what, &pointer, &bytes) is the handle's table of its device arrays
template <typename H, typename Array> int32_t cl_get_ptr(H *h, Array array, int32_t what, void **ptr_dev) {
    DZO_REQUIRE(h && ptr_dev, DZO_ERR_INVALID, "null argument");
    size_t bytes = 0;
    return array(h, what, ptr_dev, &bytes);
}

template <typename H, typename Array> int32_t cl_read(H *h, Array array, int32_t what, void *out_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && out_host, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->core.device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(array(h, what, &p, &bytes));
    return copy_blocking(out_host, p, bytes, hipMemcpyDeviceToHost);
}

}  // namespace dzo
