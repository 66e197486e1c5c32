// dzo_lbfgs_batch.hip -- the live LBFGSOptimizer (src/DZOptimization.jl:321-509) over MANY small Lennard-Jones clusters on gfx950.
//
// The reference's step!() on a 3N-variable cluster is a chain of small vector operations with a host decision per trial
// (take_backtracking_step!, :107-154).  Through dzo_lbfgs_* that is a chain of launches and a host wait per trial of ONE
// cluster.  Here one launch runs `steps` calls of step!() of EVERY instance, and nothing crosses the host in between:
//
//   * WAVE shape (N <= 64): one wave per instance (a block of 64 threads).  Lane i holds particle i; point, gradient,
//     direction and both deltas are registers.  The pair loop takes particle j from lane j through v_readlane, four
//     independent pairs per trip; energy and dots go through wave_sum_all.  No barrier.  The (s, y) history is a ring in
//     LDS (2 m 3 values per lane; history_length is a run-time value up to 32, which registers cannot index).
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per instance, thread t owns particles t, t + 256, ...  The five
//     vectors are in LDS (only their owner touches an element, except the trial point, which the pair loop reads as a
//     broadcast), the trial gradient in registers.  The history ring is in LDS where it fits the 160 KiB, else in a
//     handle-owned global slab.
//
// The step loop of either shape and the constructor's first direction are the device functions of dzo_quench_core.h (the
// kernels here are load -> run -> store around them; dzo_basin_hopping.hip runs them once per hop).
// The shapes' shared pieces (the evaluation of a trial, the block sums and dots, the owner loop, the handle's host core) are in
// dzo_cluster.h; dzo_adgd_batch.hip is the second optimizer on them.  The evaluation and count-active kernels and their launchers
// are defined here for both.  Per pair the arithmetic is dzo_pairwise.hip's: pw_pair of dzo_pairwise.h (the self term removed
// by a select); energy and gradient of a trial come out of ONE pair loop (they share the reciprocal).  Row sums over j run
// j = 0 .. N-1 in T, rows are added in fp64 by the fixed trees of dzo_common.h, one rounding back to T; dots accumulate in fp64
// in a fixed order that depends on N only.  No floating-point atomic.  The recursion is the chain form of :430-451.
#include "dzo_cluster.h"
#include "dzo_quench_core.h"
#include "dzo_quench_args.h"

#include <cmath>
#include <new>

namespace dzo {

constexpr int kQuenchMaxM = DZO_LBFGS_BATCH_MAX_HISTORY;

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
// (each kernel of this file is its body as a __device__ function and the entry point that calls it: written into the
// __global__ function itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
template <typename T, typename F> __device__ __forceinline__ void quench_wave_eval_body(QuenchArgs<T> a) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    const bool live = lane < N;
    const T x = live ? a.x[base + lane] : T(0), y = live ? a.x[base + N + lane] : T(0), z = live ? a.x[base + 2 * N + lane] : T(0);
    T E, gx, gy, gz;
    cl_wave_eval<T, F>(N, lane, x, y, z, E, gx, gy, gz);
    if (lane == 0) a.f[b] = E;
    if (a.g && live) { a.g[base + lane] = gx; a.g[base + N + lane] = gy; a.g[base + 2 * N + lane] = gz; }
    if (!a.init) return;
    T px, py, pz;
    const bool stuck = qc_wave_first_direction<T>(a.step_length, gx, gy, gz, px, py, pz);   // :381-387
    if (live) { a.d[base + lane] = px; a.d[base + N + lane] = py; a.d[base + 2 * N + lane] = pz; }
    if (lane == 0) a.stuck[b] = stuck ? 1 : 0;
}
template <typename T, typename F> __global__ __launch_bounds__(64) void quench_wave_eval_kernel(QuenchArgs<T> a) { quench_wave_eval_body<T, F>(a); }

extern __shared__ __attribute__((aligned(16))) double quench_smem[];

template <typename T, typename F> __device__ __forceinline__ void quench_wave_step_body(QuenchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // :456, the whole wave
    const int lane = threadIdx.x, N = a.N, m = a.m;
    const int64_t base = (int64_t)3 * N * b;
    const bool live = lane < N;
    auto ld = [&](const T *p, int c) { return live ? p[base + c * N + lane] : T(0); };
    QcWave<T> w;
    w.x = ld(a.x, 0); w.y = ld(a.x, 1); w.z = ld(a.x, 2);
    w.gx = ld(a.g, 0); w.gy = ld(a.g, 1); w.gz = ld(a.g, 2);
    w.px = ld(a.d, 0); w.py = ld(a.d, 1); w.pz = ld(a.d, 2);
    w.sx = ld(a.dx, 0); w.sy = ld(a.dx, 1); w.sz = ld(a.dx, 2);
    w.yx = ld(a.dg, 0); w.yy = ld(a.dg, 1); w.yz = ld(a.dg, 2);
    w.E = a.f[b]; w.dE = a.df[b];
    w.it = a.iters[b];
    w.hc = a.hcount[b]; w.halv = a.halv[b]; w.head = 0;
    const int hc0 = w.hc;
    // LDS: rho[m] | alpha[m] | S ring | Y ring; element (slot p, component c) of this lane at (p * 3 + c) * 64 + lane
    double *rho = quench_smem, *alpha = rho + m;
    T *hS = reinterpret_cast<T *>(alpha + m), *hY = hS + m * 3 * 64;
    const int64_t hbase = (int64_t)3 * N * m * b;
    for (int k = 0; k < hc0; ++k) {
        rho[k] = a.rho[(int64_t)m * b + k];                  // every lane the same value to the same address
        for (int c = 0; c < 3; ++c) {
            hS[(k * 3 + c) * 64 + lane] = live ? a.S[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
            hY[(k * 3 + c) * 64 + lane] = live ? a.Y[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
        }
    }
    const bool stuck = qc_wave_run<T, F>(N, m, lane, a.steps, a.max_halvings, w, rho, alpha, hS, hY);
    const int hc = w.hc, head = w.head;
    if (live) {
        auto st = [&](T *p, int c, T v) { p[base + c * N + lane] = v; };
        st(a.x, 0, w.x); st(a.x, 1, w.y); st(a.x, 2, w.z);
        st(a.g, 0, w.gx); st(a.g, 1, w.gy); st(a.g, 2, w.gz);
        st(a.d, 0, w.px); st(a.d, 1, w.py); st(a.d, 2, w.pz);
        st(a.dx, 0, w.sx); st(a.dx, 1, w.sy); st(a.dx, 2, w.sz);
        st(a.dg, 0, w.yx); st(a.dg, 1, w.yy); st(a.dg, 2, w.yz);
        for (int k = 0; k < hc; ++k) {
            const int p = head + k < m ? head + k : head + k - m;
            for (int c = 0; c < 3; ++c) {
                a.S[hbase + (int64_t)3 * N * k + c * N + lane] = hS[(p * 3 + c) * 64 + lane];
                a.Y[hbase + (int64_t)3 * N * k + c * N + lane] = hY[(p * 3 + c) * 64 + lane];
            }
        }
    }
    if (lane < hc) a.rho[(int64_t)m * b + lane] = rho[head + lane < m ? head + lane : head + lane - m];
    if (lane == 0) {
        a.f[b] = w.E; a.df[b] = w.dE;
        a.stuck[b] = stuck ? 1 : 0;
        a.iters[b] = w.it;
        a.hcount[b] = hc; a.halv[b] = w.halv;
    }
}
template <typename T, typename F> __global__ __launch_bounds__(64) void quench_wave_step_kernel(QuenchArgs<T> a) { quench_wave_step_body<T, F>(a); }

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
template <typename T, typename F> __device__ __forceinline__ void quench_block_eval_body(QuenchArgs<T> a) {
    __shared__ T X[3 * kClMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    for (int e = tid; e < 3 * N; e += kBlock) X[e] = a.x[base + e];
    __syncthreads();
    int par = 0;
    T E, gx[kClPer], gy[kClPer], gz[kClPer];
    cl_block_eval<T, F>(N, tid, X, red, par, E, gx, gy, gz);
    if (tid == 0) a.f[b] = E;
    if (a.g) { CL_FOR_OWN(i, a.g[base + i] = gx[q]; a.g[base + N + i] = gy[q]; a.g[base + 2 * N + i] = gz[q];) }
    if (!a.init) return;
    bool stuck;
    const T sc = qc_block_first_scale<T>(N, tid, a.step_length, gx, gy, gz, red, par, stuck);   // :381-387
    CL_FOR_OWN(i, {
        a.d[base + i] = stuck ? T(0) : sc * gx[q];
        a.d[base + N + i] = stuck ? T(0) : sc * gy[q];
        a.d[base + 2 * N + i] = stuck ? T(0) : sc * gz[q];
    })
    if (tid == 0) a.stuck[b] = stuck ? 1 : 0;
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void quench_block_eval_kernel(QuenchArgs<T> a) { quench_block_eval_body<T, F>(a); }

// HL: the history ring is in LDS (else in a.slab)
template <typename T, typename F, bool HL> __device__ __forceinline__ void quench_block_step_body(QuenchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // the whole block
    const int tid = threadIdx.x, N = a.N, m = a.m, n3 = 3 * N;
    const int64_t base = (int64_t)n3 * b, hbase = (int64_t)n3 * m * b;
    // LDS: rho[m] | alpha[m] | red[2 kWaves] | X | G | D | DX | DG | (S ring | Y ring)
    double *rho = quench_smem, *alpha = rho + m, *red = alpha + m;
    T *X = reinterpret_cast<T *>(red + 2 * kWaves), *G = X + n3, *D = G + n3, *DX = D + n3, *DG = DX + n3;
    T *hS, *hY;
    if constexpr (HL) { hS = DG + n3; hY = hS + (size_t)m * n3; }
    else { hS = a.slab + 2 * hbase; hY = hS + (size_t)m * n3; }
    T *const gx_ = pw_pin_ptr(a.x + base), *const gg_ = pw_pin_ptr(a.g + base), *const gd_ = pw_pin_ptr(a.d + base);
    T *const gdx_ = pw_pin_ptr(a.dx + base), *const gdg_ = pw_pin_ptr(a.dg + base);
    T *const gS_ = pw_pin_ptr(a.S + hbase), *const gY_ = pw_pin_ptr(a.Y + hbase), *const gf_ = pw_pin_ptr(a.f + b), *const gdf_ = pw_pin_ptr(a.df + b);
    double *const grho_ = pw_pin_ptr(a.rho + (int64_t)m * b);
    int32_t *const gstuck_ = pw_pin_ptr(a.stuck + b), *const ghc_ = pw_pin_ptr(a.hcount + b), *const ghalv_ = pw_pin_ptr(a.halv + b);
    int64_t *const git_ = pw_pin_ptr(a.iters + b);
    QcBlock<T> w{X, G, D, DX, DG, hS, hY, rho, alpha, red, *gf_, *gdf_, *git_, *ghc_, *ghalv_, 0, 0};
    const int hc0 = w.hc;
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        X[e] = gx_[e]; G[e] = gg_[e]; D[e] = gd_[e]; DX[e] = gdx_[e]; DG[e] = gdg_[e];
        for (int k = 0; k < hc0; ++k) { hS[k * n3 + e] = gS_[(int64_t)n3 * k + e]; hY[k * n3 + e] = gY_[(int64_t)n3 * k + e]; }
    })
    for (int k = 0; k < hc0; ++k) rho[k] = grho_[k];   // every thread the same value to the same address
    const bool stuck = qc_block_run<T, F>(N, m, tid, a.steps, a.max_halvings, w);
    const int hc = w.hc, head = w.head;
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        gx_[e] = X[e]; gg_[e] = G[e]; gd_[e] = D[e]; gdx_[e] = DX[e]; gdg_[e] = DG[e];
    })
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        for (int k = 0; k < hc; ++k) {
            const int p = head + k < m ? head + k : head + k - m;
            gS_[(int64_t)n3 * k + e] = hS[p * n3 + e];
            gY_[(int64_t)n3 * k + e] = hY[p * n3 + e];
        }
    })
    if (tid < hc) grho_[tid] = rho[head + tid < m ? head + tid : head + tid - m];
    if (tid == 0) {
        *gf_ = w.E; *gdf_ = w.dE;
        *gstuck_ = stuck ? 1 : 0;
        *git_ = w.it;
        *ghc_ = hc; *ghalv_ = w.halv;
    }
}
template <typename T, typename F, bool HL> __global__ __launch_bounds__(kBlock) void quench_block_step_kernel(QuenchArgs<T> a) { quench_block_step_body<T, F, HL>(a); }

// instances that are not stuck: one block, integer sums
__global__ __launch_bounds__(kBlock) void quench_count_active_kernel(int64_t batch, const int32_t *__restrict__ stuck, int64_t *__restrict__ out) {
    __shared__ unsigned long long total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned long long c = 0;
    for (int64_t k = threadIdx.x; k < batch; k += kBlock) c += stuck[k] ? 0 : 1;
    atomicAdd(&total, c);                                    // integers: the order does not matter
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (int64_t)total;
}

}  // namespace dzo

using namespace dzo;

struct dzo_lbfgs_batch_s : QaHandle {};                      // ClCore plus the ring arrays (dzo_quench_args.h)

namespace dzo {

template <typename T, typename F> static void qb_launch_eval(hipStream_t s, int64_t batch, const QuenchArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((quench_wave_eval_kernel<T, F>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((quench_block_eval_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

template <typename T> int32_t cl_launch_eval(hipStream_t s, int32_t radial, int N, int64_t batch, const T *x, T *f, T *g) {
    QuenchArgs<T> a{};
    a.N = N; a.x = const_cast<T *>(x); a.f = f; a.g = g;
    DZO_RADIAL_CASES_(radial, (qb_launch_eval<T, F>(s, batch, a)))
    return DZO_OK;
}
template int32_t cl_launch_eval<double>(hipStream_t, int32_t, int, int64_t, const double *, double *, double *);
template int32_t cl_launch_eval<float>(hipStream_t, int32_t, int, int64_t, const float *, float *, float *);

template <typename T, typename F> static const void *qb_step_kernel(const dzo_lbfgs_batch_s *h) {
    if (h->core.N <= 64) return (const void *)quench_wave_step_kernel<T, F>;
    return h->hist_lds ? (const void *)quench_block_step_kernel<T, F, true> : (const void *)quench_block_step_kernel<T, F, false>;
}

template <typename T, typename F> static void qb_launch_step(hipStream_t s, const dzo_lbfgs_batch_s *h, int steps) {
    const QuenchArgs<T> a = qa_args<T>(h, steps, 0, 0.0);
    const dim3 grid((unsigned)h->core.B);
    const size_t lds = h->core.lds_bytes;
    if (a.N <= 64) hipLaunchKernelGGL((quench_wave_step_kernel<T, F>), grid, dim3(64), lds, s, a);
    else if (h->hist_lds) hipLaunchKernelGGL((quench_block_step_kernel<T, F, true>), grid, dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((quench_block_step_kernel<T, F, false>), grid, dim3(kBlock), lds, s, a);
}

int32_t cl_count_active(ClCore *c, hipStream_t s, int64_t *active) {
    hipLaunchKernelGGL(quench_count_active_kernel, dim3(1), dim3(kBlock), 0, s, c->B, (const int32_t *)c->stuck, c->active_dev);
    DZO_HIP(hipGetLastError());
    DZO_HIP(hipMemcpyAsync(c->active_host, c->active_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DZO_HIP(hipStreamSynchronize(s));
    *active = c->active_host[0];
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

// LBFGSOptimizer(constraint_function! = nothing, ...), src/DZOptimization.jl:400-427 and :347-397, per instance
int32_t dzo_lbfgs_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, double initial_step_length,
                               int32_t history_length, dzo_lbfgs_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    DZO_REQUIRE(history_length >= 1, DZO_ERR_INVALID, "history_length must be at least 1 (got %d)", history_length);
    DZO_REQUIRE(history_length <= kQuenchMaxM, DZO_ERR_UNSUPPORTED, "history_length = %d: the batched kernels keep up to %d pairs", history_length,
                kQuenchMaxM);
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:380)");
    DZO_TRY(require_same_backend("LBFGSOptimizer", "src/DZOptimization.jl:363-364", points_dev, "initial_point", nullptr, ""));
    dzo_lbfgs_batch_s *h = new (std::nothrow) dzo_lbfgs_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.radial = radial; c.N = (int)n_particles; c.B = batch; c.x = points_dev;
    int32_t rc = qa_alloc(h, history_length);
    const void *step_kernel = nullptr;
    if (rc == DZO_OK) rc = [&]() -> int32_t { DZO_DISPATCH_RADIAL(radial, dtype, step_kernel = (qb_step_kernel<T, F>(h))); return DZO_OK; }();
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, step_kernel, "batched L-BFGS state", "batched L-BFGS constructor", [&](hipStream_t s) -> int32_t {
            DZO_TIMED("lbfgs_batch_init", s);
            DZO_DISPATCH_RADIAL(radial, dtype, (qb_launch_eval<T, F>(s, batch, qa_args<T>(h, 0, 1, initial_step_length))));
            return DZO_OK;
        });
    if (rc != DZO_OK) { qa_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_lbfgs_batch_destroy(dzo_lbfgs_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    qa_free(h);
    return DZO_OK;
}

int32_t dzo_lbfgs_batch_set_max_halvings(dzo_lbfgs_batch_t h, int64_t max_halvings) { return cl_set_max_halvings(h, max_halvings); }

// step!(::LBFGSOptimizer), src/DZOptimization.jl:454-509, `steps` times per instance
int32_t dzo_lbfgs_batch_step(dzo_lbfgs_batch_t h, int32_t steps, int32_t *all_stuck) {
    return cl_step(h, steps, all_stuck, [&](hipStream_t s) -> int32_t {
        DZO_TIMED("lbfgs_batch_step", s);
        DZO_DISPATCH_RADIAL(h->core.radial, h->core.dtype, (qb_launch_step<T, F>(s, h, steps)));
        DZO_HIP(hipGetLastError());
        return DZO_OK;
    });
}

int32_t dzo_lbfgs_batch_count_active(dzo_lbfgs_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_lbfgs_batch_get_ptr(dzo_lbfgs_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, qa_array, what, ptr_dev); }

int32_t dzo_lbfgs_batch_read(dzo_lbfgs_batch_t h, int32_t what, void *out_host) { return cl_read(h, qa_array, what, out_host); }

// objective_function and gradient_function! of every instance (:416-421), by the optimizer's own device routine
int32_t dzo_pairwise_batch_energy_gradient(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                           void *energies_dev, void *gradients_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && energies_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    const char *where = "LBFGSOptimizer", *cite = "src/DZOptimization.jl:410-420";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", energies_dev, "energies"));
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", gradients_dev, "gradients"));
    Context &c = ctx();
    {
        DZO_TIMED("pairwise_batch_energy_gradient", c.stream);
        DZO_DISPATCH(dtype, DZO_TRY(cl_launch_eval<T>(c.stream, radial, (int)n_particles, batch, (const T *)points_dev, (T *)energies_dev, (T *)gradients_dev)));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

}  // extern "C"
