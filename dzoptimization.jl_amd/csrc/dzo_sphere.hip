// dzo_sphere.hip -- the Thomson problem on gfx950: the Riesz (Coulomb, s = 1) energy of N points on the unit sphere
// (legacy/ExampleFunctions.jl: riesz_energy :30-45, riesz_gradient! :47-83, constrain_riesz_gradient_sphere! :361-374) and the live
// LBFGSOptimizer (src/DZOptimization.jl:321-509) WITH its constraint hook (constraint_function!, :133-135 and :412-414) over MANY
// configurations in one launch.
//
// The constrained counterpart of dzo_lbfgs_batch.hip, on the same pieces: the pair loop of dzo_cluster.h with the functor
// RieszRadial of dzo_pairwise.h, the step loops qc_wave_run / qc_block_run of dzo_quench_core.h with the policy QcUnitSphere as
// their last template argument, the load and store halves, the handle and the LDS layout of dzo_quench_args.h.  The launch shapes
// (WAVE: N <= 64, one wave per instance; BLOCK: one 256-thread block per instance, the ring in LDS where it fits, else in the slab)
// and the summation orders are those described in dzo_lbfgs_batch.hip.  The functor is not a DZO_RADIAL_*: it is used by the
// kernels of this file only, every one of which starts with sphere_.  No floating-point atomic.
#include "dzo_cluster.h"
#include "dzo_quench_core.h"
#include "dzo_quench_args.h"

#include <cmath>
#include <new>

namespace dzo {

constexpr int kSphereMaxM = DZO_LBFGS_BATCH_MAX_HISTORY;

// ------------------------------------------------------------------------------ project: grid over particles, block 256
// (each kernel of this file is its body as a __device__ function and the entry point that calls it, as in dzo_lbfgs_batch.hip)
template <typename T> __device__ __forceinline__ void sphere_project_body(int N, int64_t batch, T *p) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= (int64_t)N * batch) return;
    const int64_t b = k / N, base = (int64_t)3 * N * b + (k - b * N);
    T x = p[base], y = p[base + N], z = p[base + 2 * N];
    QcUnitSphere::project<T>(true, x, y, z);
    p[base] = x; p[base + N] = y; p[base + 2 * N] = z;
}
template <typename T> __global__ __launch_bounds__(kBlock) void sphere_project_kernel(int N, int64_t batch, T *p) { sphere_project_body<T>(N, batch, p); }

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
// energy and gradient (raw, or tangent: constrain_riesz_gradient_sphere!) of a point; with a.init the constructor's state (:381-397)
template <typename T> __device__ __forceinline__ void sphere_wave_eval_body(QuenchArgs<T> a, int tangent) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    const bool live = lane < N;
    const T x = live ? a.x[base + lane] : T(0), y = live ? a.x[base + N + lane] : T(0), z = live ? a.x[base + 2 * N + lane] : T(0);
    T E, gx, gy, gz;
    cl_wave_eval<T, RieszRadial<T>>(N, lane, x, y, z, E, gx, gy, gz);
    if (tangent) QcUnitSphere::tangent<T>(x, y, z, gx, gy, gz);
    if (lane == 0) a.f[b] = E;
    if (a.g && live) { a.g[base + lane] = gx; a.g[base + N + lane] = gy; a.g[base + 2 * N + lane] = gz; }
    if (!a.init) return;
    T px, py, pz;
    const bool stuck = qc_wave_first_direction<T>(a.step_length, gx, gy, gz, px, py, pz);   // :381-387
    if (live) { a.d[base + lane] = px; a.d[base + N + lane] = py; a.d[base + 2 * N + lane] = pz; }
    if (lane == 0) a.stuck[b] = stuck ? 1 : 0;
}
template <typename T> __global__ __launch_bounds__(64) void sphere_wave_eval_kernel(QuenchArgs<T> a, int tangent) { sphere_wave_eval_body<T>(a, tangent); }

extern __shared__ __attribute__((aligned(16))) double sphere_smem[];

template <typename T> __device__ __forceinline__ void sphere_wave_quench_body(QuenchArgs<T> a) {
    if (a.stuck[blockIdx.x]) return;                         // :456, the whole wave
    const int lane = threadIdx.x, N = a.N, m = a.m;
    QcWave<T> w;
    double *rho, *alpha;
    T *hS, *hY;
    qa_wave_lds<T>(sphere_smem, m, rho, alpha, hS, hY);
    qa_wave_load<T>(a, w, rho, hS, hY);
    const bool stuck = qc_wave_run<T, RieszRadial<T>, QcUnitSphere>(N, m, lane, a.steps, a.max_halvings, w, rho, alpha, hS, hY);
    qa_wave_store<T>(a, w, stuck, rho, hS, hY);
}
template <typename T> __global__ __launch_bounds__(64) void sphere_wave_quench_kernel(QuenchArgs<T> a) { sphere_wave_quench_body<T>(a); }

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
template <typename T> __device__ __forceinline__ void sphere_block_eval_body(QuenchArgs<T> a, int tangent) {
    __shared__ T X[3 * kClMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    for (int e = tid; e < 3 * N; e += kBlock) X[e] = a.x[base + e];
    __syncthreads();
    int par = 0;
    T E, gx[kClPer], gy[kClPer], gz[kClPer];
    cl_block_eval<T, RieszRadial<T>>(N, tid, X, red, par, E, gx, gy, gz);
    if (tangent) { CL_FOR_OWN(i, QcUnitSphere::tangent<T>(X[i], X[N + i], X[2 * N + i], gx[q], gy[q], gz[q]);) }
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
template <typename T> __global__ __launch_bounds__(kBlock) void sphere_block_eval_kernel(QuenchArgs<T> a, int tangent) { sphere_block_eval_body<T>(a, tangent); }

// HL: the history ring is in LDS (else in a.slab)
template <typename T, bool HL> __device__ __forceinline__ void sphere_block_quench_body(QuenchArgs<T> a) {
    if (a.stuck[blockIdx.x]) return;                         // the whole block
    const int tid = threadIdx.x, N = a.N, m = a.m;
    const QaBlockPtrs<T> g = qa_block_pin<T>(a);
    QcBlock<T> w = qa_block_place<T, HL>(a, g, sphere_smem);
    qa_block_load<T>(a, g, w);
    const bool stuck = qc_block_run<T, RieszRadial<T>, QcUnitSphere>(N, m, tid, a.steps, a.max_halvings, w);
    qa_block_store<T>(a, g, w, stuck);
}
template <typename T, bool HL> __global__ __launch_bounds__(kBlock) void sphere_block_quench_kernel(QuenchArgs<T> a) { sphere_block_quench_body<T, HL>(a); }

}  // namespace dzo

using namespace dzo;

struct dzo_sphere_lbfgs_batch_s : QaHandle {};               // ClCore plus the ring arrays, exactly as dzo_lbfgs_batch_s

namespace dzo {

static int32_t sphere_check_args(int32_t energy, int64_t N, int64_t batch, int32_t dtype) {
    DZO_REQUIRE(energy == DZO_SPHERE_ENERGY_RIESZ1, DZO_ERR_INVALID, "unknown sphere energy %d", energy);
    // The unit has no radial.  cl_check_args checks one first, so it is handed a valid constant and what it then checks is the
    // dtype, the sizes and the particle limit; ClCore.radial of a sphere handle stays at its default and nothing reads it.
    return cl_check_args(DZO_RADIAL_LENNARD_JONES, N, batch, dtype);
}

template <typename T> static void sphere_launch_project(hipStream_t s, int N, int64_t batch, T *p) {
    const int64_t blocks = ((int64_t)N * batch + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((sphere_project_kernel<T>), dim3((unsigned)blocks), dim3(kBlock), 0, s, N, batch, p);
}

template <typename T> static void sphere_launch_eval(hipStream_t s, int64_t batch, const QuenchArgs<T> &a, int tangent) {
    if (a.N <= 64) hipLaunchKernelGGL((sphere_wave_eval_kernel<T>), dim3((unsigned)batch), dim3(64), 0, s, a, tangent);
    else hipLaunchKernelGGL((sphere_block_eval_kernel<T>), dim3((unsigned)batch), dim3(kBlock), 0, s, a, tangent);
}

template <typename T> static const void *sphere_quench_kernel(const dzo_sphere_lbfgs_batch_s *h) {
    if (h->core.N <= 64) return (const void *)sphere_wave_quench_kernel<T>;
    return h->hist_lds ? (const void *)sphere_block_quench_kernel<T, true> : (const void *)sphere_block_quench_kernel<T, false>;
}

template <typename T> static void sphere_launch_quench(hipStream_t s, const dzo_sphere_lbfgs_batch_s *h, int steps) {
    const QuenchArgs<T> a = qa_args<T>(h, steps, 0, 0.0);
    const dim3 grid((unsigned)h->core.B);
    const size_t lds = h->core.lds_bytes;
    if (a.N <= 64) hipLaunchKernelGGL((sphere_wave_quench_kernel<T>), grid, dim3(64), lds, s, a);
    else if (h->hist_lds) hipLaunchKernelGGL((sphere_block_quench_kernel<T, true>), grid, dim3(kBlock), lds, s, a);
    else hipLaunchKernelGGL((sphere_block_quench_kernel<T, false>), grid, dim3(kBlock), lds, s, a);
}

}  // namespace dzo

extern "C" {

// constraint_function! of every particle, in place: p / |p|
int32_t dzo_sphere_batch_project(int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(sphere_check_args(DZO_SPHERE_ENERGY_RIESZ1, n_particles, batch, dtype));
    DZO_TRY(require_same_backend("LBFGSOptimizer", "src/DZOptimization.jl:363-364", points_dev, "points", nullptr, ""));
    Context &c = ctx();
    {
        DZO_TIMED("sphere_batch_project", c.stream);
        DZO_DISPATCH(dtype, (sphere_launch_project<T>(c.stream, (int)n_particles, batch, (T *)points_dev)));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// riesz_energy (:30-45) and riesz_gradient! (:47-83), with tangent constrain_riesz_gradient_sphere! (:361-374), of every instance
int32_t dzo_sphere_batch_energy_gradient(int32_t energy, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                         void *energies_dev, void *gradients_dev, int32_t tangent) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && energies_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(sphere_check_args(energy, n_particles, batch, dtype));
    DZO_REQUIRE(tangent == 0 || tangent == 1, DZO_ERR_INVALID, "tangent must be 0 or 1 (got %d)", tangent);
    const char *where = "LBFGSOptimizer", *cite = "src/DZOptimization.jl:410-420";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", energies_dev, "energies"));
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", gradients_dev, "gradients"));
    Context &c = ctx();
    {
        DZO_TIMED("sphere_batch_energy_gradient", c.stream);
        DZO_DISPATCH(dtype, {
            QuenchArgs<T> a{};
            a.N = (int)n_particles; a.x = const_cast<T *>((const T *)points_dev); a.f = (T *)energies_dev; a.g = (T *)gradients_dev;
            sphere_launch_eval<T>(c.stream, batch, a, tangent);
        });
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// LBFGSOptimizer(constraint_function!, f, g!, initial_point, ...), src/DZOptimization.jl:400-427 and :347-397, per instance: the
// initial point is projected in place (:412-414; the projection always succeeds)
int32_t dzo_sphere_lbfgs_batch_create(int32_t energy, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                      double initial_step_length, int32_t history_length, dzo_sphere_lbfgs_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(sphere_check_args(energy, n_particles, batch, dtype));
    DZO_REQUIRE(history_length >= 1, DZO_ERR_INVALID, "history_length must be at least 1 (got %d)", history_length);
    DZO_REQUIRE(history_length <= kSphereMaxM, DZO_ERR_UNSUPPORTED, "history_length = %d: the batched kernels keep up to %d pairs", history_length,
                kSphereMaxM);
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:380)");
    DZO_TRY(require_same_backend("LBFGSOptimizer", "src/DZOptimization.jl:363-364", points_dev, "initial_point", nullptr, ""));
    dzo_sphere_lbfgs_batch_s *h = new (std::nothrow) dzo_sphere_lbfgs_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.N = (int)n_particles; c.B = batch; c.x = points_dev;   // c.radial: unused here
    int32_t rc = qa_alloc(h, history_length);
    const void *step_kernel = nullptr;
    if (rc == DZO_OK) rc = [&]() -> int32_t { DZO_DISPATCH(dtype, step_kernel = (sphere_quench_kernel<T>(h))); return DZO_OK; }();
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, step_kernel, "batched sphere L-BFGS state", "batched sphere L-BFGS constructor", [&](hipStream_t s) -> int32_t {
            DZO_TIMED("sphere_lbfgs_batch_init", s);
            DZO_DISPATCH(dtype, {
                sphere_launch_project<T>(s, c.N, batch, (T *)points_dev);                           // :412-414
                sphere_launch_eval<T>(s, batch, qa_args<T>(h, 0, 1, initial_step_length), 1);       // f0, tangent g0, :381-387
            });
            return DZO_OK;
        });
    if (rc != DZO_OK) { qa_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_sphere_lbfgs_batch_destroy(dzo_sphere_lbfgs_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    qa_free(h);
    return DZO_OK;
}

int32_t dzo_sphere_lbfgs_batch_set_max_halvings(dzo_sphere_lbfgs_batch_t h, int64_t max_halvings) { return cl_set_max_halvings(h, max_halvings); }

// step!(::LBFGSOptimizer), src/DZOptimization.jl:454-509, `steps` times per instance, every trial projected (:133-135)
int32_t dzo_sphere_lbfgs_batch_step(dzo_sphere_lbfgs_batch_t h, int32_t steps, int32_t *all_stuck) {
    return cl_step(h, steps, all_stuck, [&](hipStream_t s) -> int32_t {
        DZO_TIMED("sphere_lbfgs_batch_step", s);
        DZO_DISPATCH(h->core.dtype, (sphere_launch_quench<T>(s, h, steps)));
        DZO_HIP(hipGetLastError());
        return DZO_OK;
    });
}

int32_t dzo_sphere_lbfgs_batch_count_active(dzo_sphere_lbfgs_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_sphere_lbfgs_batch_get_ptr(dzo_sphere_lbfgs_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, qa_array, what, ptr_dev); }

int32_t dzo_sphere_lbfgs_batch_read(dzo_sphere_lbfgs_batch_t h, int32_t what, void *out_host) { return cl_read(h, qa_array, what, out_host); }

}  // extern "C"
