// dzo_modefollow.hip -- eigenvector following (Cerjan-Miller / Wales) over MANY small Lennard-Jones clusters on gfx950:
// dzo_modefollow_batch_*.  Target index 0 polishes the minima a quench leaves at is_stuck down to a rounding-level gradient;
// target index 1 walks uphill along one followed mode to a transition state.  include/dzo.h states the step operation by
// operation (tests/modefollow_twin.py replays it on the CPU).
//
// A step of the handle is three launches on the library's stream with no host wait between them: the dense Hessians
// (dzo_hessian_batch.hip), their eigenvalues and eigenvectors (dzo_symeig.hip) -- both through dzo_chain.h -- and the step
// kernel of this file, the first consumer of the eigensolver's vectors.
//
// The step kernel: one 256-thread block per instance, n = 3N <= DZO_SYMEIG_MAX_N.
//
//   * Point, gradient, eigenvalues, projections F, mode steps h and the followed vector live in static LDS (six arrays of n
//     elements and n fp64 overlaps: 21 KiB in fp64 at n = 384).  Energy and gradient are dzo_cluster.h's routines with the
//     shapes of dzo_pairwise_batch_energy_gradient: N <= 64 the first wave alone (cl_wave_eval), above the block
//     (cl_block_eval): the same bits.
//   * F = V^T g: a wave per column, four columns of a wave in flight (c = wv + 4 k), the lanes stride the rows -- consecutive
//     addresses in the column-major V --, an fp64 fused multiply-add per element, then the wave tree.  With a followed vector
//     the overlap V[:,c].w comes from the same loads.
//   * x += V h: a thread per row, columns ascending; for a fixed column the threads' addresses are consecutive.
//   * V is read twice from L2 (114 x 114 fp64 is 104 KB per instance).  Counts of modes are block sums of small integers held
//     in fp64 (exact).  One writer per element, no atomics.
#include "dzo_chain.h"
#include "dzo_cluster.h"
#include "dzo_symeig_plan.h"

#include <new>

namespace dzo {

constexpr int kMfMaxDim = DZO_SYMEIG_MAX_N;                  // n = 3N
constexpr int kMfMaxN = DZO_MODEFOLLOW_MAX_PARTICLES;
static_assert(3 * kMfMaxN == kMfMaxDim, "one block of the eigensolver iterates on an instance's Hessian");
constexpr int kMfCols = 4;                                   // columns a wave keeps in flight in the projection

template <typename T> struct ModefollowArgs {
    int N, target_index, start_mode;
    T zero_tol;
    double max_step, grad_tol;
    T *x;                      // (3N, batch) points, moved
    const T *lam;              // (3N, batch) eigenvalues, ascending
    const T *V;                // (3N, 3N, batch) eigenvectors, column-major
    T *w;                      // (3N, batch) followed vectors, or null (target index 0)
    int32_t *w_set;            // (batch), or null
    const int32_t *sweeps;     // (batch) the eigensolver's verdicts, or null
    T *E, *g, *F;              // records: (batch), (3N, batch), (3N, batch); each may be null
    double *grms, *steplen;    // (batch); may be null
    int32_t *status;           // (batch): an instance that is not ACTIVE is left alone
    int32_t *index, *zeros, *followed;   // (batch); may be null
    int64_t *iters;            // (batch); may be null
};

template <typename T> struct ModefollowRecord {
    T E;
    double grms, steplen;
    int status, index, zeros, followed;
};

// thread 0 of the block: what the step leaves behind for instance b
template <typename T> __device__ __forceinline__ void mf_record(const ModefollowArgs<T> &a, int64_t b, const ModefollowRecord<T> &r) {
    if (a.E) a.E[b] = r.E;
    if (a.grms) a.grms[b] = r.grms;
    if (a.steplen) a.steplen[b] = r.steplen;
    if (a.index) a.index[b] = r.index;
    if (a.zeros) a.zeros[b] = r.zeros;
    if (a.followed) a.followed[b] = r.followed;
    if (a.iters && r.status == DZO_MODEFOLLOW_ACTIVE) a.iters[b] += 1;
    a.status[b] = r.status;
}

// grid batch, block 256; RF is the radial functor (F is the projections' name here).  The body is a __device__ function and the
// kernel the entry point that calls it: written into the __global__ function itself, the same statements compile to other code
// ("One table, one entry point per kernel").
template <typename T, typename RF> __device__ __forceinline__ void modefollow_step_body(ModefollowArgs<T> a) {
    __shared__ T S[6 * kMfMaxDim];                           // X | G | L | F | H | W, n elements each
    __shared__ double ov[kMfMaxDim];                         // |V[:,c].w|
    __shared__ double red[2 * kWaves];
    __shared__ T Es;
    __shared__ int chosen;
    const int64_t b = blockIdx.x;
    if (a.status[b] != DZO_MODEFOLLOW_ACTIVE) return;        // frozen: the whole block
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = a.N, n = 3 * N;
    const int64_t base = (int64_t)n * b;
    T *X = S, *G = X + n, *L = G + n, *F = L + n, *H = F + n, *W = H + n;
    const T *V = a.V + (int64_t)n * n * b;
    const bool follow = a.target_index == 1;
    const bool wset = follow && a.w_set[b] != 0;             // the same in every thread
    for (int e = tid; e < n; e += kBlock) {
        X[e] = a.x[base + e];
        L[e] = a.lam[base + e];
        W[e] = wset ? a.w[base + e] : T(0);
    }
    if (tid == 0) chosen = -1;
    __syncthreads();

    // 1. energy and gradient, the shapes of dzo_pairwise_batch_energy_gradient
    T E;
    int par = 0;
    if (N <= 64) {
        if (wv == 0) {
            const bool live = lane < N;
            const T x = live ? X[lane] : T(0), y = live ? X[N + lane] : T(0), z = live ? X[2 * N + lane] : T(0);
            T e0, gx, gy, gz;
            cl_wave_eval<T, RF>(N, lane, x, y, z, e0, gx, gy, gz);
            if (live) { G[lane] = gx; G[N + lane] = gy; G[2 * N + lane] = gz; }
            if (lane == 0) Es = e0;
        }
        __syncthreads();
        E = Es;
    } else {
        T gx[kClPer], gy[kClPer], gz[kClPer];
        cl_block_eval<T, RF>(N, tid, X, red, par, E, gx, gy, gz);
        CL_FOR_OWN(i, G[i] = gx[q]; G[N + i] = gy[q]; G[2 * N + i] = gz[q];)
        __syncthreads();
    }

    // 2. - 4. gradient norm, the classes of the modes, the freeze check
    const T zt = a.zero_tol;
    double gpart = 0, negs = 0, zers = 0;
    bool bad = !cl_finite(E);
    for (int e = tid; e < n; e += kBlock) {
        const T gv = G[e], lv = L[e];
        gpart = __builtin_fma((double)gv, (double)gv, gpart);
        bad = bad || !cl_finite(gv) || !cl_finite(lv);
        negs += lv < -zt ? 1.0 : 0.0;
        zers += cl_abs(lv) <= zt ? 1.0 : 0.0;
        if (a.g) a.g[base + e] = gv;
    }
    if (a.sweeps && a.sweeps[b] < 0) bad = true;
    const double gg = cl_block_sum(gpart, red, par);
    ModefollowRecord<T> rec;
    rec.E = E;
    rec.grms = __builtin_sqrt(gg / (double)n);
    rec.index = (int)cl_block_sum(negs, red, par);
    rec.zeros = (int)cl_block_sum(zers, red, par);
    rec.followed = -1;
    rec.steplen = 0;
    bad = __syncthreads_or(bad ? 1 : 0) != 0;
    rec.status = bad ? DZO_MODEFOLLOW_FAILED : (rec.grms <= a.grad_tol ? DZO_MODEFOLLOW_CONVERGED : DZO_MODEFOLLOW_ACTIVE);
    if (rec.status != DZO_MODEFOLLOW_ACTIVE) {               // the same in every thread: the point is not moved
        if (tid == 0) mf_record(a, b, rec);
        return;
    }

    // 5. F = V^T g and, with a followed vector, the overlaps with it
    for (int c0 = wv; c0 < n; c0 += kWaves * kMfCols) {
        double acc[kMfCols], aw[kMfCols];
#pragma unroll
        for (int j = 0; j < kMfCols; ++j) acc[j] = aw[j] = 0;
        for (int r = lane; r < n; r += 64) {
            const double gr = (double)G[r], wr = (double)W[r];
            T v[kMfCols];
#pragma unroll
            for (int j = 0; j < kMfCols; ++j) {
                const int c = c0 + kWaves * j, cc = c < n ? c : c0;   // (a column that exists; the value is dropped)
                v[j] = V[r + (int64_t)n * cc];
            }
#pragma unroll
            for (int j = 0; j < kMfCols; ++j) {
                acc[j] = __builtin_fma((double)v[j], gr, acc[j]);
                aw[j] = __builtin_fma((double)v[j], wr, aw[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kMfCols; ++j) {
            const int c = c0 + kWaves * j;
            const double f = wave_sum_all(acc[j]), o = wave_sum_all(aw[j]);
            if (lane == 0 && c < n) { F[c] = (T)f; ov[c] = __builtin_fabs(o); }
        }
    }
    __syncthreads();

    // 6. the followed mode
    int istar = -1;
    if (follow) {
        for (int i = tid; i < n; i += kBlock) {
            if (cl_abs(L[i]) <= zt) continue;
            bool win;
            if (!wset) {
                int rank = 0;
                for (int j = 0; j < i; ++j) rank += cl_abs(L[j]) <= zt ? 0 : 1;
                win = rank == a.start_mode;
            } else {
                const double oi = ov[i];
                win = oi == oi;
                for (int j = 0; j < n; ++j) {
                    const double oj = ov[j];
                    const bool nz = !(cl_abs(L[j]) <= zt);
                    win = win && !(nz && (oj > oi || (oj == oi && j < i)));
                }
            }
            if (win) chosen = i;                             // one winner at most
        }
        __syncthreads();
        istar = chosen;
        if (istar < 0) {                                     // fewer non-zero modes than start_mode, or non-finite overlaps
            rec.status = DZO_MODEFOLLOW_FAILED;
            if (tid == 0) mf_record(a, b, rec);
            return;
        }
        for (int r = tid; r < n; r += kBlock) a.w[base + r] = V[r + (int64_t)n * istar];
        if (tid == 0) a.w_set[b] = 1;
    }

    // 7. the mode steps
    double hpart = 0;
    for (int i = tid; i < n; i += kBlock) {
        const T al = cl_abs(L[i]), f = F[i];
        const T q = (f + f) / al;
        const T hq = q / (T(1) + cl_sqrt(T(1) + q * q));
        const T hs = i == istar ? hq : -hq;
        const T h = al <= zt ? T(0) : hs;
        H[i] = h;
        hpart = __builtin_fma((double)h, (double)h, hpart);
        if (a.F) a.F[base + i] = f;
    }
    // 8. the cap (the sum's barrier publishes H)
    const double hn = __builtin_sqrt(cl_block_sum(hpart, red, par));
    const bool capped = hn > a.max_step;
    if (capped) {
        const T scale = (T)(a.max_step / hn);
        for (int i = tid; i < n; i += kBlock) H[i] *= scale;
    }
    __syncthreads();

    // 9. the move
    for (int r = tid; r < n; r += kBlock) {
        const T *row = V + r;
        T acc = T(0);
#pragma unroll 8
        for (int i = 0; i < n; ++i) acc = dfma<T>(row[(int64_t)n * i], H[i], acc);
        a.x[base + r] = X[r] + acc;
    }

    // 10.
    rec.followed = istar;
    rec.steplen = capped ? a.max_step : hn;
    if (tid == 0) mf_record(a, b, rec);
}
template <typename T, typename RF> __global__ __launch_bounds__(kBlock) void modefollow_step_kernel(ModefollowArgs<T> a) { modefollow_step_body<T, RF>(a); }

template <typename T, typename RF> static void mf_launch(hipStream_t s, int64_t batch, const ModefollowArgs<T> &a) {
    hipLaunchKernelGGL((modefollow_step_kernel<T, RF>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

// the argument checks of apply and create
static int32_t mf_check_args(int32_t radial, int64_t N, int64_t batch, int32_t dtype, int32_t target_index, int32_t start_mode, double max_step,
                             double zero_tol, double grad_tol) {
    DZO_TRY(pw_check_args(radial, dtype, N, batch, "batch", kMfMaxN, DZO_ERR_UNSUPPORTED,
                          "one block of the eigensolver iterates on an instance's 3N x 3N Hessian"));
    DZO_REQUIRE(target_index == 0 || target_index == 1, DZO_ERR_INVALID, "target_index must be 0 (a minimum) or 1 (a transition state), got %d",
                target_index);
    DZO_REQUIRE(start_mode >= 0, DZO_ERR_INVALID, "start_mode must not be negative (got %d)", start_mode);
    DZO_REQUIRE(max_step > 0, DZO_ERR_INVALID, "max_step must be positive (got %g)", max_step);
    DZO_REQUIRE(zero_tol >= 0 && grad_tol >= 0, DZO_ERR_INVALID, "zero_tol and grad_tol must not be negative (got %g, %g)", zero_tol, grad_tol);
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

struct dzo_modefollow_batch_s {
    ClCore core;                     // x, g, f; stuck = the status (ACTIVE is 0); iters
    void *hess = nullptr, *lam = nullptr, *V = nullptr, *work = nullptr, *w = nullptr;
    int32_t *sweeps = nullptr, *w_set = nullptr, *index = nullptr, *zeros = nullptr, *followed = nullptr;
    double *grms = nullptr, *steplen = nullptr;
    int32_t target_index = 0, start_mode = 0;
    double max_step = 0, zero_tol = 0, grad_tol = 0;
};

namespace dzo {

static void mf_free(dzo_modefollow_batch_s *h) {
    cl_free(h, {h->hess, h->lam, h->V, h->work, h->w, h->sweeps, h->w_set, h->index, h->zeros, h->followed, h->grms, h->steplen});
}

template <typename T> static ModefollowArgs<T> mf_args(const dzo_modefollow_batch_s *h) {
    const ClCore &c = h->core;
    ModefollowArgs<T> a;
    a.N = c.N; a.target_index = h->target_index; a.start_mode = h->start_mode;
    a.zero_tol = (T)h->zero_tol; a.max_step = h->max_step; a.grad_tol = h->grad_tol;
    a.x = (T *)c.x; a.lam = (const T *)h->lam; a.V = (const T *)h->V; a.w = (T *)h->w; a.w_set = h->w_set; a.sweeps = h->sweeps;
    a.E = (T *)c.f; a.g = (T *)c.g; a.F = nullptr;
    a.grms = h->grms; a.steplen = h->steplen;
    a.status = c.stuck; a.index = h->index; a.zeros = h->zeros; a.followed = h->followed; a.iters = c.iters;
    return a;
}

// `what` -> device address, bytes
static int32_t mf_array(dzo_modefollow_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const ClCore &c = h->core;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, n3 = 3 * (size_t)c.N;
    switch (what) {
    case DZO_MODEFOLLOW_POINTS: *p = c.x; *bytes = es * n3 * B; break;
    case DZO_MODEFOLLOW_GRADIENTS: *p = c.g; *bytes = es * n3 * B; break;
    case DZO_MODEFOLLOW_ENERGIES: *p = c.f; *bytes = es * B; break;
    case DZO_MODEFOLLOW_GRMS: *p = h->grms; *bytes = 8 * B; break;
    case DZO_MODEFOLLOW_STATUS: *p = c.stuck; *bytes = 4 * B; break;
    case DZO_MODEFOLLOW_INDEX: *p = h->index; *bytes = 4 * B; break;
    case DZO_MODEFOLLOW_ZEROS: *p = h->zeros; *bytes = 4 * B; break;
    case DZO_MODEFOLLOW_FOLLOWED_MODE: *p = h->followed; *bytes = 4 * B; break;
    case DZO_MODEFOLLOW_STEP_LENGTHS: *p = h->steplen; *bytes = 8 * B; break;
    case DZO_MODEFOLLOW_ITERATION_COUNTS: *p = c.iters; *bytes = 8 * B; break;
    case DZO_MODEFOLLOW_EIGENVALUES: *p = h->lam; *bytes = es * n3 * B; break;
    case DZO_MODEFOLLOW_EIGENVECTORS: *p = h->V; *bytes = es * n3 * n3 * B; break;
    case DZO_MODEFOLLOW_SWEEPS: *p = h->sweeps; *bytes = 4 * B; break;
    case DZO_MODEFOLLOW_FOLLOW: *p = h->w; *bytes = es * n3 * B; break;
    default: set_error("unknown mode-following array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

// the step of include/dzo.h, once, from the caller's modes
int32_t dzo_modefollow_batch_apply(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, const void *eigenvalues_dev,
                                   const void *eigenvectors_dev, void *follow_dev, int32_t *follow_set_dev, int32_t target_index, int32_t start_mode,
                                   double max_step, double zero_tol, double grad_tol, void *energies_dev, void *gradients_dev, void *projections_dev,
                                   double *grms_dev, int32_t *status_dev, int32_t *index_dev, int32_t *zeros_dev, int32_t *followed_dev,
                                   double *step_lengths_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && eigenvalues_dev && eigenvectors_dev && status_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(mf_check_args(radial, n_particles, batch, dtype, target_index, start_mode, max_step, zero_tol, grad_tol));
    DZO_REQUIRE(target_index == 0 || (follow_dev && follow_set_dev), DZO_ERR_INVALID, "target_index 1 needs follow_dev and follow_set_dev");
    const char *where = "dzo_modefollow_batch_apply", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", eigenvalues_dev, "eigenvalues"));
    DZO_TRY(require_same_backend(where, cite, eigenvectors_dev, "eigenvectors", status_dev, "status"));
    DZO_TRY(require_same_backend(where, cite, follow_dev, "follow", follow_set_dev, "follow_set"));
    DZO_TRY(require_same_backend(where, cite, energies_dev, "energies", gradients_dev, "gradients"));
    DZO_TRY(require_same_backend(where, cite, projections_dev, "projections", grms_dev, "grms"));
    DZO_TRY(require_same_backend(where, cite, index_dev, "index", zeros_dev, "zeros"));
    DZO_TRY(require_same_backend(where, cite, followed_dev, "followed", step_lengths_dev, "step_lengths"));
    Context &c = ctx();
    {
        DZO_TIMED("modefollow_step", c.stream);
        DZO_HIP(hipMemsetAsync(status_dev, 0, 4 * (size_t)batch, c.stream));   // every instance ACTIVE
        DZO_DISPATCH_RADIAL(radial, dtype, ModefollowArgs<T> a;
                     a.N = (int)n_particles; a.target_index = target_index; a.start_mode = start_mode;
                     a.zero_tol = (T)zero_tol; a.max_step = max_step; a.grad_tol = grad_tol;
                     a.x = (T *)points_dev; a.lam = (const T *)eigenvalues_dev; a.V = (const T *)eigenvectors_dev;
                     a.w = (T *)follow_dev; a.w_set = follow_set_dev; a.sweeps = nullptr;
                     a.E = (T *)energies_dev; a.g = (T *)gradients_dev; a.F = (T *)projections_dev;
                     a.grms = grms_dev; a.steplen = step_lengths_dev;
                     a.status = status_dev; a.index = index_dev; a.zeros = zeros_dev; a.followed = followed_dev; a.iters = nullptr;
                     (mf_launch<T, F>(c.stream, batch, a)));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

int32_t dzo_modefollow_batch_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev, int32_t target_index,
                                    double max_step, double zero_tol, double grad_tol, dzo_modefollow_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(mf_check_args(radial, n_particles, batch, dtype, target_index, 0, max_step, zero_tol, grad_tol));
    DZO_TRY(require_same_backend("dzo_modefollow_batch_create", "every array of a handle lives on one device", points_dev, "points", nullptr, ""));
    dzo_modefollow_batch_s *h = new (std::nothrow) dzo_modefollow_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.radial = radial; c.N = (int)n_particles; c.B = batch; c.x = points_dev;
    h->target_index = target_index; h->max_step = max_step; h->zero_tol = zero_tol; h->grad_tol = grad_tol;
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles;
    const bool in_memory = symeig_plan((int64_t)n3, dtype).storage == DZO_SYMEIG_STORAGE_MEMORY;
    int32_t rc = cl_alloc({{&c.g, es * n3 * B}, {&c.f, es * B}, {(void **)&c.stuck, 4 * B}, {(void **)&c.iters, 8 * B}, {(void **)&c.active_dev, 8},
                           {&h->hess, es * n3 * n3 * B}, {&h->lam, es * n3 * B}, {&h->V, es * n3 * n3 * B},
                           {in_memory ? &h->work : nullptr, es * n3 * n3 * B}, {&h->w, es * n3 * B}, {(void **)&h->sweeps, 4 * B},
                           {(void **)&h->w_set, 4 * B}, {(void **)&h->index, 4 * B}, {(void **)&h->zeros, 4 * B}, {(void **)&h->followed, 4 * B},
                           {(void **)&h->grms, 8 * B}, {(void **)&h->steplen, 8 * B}},
                          "the mode-following state");
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, nullptr, "mode-following state", "mode-following constructor", [&](hipStream_t s) -> int32_t {
            DZO_TRY(se_prepare((int64_t)n3, dtype));
            DZO_TIMED("modefollow_init", s);
            // the energies and gradients of the points as given; every other record is zero until the first step
            DZO_DISPATCH(dtype, DZO_TRY(cl_launch_eval<T>(s, radial, c.N, batch, (const T *)c.x, (T *)c.f, (T *)c.g)));
            return DZO_OK;
        });
    if (rc != DZO_OK) { mf_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_modefollow_batch_destroy(dzo_modefollow_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    mf_free(h);
    return DZO_OK;
}

int32_t dzo_modefollow_batch_set_start_mode(dzo_modefollow_batch_t h, int32_t mode) {
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(mode >= 0, DZO_ERR_INVALID, "start_mode must not be negative (got %d)", mode);
    h->start_mode = mode;
    return DZO_OK;
}

int32_t dzo_modefollow_batch_set_directions(dzo_modefollow_batch_t h, const void *dirs_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && dirs_dev, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->core.device);
    DZO_TRY(require_same_backend("dzo_modefollow_batch_set_directions", "every array of a handle lives on one device", dirs_dev, "directions", nullptr, ""));
    const ClCore &c = h->core;
    hipStream_t s = ctx().stream;
    DZO_HIP(hipMemcpyAsync(h->w, dirs_dev, dtype_size(c.dtype) * 3 * (size_t)c.N * (size_t)c.B, hipMemcpyDeviceToDevice, s));
    DZO_HIP(hipMemsetD32Async((hipDeviceptr_t)h->w_set, 1, (size_t)c.B, s));
    return DZO_OK;
}

// per step: Hessian, eigensolver with vectors, the step kernel; nothing waits in between
int32_t dzo_modefollow_batch_step(dzo_modefollow_batch_t h, int32_t steps, int32_t *all_done) {
    return cl_step(h, steps, all_done, [&](hipStream_t s) -> int32_t {
        const ClCore &c = h->core;
        for (int32_t k = 0; k < steps; ++k) {
            {
                DZO_TIMED("modefollow_hessian", s);
                DZO_TRY(hb_enqueue_hessian(s, c.radial, c.dtype, c.N, c.B, c.x, h->hess));
            }
            {
                DZO_TIMED("modefollow_eigen", s);
                DZO_TRY(se_enqueue(s, 3 * (int64_t)c.N, c.B, c.dtype, h->hess, h->work, h->lam, h->V, h->sweeps, 0));
            }
            DZO_TIMED("modefollow_step", s);
            DZO_DISPATCH_RADIAL(c.radial, c.dtype, (mf_launch<T, F>(s, c.B, mf_args<T>(h))));
            DZO_HIP(hipGetLastError());
        }
        return DZO_OK;
    });
}

int32_t dzo_modefollow_batch_count_active(dzo_modefollow_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_modefollow_batch_get_ptr(dzo_modefollow_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, mf_array, what, ptr_dev); }

int32_t dzo_modefollow_batch_read(dzo_modefollow_batch_t h, int32_t what, void *out_host) { return cl_read(h, mf_array, what, out_host); }

}  // extern "C"
