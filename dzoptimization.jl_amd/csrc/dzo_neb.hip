// dzo_neb.hip -- the nudged elastic band with a climbing image (Henkelman & Jonsson 2000; Henkelman, Uberuaga & Jonsson 2000)
// over MANY pairs of Lennard-Jones minima on gfx950: dzo_neb_batch_*.  The double-ended search of the library: where the
// mode-following units start from one point and end where they end, a band of n_images images is strung between two given
// minima and relaxed until its highest image sits on the saddle that joins them.  include/dzo.h, "Batched nudged elastic
// band", states the iteration operation by operation (tests/neb_twin.py replays it on the CPU); the numbers 1 .. 6 below are
// its items.
//
// One 256-thread block per band, `steps` iterations per launch, the phases of an iteration separated by workgroup barriers
// only.  Two launch shapes and ONE body (neb_run):
//
//   * WAVE shape (N <= 64): the interior images are dealt round-robin to the four waves (image m to wave (m - 1) % 4), lane i
//     holds particle i of the wave's image.  The band, its velocities and its forces live in LDS for the whole launch.
//   * BLOCK shape (65 <= N <= 1024): the block takes the images one after another, thread t owns particles t, t + 256, ...;
//     the image under evaluation is staged in LDS for the pair loop of cl_block_eval.  The band's state lives in LDS where
//     dzo_neb_plan.h says it fits, otherwise in device memory (the caller's band, the handle's velocities and forces).
//
// Energies and gradients are cl_wave_eval / cl_block_eval, so they carry the bits of dzo_pairwise_batch_energy_gradient.  Sums
// over the particles are fp64 in the order of the sums of the cluster units: cl_dot3 per particle, the wave tree, then (BLOCK)
// the four wave sums in wave order (cl_block_sum).  Every decision is taken from values every thread reads from LDS behind a
// barrier: the control flow around the barriers is block-uniform.  One writer per element; every loop is bounded by an
// argument.
#include "dzo_cluster.h"
#include "dzo_neb_plan.h"

#include <cmath>
#include <new>

namespace dzo {

static_assert(DZO_NEB_MAX_PARTICLES == kClMaxN, "the argument checks of dzo_cluster.h state the particle bound");
static_assert(kNebLdsLimit == (int64_t)kClLdsMax, "the plan allows what the cluster units allow");
constexpr int kNebArgDoubles = 24;                           // room for the LDS copy of the arguments
static_assert(kNebSmallBytes == 8 * (2 * kWaves + 2 * DZO_NEB_MAX_IMAGES + kNebArgDoubles), "red, F.F, E and the arguments");

extern __shared__ double neb_lds[];

template <typename T> struct NebArgs {
    int N, M, steps, climb, ends, in_lds;
    int64_t climb_after;
    double spring, dt, max_move, force_tol;
    T *band;                   // (3N, M batch) images, the interior ones moved
    T *vel;                    // (3N, M batch) velocities, updated
    T *force;                  // (3N, M batch) record; the working array too when !in_lds (then never null)
    T *tan, *grad, *E;         // records: (3N, M batch), (3N, M batch), (M, batch); tan and grad may be null, E only with `ends`
    double *frms, *res;        // (M, batch), (batch); may be null
    int32_t *climbing, *highest;   // (batch); may be null
    int32_t *status;           // (batch): a band that is not ACTIVE is left alone
    int64_t *iters;            // (batch) moves made so far; null: none
};

template <typename T, typename F, bool BLOCK> __device__ __forceinline__ void neb_run(const NebArgs<T> &a) {
    constexpr int PER = BLOCK ? kClPer : 1;
    const int64_t b = blockIdx.x;
    if (a.status[b] != DZO_NEB_ACTIVE) return;               // frozen: the whole block
    const int tid = threadIdx.x, wv = tid >> 6;
    const int own = BLOCK ? tid : (tid & 63);                // first particle of the thread
    const int N = a.N, n = 3 * N, M = a.M;
    const int64_t base = (int64_t)n * M * b;
    // images of this thread: m0, m0 + dm, ... < M - 1
    const int m0 = BLOCK ? 1 : 1 + wv, dm = BLOCK ? 1 : kWaves;
    int par = 0;

    // the LDS of dzo_neb_plan.h
    double *red = neb_lds, *FF = red + 2 * kWaves;
    T *Es = (T *)(FF + DZO_NEB_MAX_IMAGES);
    // The arguments that are needed after the prologue are read from a copy in LDS, not from the kernel arguments: those
    // are loaded into scalar registers at entry and would stay there to the last use, 13 pointers and 5 fp64 values across a
    // loop whose own uniform state fills the scalar file (17 to 60 scalar registers spilled to vector lanes without the copy, none
    // with it: tests/test_neb_build.py).  Thread 0 writes the copy; the first barrier publishes it.  The construction buys the
    // register budget, not a measured time: whether a launch is faster or slower with it has NOT been measured (spills of this
    // kind are lane moves, no memory traffic, and the LDS reads here are broadcasts).  The alternative, a second argument block
    // of the record pointers read from device memory where it is needed, costs an allocation per handle and per apply call.
    NebArgs<T> *P = (NebArgs<T> *)(FF + 2 * DZO_NEB_MAX_IMAGES);
    static_assert(sizeof(NebArgs<T>) <= 8 * kNebArgDoubles, "the LDS copy of the arguments has its room");
    if (tid == 0) *P = a;
    const NebArgs<T> &p = *P;
    T *stage = (T *)(neb_lds + kNebSmallBytes / 8);
    T *L = stage + (BLOCK ? n : 0);
    const bool in_lds = BLOCK ? (a.in_lds != 0 && a.steps > 0) : true;
    T *Fb = in_lds ? L + 2 * (size_t)n * M : a.force + base;   // ... of the prologue

    bool live[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) live[q] = own + kBlock * q < N;

    // a sum over the particles of one image in every thread that works on it, in the order of the sums
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
    auto load = [&](const T *p, T (&v)[3][PER]) {
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][q] = live[q] ? p[c * N + own + kBlock * q] : T(0);
    };
    auto store = [&](T *p, const T (&v)[3][PER]) {
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (live[q]) p[c * N + own + kBlock * q] = v[c][q];
    };
    // item 1: E and g of image m, read at xm.  BLOCK: every earlier read of the stage lies before a barrier every thread has
    // passed (the sum that ends cl_block_eval, or the barrier before the phase), so the image can be staged at once.
    auto evaluate = [&](int m, const T *xm, T *grad, bool keep_g) {
        T x[3][PER], g[3][PER], E;
        load(xm, x);
        if constexpr (BLOCK) {
            store(stage, x);
            __syncthreads();
            cl_block_eval<T, F>(N, tid, stage, red, par, E, g[0], g[1], g[2]);
        } else {
            cl_wave_eval<T, F>(N, own, x[0][0], x[1][0], x[2][0], E, g[0][0], g[1][0], g[2][0]);
        }
        if (keep_g) store(Fb + (size_t)m * n, g);
        if (grad) store(grad + base + (int64_t)m * n, g);
        if (own == 0) Es[m] = E;
    };

    // the band as it stands: into LDS (the interior images; the ends never move and are read where they are)
    if (in_lds && a.steps > 0) {
        for (int e = n + tid; e < n * (M - 1); e += kBlock) { L[e] = a.band[base + e]; L[(size_t)n * M + e] = a.vel[base + e]; }
        for (int e = tid; e < n; e += kBlock) { L[e] = a.band[base + e]; L[(size_t)n * (M - 1) + e] = a.band[base + (int64_t)n * (M - 1) + e]; }
    }
    if (a.steps > 0)                                         // the ends feel no force
        for (int e = tid; e < n; e += kBlock) {
            Fb[e] = Fb[(size_t)n * (M - 1) + e] = T(0);
            if (a.tan) a.tan[base + e] = a.tan[base + (int64_t)n * (M - 1) + e] = T(0);   // ... and have no tangent
        }
    // the ends' energies: evaluated once (create, apply), then read
    if (a.ends) {
        if (BLOCK || wv == 0) evaluate(0, a.band + base, a.grad, false);
        if (BLOCK || wv == 1) evaluate(M - 1, a.band + base + (int64_t)n * (M - 1), a.grad, false);
    } else if (tid == 0) {
        Es[0] = a.E[(int64_t)M * b];
        Es[M - 1] = a.E[(int64_t)M * b + M - 1];
    }
    __syncthreads();
    if (p.ends && p.E && tid == 0) {
        p.E[(int64_t)M * b] = Es[0];
        p.E[(int64_t)M * b + M - 1] = Es[M - 1];
    }

    // from here on the arguments are p's
    T *X = in_lds ? L : p.band + base;
    T *V = in_lds ? L + (size_t)n * M : p.vel + base;
    Fb = in_lds ? L + 2 * (size_t)n * M : p.force + base;
    const int64_t it0 = p.iters ? p.iters[b] : 0;
    const T dtT = (T)p.dt;
    int moved = 0, status = DZO_NEB_ACTIVE, hi = 1, climbing = -1;
    double resid = 0;
    for (int it = 0; it < a.steps; ++it) {
        // 1. energies and gradients of the interior images, from the band as it stands
        for (int m = m0; m < M - 1; m += dm) evaluate(m, X + (size_t)m * n, p.grad, true);
        __syncthreads();
        // the interior image of highest energy, the first one in index order
        hi = 1;
        {
            T best = Es[1];
            for (int m = 2; m < M - 1; ++m) {
                const T e = Es[m];
                if (e > best) { best = e; hi = m; }
            }
        }
        climbing = (p.climb != 0 && it0 + it >= p.climb_after) ? hi : -1;

        // 2, 3. tangent and force of every interior image; g is replaced by F in place
        for (int m = m0; m < M - 1; m += dm) {
            const T El = Es[m - 1], Em = Es[m], Er = Es[m + 1];
            int branch;                                      // 0: d+, 1: d-, 2: wp d+ + wm d-
            T wp = T(0), wm = T(0);
            if (Er > Em && Em > El) branch = 0;
            else if (Er < Em && Em < El) branch = 1;
            else {
                branch = 2;
                const T ar = cl_abs(Er - Em), al = cl_abs(El - Em);
                const T hiw = ar > al ? ar : al, low = ar > al ? al : ar;
                wp = Er > El ? hiw : low;
                wm = Er > El ? low : hiw;
            }
            T x[3][PER], dp[3][PER], dn[3][PER], t[3][PER], g[3][PER];
            load(X + (size_t)m * n, x);
            load(X + (size_t)(m + 1) * n, dp);
            load(X + (size_t)(m - 1) * n, dn);
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dp[c][q] = dp[c][q] - x[c][q];
                    dn[c][q] = x[c][q] - dn[c][q];
                    t[c][q] = branch == 0 ? dp[c][q] : branch == 1 ? dn[c][q] : dfma<T>(wp, dp[c][q], wm * dn[c][q]);
                }
            const double tn = __builtin_sqrt(dot(t, t)), dpn = __builtin_sqrt(dot(dp, dp)), dnn = __builtin_sqrt(dot(dn, dn));
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[c][q] = (T)((double)t[c][q] / tn);
            load(Fb + (size_t)m * n, g);
            const double cg = dot(g, t);
            if (m == climbing) {
                const double c2 = cg + cg;
#pragma unroll
                for (int q = 0; q < PER; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[c][q] = (T)(-(double)g[c][q] + c2 * (double)t[c][q]);
            } else {
                const double w = p.spring * (dpn - dnn);
#pragma unroll
                for (int q = 0; q < PER; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[c][q] = (T)(-((double)g[c][q] - cg * (double)t[c][q]) + w * (double)t[c][q]);
            }
            const double ff = dot(g, g);
            store(Fb + (size_t)m * n, g);
            if (p.tan) store(p.tan + base + (int64_t)m * n, t);
            if (own == 0) FF[m] = ff;
        }
        __syncthreads();

        // 4. residual and status, the same in every thread
        resid = 0;
        bool bad = !cl_finite(Es[0]) || !cl_finite(Es[M - 1]);
        for (int m = 1; m < M - 1; ++m) {
            const double ff = FF[m], fr = __builtin_sqrt(ff / (double)n);
            bad = bad || !(ff < __builtin_inf()) || !cl_finite(Es[m]);
            resid = fr > resid ? fr : resid;
        }
        status = bad ? DZO_NEB_FAILED : (resid <= p.force_tol ? DZO_NEB_CONVERGED : DZO_NEB_ACTIVE);
        if (status != DZO_NEB_ACTIVE) break;                 // frozen: nothing moves

        // 5. projected velocity Verlet, image by image
        for (int m = m0; m < M - 1; m += dm) {
            T x[3][PER], v[3][PER], f[3][PER], s[3][PER];
            load(V + (size_t)m * n, v);
            load(Fb + (size_t)m * n, f);
            const double vf = dot(v, f), r = vf / FF[m];
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const T vp = vf > 0 ? (T)(r * (double)f[c][q]) : T(0);
                    v[c][q] = dfma<T>(dtT, f[c][q], vp);
                    s[c][q] = dtT * v[c][q];
                }
            const double sn = __builtin_sqrt(dot(s, s));
            load(X + (size_t)m * n, x);
            const double k = p.max_move / sn;
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const T sc = sn > p.max_move ? (T)(k * (double)s[c][q]) : s[c][q];
                    x[c][q] = x[c][q] + sc;
                }
            store(V + (size_t)m * n, v);
            store(X + (size_t)m * n, x);
        }
        moved += 1;
        __syncthreads();                                     // 6: the next iteration reads a complete band
    }

    if (a.steps > 0) {
        // the records of the band before the move of the last iteration made (Es and FF: behind the barrier after item 3)
        if (tid < M) {
            const bool inner = tid > 0 && tid < M - 1;
            if (p.E) p.E[(int64_t)M * b + tid] = Es[tid];
            if (p.frms) p.frms[(int64_t)M * b + tid] = inner ? __builtin_sqrt(FF[tid] / (double)n) : 0.0;
        }
        if (tid == 0) {
            if (p.res) p.res[b] = resid;
            if (p.climbing) p.climbing[b] = climbing;
            if (p.highest) p.highest[b] = hi;
        }
        if (in_lds) {
            for (int e = n + tid; e < n * (M - 1); e += kBlock) {
                p.band[base + e] = L[e];
                p.vel[base + e] = L[(size_t)n * M + e];
            }
            if (p.force)
                for (int e = tid; e < n * M; e += kBlock) p.force[base + e] = L[2 * (size_t)n * M + e];
        }
        if (tid == 0) {
            if (p.iters) p.iters[b] = it0 + moved;
            p.status[b] = status;
        }
    }
}

// ------------------------------------------------------------------------------ the two shapes: grid batch, block 256
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void neb_wave_kernel(NebArgs<T> a) { neb_run<T, F, false>(a); }
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void neb_block_kernel(NebArgs<T> a) { neb_run<T, F, true>(a); }

// x_m = fma(T(m / (M - 1)), b - a, a) for the interior images, copies of a and b at the ends: one thread per element
template <typename T> __global__ __launch_bounds__(kBlock) void neb_interp_kernel(int n, int M, int64_t total, const T *a, const T *b, T *band) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= total) return;
    const int64_t img = idx / n;
    const int e = (int)(idx - img * n), m = (int)(img % M);
    const int64_t src = (img / M) * n + e;
    const T xa = a[src], xb = b[src];
    const T t = (T)((double)m / (double)(M - 1));
    band[idx] = m == 0 ? xa : m == M - 1 ? xb : dfma<T>(t, xb - xa, xa);
}

template <typename T, typename F> static const void *neb_kernel(const NebPlan &plan) {
    return plan.shape == DZO_NEB_SHAPE_WAVE ? (const void *)neb_wave_kernel<T, F> : (const void *)neb_block_kernel<T, F>;
}

// the LDS attribute of the kernel that serves (radial, N, M, dtype), once per call that launches it: it belongs to the kernel and is
// raised to the limit, so that a later, smaller request does not lower it
static int32_t neb_prepare(int32_t radial, int32_t dtype, const NebPlan &plan) {
    if (plan.lds_bytes <= 48 * 1024) return DZO_OK;
    DZO_DISPATCH_RADIAL(radial, dtype, DZO_HIP(hipFuncSetAttribute((neb_kernel<T, F>(plan)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClLdsMax)));
    return DZO_OK;
}

template <typename T, typename F> static void neb_launch(hipStream_t s, int64_t batch, const NebPlan &plan, const NebArgs<T> &a) {
    if (plan.shape == DZO_NEB_SHAPE_WAVE) hipLaunchKernelGGL((neb_wave_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), (size_t)plan.lds_bytes, s, a);
    else hipLaunchKernelGGL((neb_block_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), (size_t)plan.lds_bytes, s, a);
}

// the argument checks of every entry point (the ones without a radial pass Lennard-Jones)
static int32_t neb_check_sizes(int32_t radial, int64_t N, int32_t M, int64_t batch, int32_t dtype) {
    DZO_TRY(cl_check_args(radial, N, batch, dtype));
    DZO_REQUIRE(M >= 3 && M <= DZO_NEB_MAX_IMAGES, DZO_ERR_INVALID, "n_images must be in 3 .. %d (got %d): two fixed ends and at least one image between them",
                DZO_NEB_MAX_IMAGES, M);
    DZO_REQUIRE(batch * M <= (int64_t)1 << 30, DZO_ERR_INVALID, "batch * n_images must not exceed 2^30 (got %lld)", (long long)(batch * M));
    return DZO_OK;
}

// ... and of apply and create
static int32_t neb_check_args(int32_t radial, int64_t N, int32_t M, int64_t batch, int32_t dtype, double spring, double dt, double max_move,
                              double force_tol) {
    DZO_TRY(neb_check_sizes(radial, N, M, batch, dtype));
    DZO_REQUIRE(spring > 0 && dt > 0 && max_move > 0, DZO_ERR_INVALID, "spring, dt and max_move must be positive (got %g, %g, %g)", spring, dt, max_move);
    DZO_REQUIRE(force_tol >= 0, DZO_ERR_INVALID, "force_tol must not be negative (got %g)", force_tol);
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

struct dzo_neb_batch_s {
    ClCore core;                     // x = the band, f = the energies (M per band); stuck = the status (ACTIVE is 0); iters; B = the bands
    void *vel = nullptr, *force = nullptr, *tan = nullptr;
    double *frms = nullptr, *res = nullptr;
    int32_t *climbing = nullptr, *highest = nullptr;
    int32_t M = 0, climb = 0;
    int64_t climb_after = 0;
    double spring = 0, dt = 0, max_move = 0, force_tol = 0;
    NebPlan plan{};
};

namespace dzo {

static void neb_free(dzo_neb_batch_s *h) { cl_free(h, {h->vel, h->force, h->tan, h->frms, h->res, h->climbing, h->highest}); }

template <typename T> static NebArgs<T> neb_args(const dzo_neb_batch_s *h, int steps, int ends) {
    const ClCore &c = h->core;
    NebArgs<T> a{};
    a.N = c.N; a.M = h->M; a.steps = steps; a.climb = h->climb; a.ends = ends; a.in_lds = h->plan.storage == DZO_NEB_STORAGE_LDS;
    a.climb_after = h->climb_after; a.spring = h->spring; a.dt = h->dt; a.max_move = h->max_move; a.force_tol = h->force_tol;
    a.band = (T *)c.x; a.vel = (T *)h->vel; a.force = (T *)h->force; a.tan = (T *)h->tan; a.E = (T *)c.f;
    a.frms = h->frms; a.res = h->res; a.climbing = h->climbing; a.highest = h->highest; a.status = c.stuck; a.iters = c.iters;
    return a;
}

// `what` -> device address, bytes
static int32_t neb_array(dzo_neb_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const ClCore &c = h->core;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, M = (size_t)h->M, n3 = 3 * (size_t)c.N;
    switch (what) {
    case DZO_NEB_BAND: *p = c.x; *bytes = es * n3 * M * B; break;
    case DZO_NEB_VELOCITIES: *p = h->vel; *bytes = es * n3 * M * B; break;
    case DZO_NEB_FORCES: *p = h->force; *bytes = es * n3 * M * B; break;
    case DZO_NEB_TANGENTS: *p = h->tan; *bytes = es * n3 * M * B; break;
    case DZO_NEB_ENERGIES: *p = c.f; *bytes = es * M * B; break;
    case DZO_NEB_FORCE_RMS: *p = h->frms; *bytes = 8 * M * B; break;
    case DZO_NEB_RESIDUALS: *p = h->res; *bytes = 8 * B; break;
    case DZO_NEB_CLIMBING_IMAGES: *p = h->climbing; *bytes = 4 * B; break;
    case DZO_NEB_HIGHEST_IMAGES: *p = h->highest; *bytes = 4 * B; break;
    case DZO_NEB_STATUS: *p = c.stuck; *bytes = 4 * B; break;
    case DZO_NEB_ITERATION_COUNTS: *p = c.iters; *bytes = 8 * B; break;
    default: set_error("unknown elastic-band array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

int32_t dzo_neb_plan(int64_t n_particles, int32_t n_images, int32_t dtype, int32_t *shape, int32_t *storage, int64_t *lds_bytes) {
    DZO_TRY(neb_check_sizes(DZO_RADIAL_LENNARD_JONES, n_particles, n_images, 1, dtype));
    const NebPlan plan = neb_plan(n_particles, n_images, dtype);
    if (shape) *shape = plan.shape;
    if (storage) *storage = plan.storage;
    if (lds_bytes) *lds_bytes = plan.lds_bytes;
    return DZO_OK;
}

int32_t dzo_neb_batch_interpolate(int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, const void *a_dev, const void *b_dev,
                                  void *band_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(a_dev && b_dev && band_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(neb_check_sizes(DZO_RADIAL_LENNARD_JONES, n_particles, n_images, batch, dtype));
    const char *where = "dzo_neb_batch_interpolate", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, a_dev, "a", b_dev, "b"));
    DZO_TRY(require_same_backend(where, cite, band_dev, "band", nullptr, ""));
    Context &c = ctx();
    const int n = 3 * (int)n_particles;
    const int64_t total = (int64_t)n * n_images * batch;
    {
        DZO_TIMED("neb_interpolate", c.stream);
        DZO_DISPATCH(dtype, hipLaunchKernelGGL((neb_interp_kernel<T>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, c.stream, n,
                                               (int)n_images, total, (const T *)a_dev, (const T *)b_dev, (T *)band_dev));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// the iteration of include/dzo.h, once, from the caller's band and velocities
int32_t dzo_neb_batch_apply(int32_t radial, int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, void *band_dev, void *velocities_dev,
                            double spring, double dt, double max_move, double force_tol, int32_t climb, void *energies_dev, void *gradients_dev,
                            void *forces_dev, void *tangents_dev, double *force_rms_dev, double *residuals_dev, int32_t *climbing_dev,
                            int32_t *highest_dev, int32_t *status_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(band_dev && velocities_dev && status_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(neb_check_args(radial, n_particles, n_images, batch, dtype, spring, dt, max_move, force_tol));
    const char *where = "dzo_neb_batch_apply", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, band_dev, "band", velocities_dev, "velocities"));
    DZO_TRY(require_same_backend(where, cite, status_dev, "status", energies_dev, "energies"));
    DZO_TRY(require_same_backend(where, cite, gradients_dev, "gradients", forces_dev, "forces"));
    DZO_TRY(require_same_backend(where, cite, tangents_dev, "tangents", force_rms_dev, "force_rms"));
    DZO_TRY(require_same_backend(where, cite, residuals_dev, "residuals", climbing_dev, "climbing"));
    DZO_TRY(require_same_backend(where, cite, highest_dev, "highest", nullptr, ""));
    Context &c = ctx();
    const NebPlan plan = neb_plan(n_particles, n_images, dtype);
    DZO_TRY(neb_prepare(radial, dtype, plan));
    void *work = nullptr;                                    // MEMORY storage iterates on the forces: they need a home
    if (plan.storage == DZO_NEB_STORAGE_MEMORY && !forces_dev)
        DZO_TRY(device_alloc(&work, dtype_size(dtype) * 3 * (size_t)n_particles * (size_t)n_images * (size_t)batch, "the elastic band's forces", false));
    int32_t rc = [&]() -> int32_t {
        {
            DZO_TIMED("neb_step", c.stream);
            DZO_HIP(hipMemsetAsync(status_dev, 0, 4 * (size_t)batch, c.stream));   // every band ACTIVE
            DZO_DISPATCH_RADIAL(radial, dtype, NebArgs<T> a{};
                         a.N = (int)n_particles; a.M = n_images; a.steps = 1; a.climb = climb; a.ends = 1; a.in_lds = plan.storage == DZO_NEB_STORAGE_LDS;
                         a.climb_after = 0; a.spring = spring; a.dt = dt; a.max_move = max_move; a.force_tol = force_tol;
                         a.band = (T *)band_dev; a.vel = (T *)velocities_dev; a.force = (T *)(forces_dev ? forces_dev : work);
                         a.tan = (T *)tangents_dev; a.grad = (T *)gradients_dev; a.E = (T *)energies_dev; a.frms = force_rms_dev; a.res = residuals_dev;
                         a.climbing = climbing_dev; a.highest = highest_dev; a.status = status_dev; a.iters = nullptr;
                         (neb_launch<T, F>(c.stream, batch, plan, a)));
            DZO_HIP(hipGetLastError());
        }
        DZO_HIP(hipStreamSynchronize(c.stream));
        return DZO_OK;
    }();
    if (work) (void)hipFree(work);
    return rc;
}

int32_t dzo_neb_batch_create(int32_t radial, int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, void *band_dev, double spring,
                             double dt, double max_move, double force_tol, int32_t climb, int64_t climb_after, dzo_neb_batch_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(band_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(neb_check_args(radial, n_particles, n_images, batch, dtype, spring, dt, max_move, force_tol));
    DZO_REQUIRE(climb_after >= 0, DZO_ERR_INVALID, "climb_after must not be negative (got %lld)", (long long)climb_after);
    DZO_TRY(require_same_backend("dzo_neb_batch_create", "every array of a handle lives on one device", band_dev, "band", nullptr, ""));
    dzo_neb_batch_s *h = new (std::nothrow) dzo_neb_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    ClCore &c = h->core;
    c.device = ctx().device; c.dtype = dtype; c.radial = radial; c.N = (int)n_particles; c.B = batch; c.x = band_dev;
    h->M = n_images; h->climb = climb != 0; h->climb_after = climb_after; h->spring = spring; h->dt = dt; h->max_move = max_move; h->force_tol = force_tol;
    h->plan = neb_plan(n_particles, n_images, dtype);
    const size_t es = dtype_size(dtype), B = (size_t)batch, M = (size_t)n_images, n3 = 3 * (size_t)n_particles;
    int32_t rc = cl_alloc({{&c.f, es * M * B}, {(void **)&c.stuck, 4 * B}, {(void **)&c.iters, 8 * B}, {(void **)&c.active_dev, 8},
                           {&h->vel, es * n3 * M * B}, {&h->force, es * n3 * M * B}, {&h->tan, es * n3 * M * B}, {(void **)&h->frms, 8 * M * B},
                           {(void **)&h->res, 8 * B}, {(void **)&h->climbing, 4 * B}, {(void **)&h->highest, 4 * B}},
                          "the elastic-band state");
    if (rc == DZO_OK) rc = neb_prepare(radial, dtype, h->plan);
    if (rc == DZO_OK)
        rc = cl_finish_create(&c, nullptr, "elastic-band state", "elastic-band constructor", [&](hipStream_t s) -> int32_t {
            DZO_TIMED("neb_init", s);
            DZO_HIP(hipMemsetAsync(h->climbing, 0xff, 4 * B, s));   // -1: no image climbs yet
            // the energies of the fixed ends; every other record is zero until the first iteration
            DZO_DISPATCH_RADIAL(radial, dtype, (neb_launch<T, F>(s, batch, h->plan, neb_args<T>(h, 0, 1))));
            return DZO_OK;
        });
    if (rc != DZO_OK) { neb_free(h); return rc; }
    *out = h;
    return DZO_OK;
}

int32_t dzo_neb_batch_destroy(dzo_neb_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->core.device);
    (void)hipStreamSynchronize(ctx().stream);
    neb_free(h);
    return DZO_OK;
}

// `steps` iterations of every ACTIVE band in ONE launch; nothing waits inside it or after it
int32_t dzo_neb_batch_step(dzo_neb_batch_t h, int32_t steps, int32_t *all_done) {
    return cl_step(h, steps, all_done, [&](hipStream_t s) -> int32_t {
        const ClCore &c = h->core;
        DZO_TIMED("neb_step", s);
        DZO_DISPATCH_RADIAL(c.radial, c.dtype, (neb_launch<T, F>(s, c.B, h->plan, neb_args<T>(h, steps, 0))));
        DZO_HIP(hipGetLastError());
        return DZO_OK;
    });
}

int32_t dzo_neb_batch_count_active(dzo_neb_batch_t h, int64_t *active) { return cl_count(h, active); }

int32_t dzo_neb_batch_get_ptr(dzo_neb_batch_t h, int32_t what, void **ptr_dev) { return cl_get_ptr(h, neb_array, what, ptr_dev); }

int32_t dzo_neb_batch_read(dzo_neb_batch_t h, int32_t what, void *out_host) { return cl_read(h, neb_array, what, out_host); }

}  // extern "C"
