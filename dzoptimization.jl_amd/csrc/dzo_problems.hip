// dzo_problems.hip -- device-side synthetic objectives (K12).
//
// These are the *user's* callbacks in the reference (objective_function / gradient_function!,
// src/DZOptimization.jl:324-325); the reference ships only the 2-D Rosenbrock pair
// (legacy/ExampleFunctions.jl:10-24, README.md:25-31).  Elementwise expressions are the same
// explicit-fma expressions as oracle/dzo_oracle_impl.h so values agree bit-for-bit per term;
// only the (deterministic, two-stage) reduction order differs.
#include <limits>

#include "dzo_problems.h"
#include "dzo_pairwise.h"
#include "dzo_rosen.h"

namespace dzo {

// ------------------------------------------------------------------ 2-D Rosenbrock (config 1)
template <typename T>
__global__ void rosen2d_eval_kernel(const T *__restrict__ x, double *__restrict__ result) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        T t1 = (T)1 - x[0];
        T t2 = x[1] - x[0] * x[0];
        result[0] = (double)(t1 * t1 + (T)100 * (t2 * t2));
    }
}
template <typename T>
__global__ void rosen2d_grad_kernel(T *__restrict__ g, const T *__restrict__ x) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        T t1 = (T)1 - x[0];
        T t2 = x[1] - x[0] * x[0];
        g[0] = (T)-2 * t1 - (T)400 * x[0] * t2;
        g[1] = (T)200 * t2;
    }
}

// ------------------------------------------------------------------ chained Rosenbrock (config 3)
template <typename T>
__global__ __launch_bounds__(kBlock) void rosen_chain_eval_kernel(int64_t n, const T *__restrict__ x,
                                                                  double *__restrict__ partials) {
    constexpr int N = Vec16<T>::N;
    __shared__ double lds[kWaves];
    double acc = 0;
    const int64_t nvec = n / N;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += nthreads) {
        const int64_t i = v * N;
        T xv[N];
        load16(x + i, xv);
        const T xnext = (i + N < n) ? x[i + N] : (T)0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const T xn = (j + 1 < N) ? xv[(j + 1) % N] : xnext;
            if (i + j + 1 < n) acc += rosen_term<T>(xv[j], xn);
        }
    }
    const int64_t t = nvec * N + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t + 1 < n) acc += rosen_term<T>(x[t], x[t + 1]);
    double r = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rosen_chain_grad_kernel(int64_t n, T *__restrict__ g,
                                                                  const T *__restrict__ x) {
    constexpr int N = Vec16<T>::N;
    const int64_t nvec = n / N;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += nthreads) {
        const int64_t i = v * N;
        T xv[N], gv[N];
        load16(x + i, xv);
        const T xprev = (i > 0) ? x[i - 1] : (T)0;
        const T xnext = (i + N < n) ? x[i + N] : (T)0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const T xp = (j > 0) ? xv[(j + N - 1) % N] : xprev;
            const T xn = (j + 1 < N) ? xv[(j + 1) % N] : xnext;
            gv[j] = rosen_grad_elem<T>(i + j, n, xp, xv[j], xn);
        }
        store16(g + i, gv);
    }
    const int64_t t = nvec * N + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) g[t] = rosen_grad_elem<T>(t, n, t > 0 ? x[t - 1] : (T)0, x[t], t + 1 < n ? x[t + 1] : (T)0);
}

// ------------------------------------------------------------------ chained quadratic (dzo_rosen.h)
// (plain elementwise kernels: this objective's fast path is the L-BFGS point pass, which recomputes these in registers)
template <typename T>
__global__ __launch_bounds__(kBlock) void qchain_eval_kernel(int64_t n, const T *__restrict__ x, T lambda, double *__restrict__ partials) {
    __shared__ double lds[kWaves];
    double acc = 0;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads)
        acc += qchain_term<T>(qchain_coef<T>(i, n, lambda), x[i], i + 1 < n ? x[i + 1] : (T)0);
    const double r = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void qchain_grad_kernel(int64_t n, T *__restrict__ g, const T *__restrict__ x, T lambda) {
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads)
        g[i] = qchain_grad_coef<T>(qchain_coef<T>(i, n, lambda), i > 0 ? x[i - 1] : (T)0, x[i], i + 1 < n ? x[i + 1] : (T)0);
}

// Fused tail of an accepted L-BFGS step for the chained Rosenbrock objective (K3 + K5 + K12):
//   delta_point    = x - x_old                       (src/DZOptimization.jl:145)
//   g_new          = grad f(x)                       (:479)
//   delta_gradient = g_new - g_old                   (:478,:480)
//   partials of rho = delta_point . delta_gradient   (:505)
// One pass: reads x, x_old (in dx), g_old; writes dx, g (in place), dg.  6n elements instead of
// the 11n of the four separate passes (axpby 3n, copy 2n, gradient 2n, delta+rho 4n).  Neighbour
// values for the gradient stencil come from wave shuffles; only lanes 0 / 63 touch memory again.
template <typename T>
__global__ __launch_bounds__(kBlock) void rosen_accept_grad_delta_kernel(int64_t n, const T *__restrict__ x,
                                                                         T *dx, T *g,
                                                                         T *__restrict__ dg,
                                                                         double *__restrict__ partials,
                                                                         const int32_t *__restrict__ gate,
                                                                         const T *xold, const T *gold) {
    // xold / gold: where x_old and g_old are read from -- dx and g themselves on the ordinary path
    // (in place), the single pass's backups after its first trial was rejected (no restore copies)
    constexpr int N = Vec16<T>::N;
    constexpr int U = 2;
    __shared__ double lds[kWaves];
    // speculative launch: the host enqueues this kernel before it knows whether the trial was
    // accepted; the device-side decision (decide_kernel) gates it
    if (gate && *gate != 1) return;
    const int lane = threadIdx.x & 63;
    double acc = 0;
    const int64_t nvec = n / N;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * U; base < nvec; base += nthreads * U) {
        T xv[U][N], xo[U][N], go[U][N];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t v = base + (int64_t)u * kBlock + threadIdx.x;
            ok[u] = v < nvec;
            if (ok[u]) { load16(x + v * N, xv[u]); load16(xold + v * N, xo[u]); load16(gold + v * N, go[u]); }
            else {
#pragma unroll
                for (int j = 0; j < N; ++j) { xv[u][j] = 0; xo[u][j] = 0; go[u][j] = 0; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t v = base + (int64_t)u * kBlock + threadIdx.x;
            const int64_t i = v * N;
            // neighbours: previous lane's last element, next lane's first element
            T xprev = lane_prev<T>(xv[u][N - 1]);
            T xnext = lane_next<T>(xv[u][0]);
            if (ok[u]) {
                if (lane == 0) xprev = i > 0 ? x[i - 1] : (T)0;
                if (lane == 63 || v + 1 >= nvec) xnext = (i + N < n) ? x[i + N] : (T)0;
                T gn[N], dxn[N], dgn[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const T xp = j > 0 ? xv[u][(j + N - 1) % N] : xprev;
                    const T xn = j + 1 < N ? xv[u][(j + 1) % N] : xnext;
                    gn[j] = rosen_grad_elem<T>(i + j, n, xp, xv[u][j], xn);
                    dxn[j] = xv[u][j] - xo[u][j];
                    dgn[j] = gn[j] - go[u][j];
                    acc = __builtin_fma((double)dxn[j], (double)dgn[j], acc);
                }
                store16(dx + i, dxn);
                store16(g + i, gn);
                store16(dg + i, dgn);
            }
        }
    }
    // scalar tail
    const int64_t t = nvec * N + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) {
        const T gn = rosen_grad_elem<T>(t, n, t > 0 ? x[t - 1] : (T)0, x[t], t + 1 < n ? x[t + 1] : (T)0);
        const T dxn = x[t] - xold[t];
        const T dgn = gn - gold[t];
        acc = __builtin_fma((double)dxn, (double)dgn, acc);
        dx[t] = dxn; g[t] = gn; dg[t] = dgn;
    }
    const double r = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// Trial point + objective in one pass (K2 + K12): x = fma(t, d, x_old) (src/DZOptimization.jl:124,
// bit-identical to trial_kernel), the "any element changed" flag (:128), the backup of x_old on
// the first trial (:118) and the per-block partial sums of every objective term f_i(x_i, x_{i+1})
// whose two elements are held by one wave-row (64 lanes x 16 B): the right-hand neighbour of a
// lane's last element comes from the next lane by shuffle.  The terms that straddle two rows
// (one per 64 vectors) and the scalar tail are summed by rosen_edge_terms_kernel afterwards --
// they cannot be formed here because on the first trial x is overwritten in place by other
// waves.  Saves the objective kernel's own pass over x (n T per trial).
template <typename T, bool FIRST>
__global__ __launch_bounds__(kBlock) void rosen_trial_eval_kernel(int64_t n, T *x, T *__restrict__ backup,
                                                                  const T *__restrict__ d, T t,
                                                                  int32_t *__restrict__ changed,
                                                                  double *__restrict__ partials) {
    constexpr int N = Vec16<T>::N;
    constexpr int U = 4;
    __shared__ double lds[kWaves];
    __shared__ int lds_flag;
    const int lane = threadIdx.x & 63;
    const int64_t nvec = n / N;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    const T *src = FIRST ? x : backup;
    bool diff = false;
    double acc = 0;
    for (int64_t base = (int64_t)blockIdx.x * kBlock * U; base < nvec; base += nthreads * U) {
        T xo[U][N], dv[U][N];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t v = base + (int64_t)u * kBlock + threadIdx.x;
            ok[u] = v < nvec;
            if (ok[u]) {
                load16(src + v * N, xo[u]);
                load16(d + v * N, dv[u]);
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) { xo[u][j] = (T)0; dv[u][j] = (T)0; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t v = base + (int64_t)u * kBlock + threadIdx.x;
            T xn[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                xn[j] = dfma(t, dv[u][j], xo[u][j]);                 // :124
                diff |= ok[u] && !is_equal(xn[j], xo[u][j]);         // :128
            }
            const T xnext = lane_next<T>(xn[0]);
            // the row's last vector (lane 63, or the last vector of x) leaves its final term to the edge kernel
            const bool has_next = lane != 63 && v + 1 < nvec;
            if (ok[u]) {
#pragma unroll
                for (int j = 0; j + 1 < N; ++j) acc += rosen_term<T>(xn[j], xn[j + 1]);
                if (has_next) acc += rosen_term<T>(xn[N - 1], xnext);
                store16(x + v * N, xn);
                if (FIRST) store16(backup + v * N, xo[u]);           // :118
            }
        }
    }
    // scalar tail (n not a multiple of the vector width): the point only; its terms are edge terms
    const int64_t e = nvec * N + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < n) {
        const T xo = src[e];
        const T xn = dfma(t, d[e], xo);
        diff |= !is_equal(xn, xo);
        if (FIRST) backup[e] = xo;
        x[e] = xn;
    }
    block_raise_flag(diff, changed, &lds_flag);
    const double r = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// Objective terms that straddle two wave-rows of rosen_trial_eval_kernel, one thread per row, plus
// the terms of the scalar tail.  Reads the finished x (2 elements per term).
template <typename T>
__global__ __launch_bounds__(kBlock) void rosen_edge_terms_kernel(int64_t n, const T *__restrict__ x,
                                                                  double *__restrict__ partials) {
    constexpr int N = Vec16<T>::N;
    __shared__ double lds[kWaves];
    const int64_t nvec = n / N;
    const int64_t rows = (nvec + 63) / 64;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc = 0;
    if (r < rows) {
        const int64_t vend = (r + 1) * 64 < nvec ? (r + 1) * 64 : nvec;   // one past the row's last vector
        const int64_t i = vend * N - 1;
        if (i + 1 < n) acc += rosen_term<T>(x[i], x[i + 1]);
    }
    if (r == 0) {
        for (int64_t e = nvec * N; e + 1 < n; ++e) acc += rosen_term<T>(x[e], x[e + 1]);
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ------------------------------------------------------------------ dense quadratic (config 2)
// One block per column j of the column-major symmetric A: c_j = A[:,j].x (coalesced along
// the column), g_j = c_j, and the objective partial is x_j*c_j.  No cross-block reduction.
template <typename T, bool WRITE_G>
__global__ __launch_bounds__(kBlock) void quadratic_kernel(int64_t n, const T *__restrict__ A,
                                                           const T *__restrict__ x, T *__restrict__ g,
                                                           double *__restrict__ partials) {
    constexpr int N = Vec16<T>::N;
    __shared__ double lds[kWaves];
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const T *col = A + j * n;
        double acc = 0;
        const bool vec = ((n % N) == 0);  // column starts stay 16-B aligned
        if (vec) {
            for (int64_t i = (int64_t)threadIdx.x * N; i < n; i += (int64_t)kBlock * N) {
                T av[N], xv[N];
                load16(col + i, av);
                load16(x + i, xv);
#pragma unroll
                for (int q = 0; q < N; ++q) acc = __builtin_fma((double)av[q], (double)xv[q], acc);
            }
        } else {
            for (int64_t i = threadIdx.x; i < n; i += kBlock) acc = __builtin_fma((double)col[i], (double)x[i], acc);
        }
        double c = block_sum(acc, lds);
        if (threadIdx.x == 0) {
            if (WRITE_G) g[j] = (T)c;
            else partials[j] = c * (double)x[j];
        }
    }
}

__global__ __launch_bounds__(kBlock) void finish_scaled_sum_kernel(const double *__restrict__ partials, int64_t count,
                                                                   double scale, double *__restrict__ result) {
    __shared__ double lds[kWaves];
    double v[1] = {0};
    strided_sums<1>(partials, count, v);
    double r = block_sum(v[0], lds);
    if (threadIdx.x == 0) result[0] = scale * r;
}

// One search direction with up to three step sizes evaluated in the same pass over A (the request the search needs
// now plus the one or two it will most likely need next).
template <typename T> struct PhiDir {
    const T *dir;
    T ts[3];
    T *point_out[3];
    const T *ref[3];       // stagnation test against a stored point (may be null) ...
    int ref_req[3];        // ... or against request ref_req[q] of the same direction in this launch (-1: none)
    T *grad_out[3];        // may be null: A*x_t, the gradient at the trial point, is a by-product (c_j = A[:,j].x_t)
    int active[3];
};
// the one request of quadratic_phi_kernel: request 0 of side a
template <typename T> __device__ __forceinline__ PhiDir<T> phi_single_request(const T *dir, T ts, T *point_out, const T *ref) {
    PhiDir<T> d;
#pragma unroll
    for (int r = 0; r < 3; ++r) { d.ts[r] = (T)0; d.point_out[r] = nullptr; d.ref[r] = nullptr; d.ref_req[r] = -1; d.grad_out[r] = nullptr; d.active[r] = 0; }
    d.dir = dir; d.ts[0] = ts; d.point_out[0] = point_out; d.ref[0] = ref; d.active[0] = 1;
    return d;
}

// What ONE thread does for element j of one direction once the column sums c_j = A[:,j].x_t of its requests are known:
// per active request the objective partial x_t[j] c_j, element j of the trial point, of its gradient (a by-product) and the
// bracket's three flags (:71-80 and the :150 stagnation test).  `sum_of(slot)`: the column sum of request slot = 3 side + r
// (asked for active requests only).  The references are read before any point_out store: a reference may be one of this
// launch's own output buffers.  FLAGS_MAY_BE_NULL: the single-request kernel's plain evaluations carry no flags.
template <typename T, bool FLAGS_MAY_BE_NULL = false, typename SumOf>
__device__ __forceinline__ void phi_finish_element(const PhiDir<T> &d, int side, int64_t j, T xo, SumOf sum_of,
                                                   double *__restrict__ partials, int32_t *__restrict__ flags, int64_t n) {
    const T dj = d.dir[j];
    T xt[3], refv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) xt[r] = dfma(d.ts[r], dj, xo);
#pragma unroll
    for (int r = 0; r < 3; ++r) refv[r] = (d.active[r] && d.ref[r]) ? d.ref[r][j] : (T)0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (!d.active[r]) continue;
        const int slot = side * 3 + r;
        const double c = sum_of(slot);
        partials[(int64_t)slot * n + j] = c * (double)xt[r];
        d.point_out[r][j] = xt[r];
        if (d.grad_out[r]) d.grad_out[r][j] = (T)c;              // exactly what quadratic_kernel<WRITE_G> stores
        if (FLAGS_MAY_BE_NULL && !flags) continue;
        if (xo != xt[r]) flags[slot * 3 + 0] = 1;
        if (dj != (T)0) flags[slot * 3 + 1] = 1;
        if (d.ref[r]) { if (!is_equal(xt[r], refv[r])) flags[slot * 3 + 2] = 1; }
        else if (d.ref_req[r] >= 0) { if (!is_equal(xt[r], xt[d.ref_req[r]])) flags[slot * 3 + 2] = 1; }
    }
}

// phi(t) = f(x + ts*dir) for the dense quadratic (legacy/DZOptimization.jl:25-46) without a separate
// trial-point launch: the point is formed on the fly (same fma as phi_point_kernel) and block j
// also stores element j of it and raises the bracket's two flags; finish_scaled_sum_kernel then
// sums the n partials, so the value is bit-identical to the three-launch sequence it replaces.
// (Folding the final sum in as well, "last block done", needs a device-scope fence per block --
// an L2 write-back on this multi-die part: 2.1 ms per step instead of 0.58.)
template <typename T>
__global__ __launch_bounds__(kBlock) void quadratic_phi_kernel(int64_t n, const T *__restrict__ A, const T *__restrict__ x,
                                                               const T *__restrict__ dir, T ts, T *__restrict__ point_out,
                                                               double *__restrict__ partials, int32_t *__restrict__ flags,
                                                               const T *__restrict__ ref) {
    constexpr int N = Vec16<T>::N;
    __shared__ double lds[kWaves];
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const T *col = A + j * n;
        double acc = 0;
        const bool vec = ((n % N) == 0);
        if (vec) {
            for (int64_t i = (int64_t)threadIdx.x * N; i < n; i += (int64_t)kBlock * N) {
                T av[N], xv[N], dv[N];
                load16(col + i, av);
                load16(x + i, xv);
                load16(dir + i, dv);
#pragma unroll
                for (int q = 0; q < N; ++q) acc = __builtin_fma((double)av[q], (double)dfma(ts, dv[q], xv[q]), acc);
            }
        } else {
            for (int64_t i = threadIdx.x; i < n; i += kBlock) acc = __builtin_fma((double)col[i], (double)dfma(ts, dir[i], x[i]), acc);
        }
        const double c = block_sum(acc, lds);
        if (threadIdx.x == 0)
            phi_finish_element<T, true>(phi_single_request<T>(dir, ts, point_out, ref), 0, j, x[j], [&](int) { return c; }, partials, flags, n);
    }
}

// device-driven searches: the requests as the previous round's finish kernel posted them (see quadratic_phi6_kernel)
template <typename T> __device__ __forceinline__ int phi6_take_requests(PhiDir<T> &a, PhiDir<T> &b, const PhiReqDev *__restrict__ dreq) {
    int any = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        a.ts[r] = (T)dreq->ts[0][r]; a.active[r] = dreq->active[0][r]; a.ref_req[r] = dreq->ref_req[0][r];
        b.ts[r] = (T)dreq->ts[1][r]; b.active[r] = dreq->active[1][r]; b.ref_req[r] = dreq->ref_req[1][r];
        any |= a.active[r] | b.active[r];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { a.ref[r] = nullptr; b.ref[r] = nullptr; }
    const int ra = dreq->use_ref[0][0], rb = dreq->use_ref[1][0];
    if (ra) a.ref[0] = ra == 1 ? a.point_out[0] : (ra == 2 ? a.point_out[1] : a.point_out[2]);
    if (rb) b.ref[0] = rb == 1 ? b.point_out[0] : (rb == 2 ? b.point_out[1] : b.point_out[2]);
    return any;
}

// Two line-search evaluations in one pass over A (the two searches of the dense BFGS step run
// side by side, legacy/DZOptimization.jl:922-932): request r evaluates f(x + ts[r]*dir[r]); each A
// column is loaded once and used for both.  Per request the arithmetic is that of
// quadratic_phi_kernel, so every value is bit-identical to a separate evaluation.
template <typename T>
__global__ __launch_bounds__(kBlock) void quadratic_phi6_kernel(int64_t n, const T *__restrict__ A, const T *__restrict__ x,
                                                                PhiDir<T> a, PhiDir<T> b,
                                                                double *__restrict__ partials, int32_t *__restrict__ flags,
                                                                const PhiReqDev *__restrict__ dreq) {
    constexpr int N = Vec16<T>::N;
    __shared__ double lds6[6 * kWaves];
    // device-driven search (dzo_bfgs.hip): which requests run, their step sizes and their :150 references were posted by the
    // previous round's finish kernel; a round behind a finished search does nothing
    if (dreq) { if (!phi6_take_requests<T>(a, b, dreq)) return; }
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const T *col = A + j * n;
        double acc[6] = {0, 0, 0, 0, 0, 0};
        const bool vec = ((n % N) == 0);
        if (vec) {
            for (int64_t i = (int64_t)threadIdx.x * N; i < n; i += (int64_t)kBlock * N) {
                T av[N], xv[N], da[N], db[N];
                load16(col + i, av);
                load16(x + i, xv);
                load16(a.dir + i, da);
                load16(b.dir + i, db);
#pragma unroll
                for (int q = 0; q < N; ++q) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {      // (wave-uniform skips: later rounds carry one or two requests per direction)
                        if (a.active[r]) acc[r] = __builtin_fma((double)av[q], (double)dfma(a.ts[r], da[q], xv[q]), acc[r]);
                        if (b.active[r]) acc[3 + r] = __builtin_fma((double)av[q], (double)dfma(b.ts[r], db[q], xv[q]), acc[3 + r]);
                    }
                }
            }
        } else {
            for (int64_t i = threadIdx.x; i < n; i += kBlock) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    acc[r] = __builtin_fma((double)col[i], (double)dfma(a.ts[r], a.dir[i], x[i]), acc[r]);
                    acc[3 + r] = __builtin_fma((double)col[i], (double)dfma(b.ts[r], b.dir[i], x[i]), acc[3 + r]);
                }
            }
        }
        double c[6];
        block_sum_multi<6>(acc, lds6, c);                  // (inactive requests sum zeros; each value = block_sum of it)
        if (threadIdx.x == 0) {
            const T xo = x[j];
#pragma unroll
            for (int side = 0; side < 2; ++side)
                phi_finish_element<T>(side ? b : a, side, j, xo, [&](int slot) { return c[slot]; }, partials, flags, n);
        }
    }
}

// The same launch with a block walking kPhi6Cols columns at once and two register sets of requests in flight (round 4).  The
// one-column kernel waits for each iteration's four loads before it asks for the next ones (24 KB per CU in flight).  Here
// the loads of iteration it + 1 are on their way while iteration it is computed -- and they are UNCONDITIONAL
// (addresses clamped to the last vector, the sums predicated instead): a prefetch under `if (i < n)` makes the compiler
// wait for vmcnt(0) before the older set may be used, because requests complete in order and a younger request that may
// not have been issued cannot be counted on (that is why the first pipelined forms of this kernel measured nothing,
// profiles/r04_phi6_experiments.md).  x, dir_a, dir_b are loaded and the six trial values formed once per kPhi6Cols columns.
// Element i still belongs to thread (i / N) % 256 in iteration i / (256 N), the per-thread sums run over q, then over the
// iterations, and the block sum is wave_sum + the waves in order: every value is bit for bit what quadratic_phi6_kernel
// (and quadratic_phi_kernel, quadratic_kernel) give.  n % N == 0 only.
// Two columns, ONE set ahead, 108 registers = four blocks per CU in fp64 (two in fp32), so that the 2048 groups of config 2
// are two full rounds of the 1024 resident blocks: 27.3 us per round against the one-column kernel's 32.4.  (Two sets ahead,
// 140 registers, three blocks per CU: 28.8 us; four columns: 30.2 us; forms pressed into more blocks per CU than their
// registers allow spill and lose everything, 35-55 us.  Both were retired.)
constexpr int kPhi6Cols = 2;
template <typename T>
__global__ __launch_bounds__(kBlock, (sizeof(T) == 8 ? 4 : 2)) void quadratic_phi6_cols_kernel(int64_t n, const T *__restrict__ A, const T *__restrict__ x,
                                                                     PhiDir<T> a, PhiDir<T> b,
                                                                     double *__restrict__ partials, int32_t *__restrict__ flags,
                                                                     const PhiReqDev *__restrict__ dreq) {
    constexpr int N = Vec16<T>::N;
    constexpr int CG = kPhi6Cols;
    __shared__ double lds[CG * 6 * kWaves];
    if (dreq) { if (!phi6_take_requests<T>(a, b, dreq)) return; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t groups = (n + CG - 1) / CG;
    const int64_t st = (int64_t)kBlock * N;
    const int64_t i0 = (int64_t)threadIdx.x * N;
    const int iters = (int)((n + st - 1) / st);                             // (uniform; a thread's own count may be one less)
    const int64_t ilast = n - N;
    struct Tile { T av[CG][N], xv[N], da[N], db[N]; };
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t j0 = grp * CG;
        double acc[CG][6];
#pragma unroll
        for (int c = 0; c < CG; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[c][r] = 0;
        auto fetch = [&](Tile &t, int it) {                                  // always issued; past the end: the last vector again
            int64_t i = i0 + (int64_t)it * st;
            i = i < n ? i : ilast;
#pragma unroll
            for (int c = 0; c < CG; ++c) {
                const int64_t jc = j0 + c < n ? j0 + c : n - 1;              // (a column past the end: loaded, never used)
                load16(A + jc * n + i, t.av[c]);
            }
            load16(x + i, t.xv);
            load16(a.dir + i, t.da);
            load16(b.dir + i, t.db);
        };
        auto consume = [&](const Tile &t, int it) {
            if (i0 + (int64_t)it * st >= n) return;
            double xt[6][N];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    xt[r][q] = a.active[r] ? (double)dfma(a.ts[r], t.da[q], t.xv[q]) : 0.0;
                    xt[3 + r][q] = b.active[r] ? (double)dfma(b.ts[r], t.db[q], t.xv[q]) : 0.0;
                }
            }
#pragma unroll
            for (int c = 0; c < CG; ++c) {
#pragma unroll
                for (int q = 0; q < N; ++q) {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {                              // (wave-uniform skips, as in the one-column kernel)
                        if (a.active[r]) acc[c][r] = __builtin_fma((double)t.av[c][q], xt[r][q], acc[c][r]);
                        if (b.active[r]) acc[c][3 + r] = __builtin_fma((double)t.av[c][q], xt[3 + r][q], acc[c][3 + r]);
                    }
                }
            }
        };
        Tile t0, t1;
        fetch(t0, 0);
        int it = 0;
        for (; it + 2 <= iters; it += 2) {
            fetch(t1, it + 1); consume(t0, it);
            fetch(t0, it + 2); consume(t1, it + 1);
        }
        if (it < iters) consume(t0, it);
#pragma unroll
        for (int c = 0; c < CG; ++c) {
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const int on = r < 3 ? a.active[r] : b.active[r - 3];
                if (!on) continue;                                           // (uniform; an inactive request's sum is never read)
                const double w = wave_sum(acc[c][r]);
                if (lane == 0) lds[(c * 6 + r) * kWaves + wave] = w;
            }
        }
        __syncthreads();
        if (threadIdx.x < CG && j0 + threadIdx.x < n) {
            const int c = threadIdx.x;
            const int64_t j = j0 + c;
            const T xo = x[j];
            auto sum_of = [&](int slot) {
                double cs = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) cs += lds[(c * 6 + slot) * kWaves + w];
                return cs;
            };
#pragma unroll
            for (int side = 0; side < 2; ++side) phi_finish_element<T>(side ? b : a, side, j, xo, sum_of, partials, flags, n);
        }
        __syncthreads();
    }
}

// values to out[0..5], flags {changed, nonzero, differs from ref} of request q to the int32 view of
// out[8..] at 3q; flags re-armed
__global__ __launch_bounds__(kBlock) void finish_phi6_kernel(const double *__restrict__ partials, int64_t count, double scale,
                                                             double *__restrict__ out, int32_t *__restrict__ flags, double ticket) {
    __shared__ double lds6[6 * kWaves];
    double v[6] = {0, 0, 0, 0, 0, 0};
    strided_sums<6>(partials, count, v);
    double sres[6];
    block_sum_multi<6>(v, lds6, sres);
    if (threadIdx.x == 0) {
        unsigned long long seal = seal_bits(ticket);             // (wait_sealed: out[0..16], seal in out[17])
#pragma unroll
        for (int r = 0; r < 6; ++r) { const double v = scale * sres[r]; out[r] = v; seal ^= seal_bits(v); }
        out[6] = 0; out[7] = 0;
        int32_t *ho = reinterpret_cast<int32_t *>(out + 8);
        for (int q = 0; q < 18; q += 2) {
            const int32_t f0 = flags[q], f1 = flags[q + 1];
            flags[q] = 0; flags[q + 1] = 0;
            ho[q] = f0; ho[q + 1] = f1;
            seal ^= (unsigned long long)(uint32_t)f0 | ((unsigned long long)(uint32_t)f1 << 32);
        }
        store_seal(out + 17, seal);
        __threadfence_system();
        out[20] = ticket;                                        // the host spins on this word (wait_ticket)
        __threadfence_system();
    }
}

// finish of quadratic_phi_kernel: value and the three flags straight into the pinned host buffer
// (out[0] = f, int32 view of out[4..5] = flags), flags re-armed for the next evaluation
__global__ __launch_bounds__(kBlock) void finish_phi_kernel(const double *__restrict__ partials, int64_t count, double scale,
                                                            double *__restrict__ out, int32_t *__restrict__ flags) {
    __shared__ double lds[kWaves];
    double v[1] = {0};
    strided_sums<1>(partials, count, v);
    const double r = block_sum(v[0], lds);
    if (threadIdx.x == 0) {
        out[0] = scale * r;
        if (flags) {
            int32_t *ho = reinterpret_cast<int32_t *>(out + 4);
            ho[0] = flags[0]; ho[1] = flags[1]; ho[2] = flags[2];
            flags[0] = 0; flags[1] = 0; flags[2] = 0;
        }
        __threadfence_system();
    }
}

// ------------------------------------------------------------------ log-sum-exp (config 4)
template <typename T>
__global__ __launch_bounds__(kBlock) void lse_max_kernel(int64_t n, const T *__restrict__ x,
                                                         double *__restrict__ partials) {
    __shared__ double lds[kWaves];
    double mx = -1.7976931348623157e308;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) mx = fmax(mx, (double)x[i]);
    const double r = block_max(mx, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}
__global__ __launch_bounds__(kBlock) void lse_finish_max_kernel(const double *__restrict__ partials, int count,
                                                                double *__restrict__ result) {
    __shared__ double lds[kWaves];
    double mx = -1.7976931348623157e308;
    for (int i = threadIdx.x; i < count; i += kBlock) mx = fmax(mx, partials[i]);
    const double r = block_max(mx, lds);
    if (threadIdx.x == 0) result[0] = r;
}
// partials[b] = sum exp(x - mx), partials[grid + b] = sum (x - c)^2
template <typename T>
__global__ __launch_bounds__(kBlock) void lse_sums_kernel(int64_t n, const T *__restrict__ x, const T *__restrict__ c,
                                                          const double *__restrict__ mx_dev,
                                                          double *__restrict__ partials) {
    __shared__ double lds[kWaves];
    const T mx = (T)mx_dev[0];
    double se = 0, sq = 0;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
        se += exp((double)(x[i] - mx));
        const T dlt = x[i] - c[i];
        sq = __builtin_fma((double)dlt, (double)dlt, sq);
    }
    double r1 = block_sum(se, lds);
    double r2 = block_sum(sq, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = r1;
        partials[gridDim.x + blockIdx.x] = r2;
    }
}
// result[0] = mx + log(se) + lambda/2 * sq ; result[1] = se
__global__ __launch_bounds__(kBlock) void lse_finish_kernel(const double *__restrict__ partials, int count,
                                                            const double *__restrict__ mx_dev, double lambda,
                                                            double *__restrict__ result) {
    __shared__ double lds[kWaves];
    double se = reduce_partials_all(partials, count, lds);
    double sq = reduce_partials_all(partials + count, count, lds);
    if (threadIdx.x == 0) {
        result[1] = se;
        result[0] = mx_dev[0] + log(se) + 0.5 * lambda * sq;
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void lse_grad_kernel(int64_t n, T *__restrict__ g, const T *__restrict__ x,
                                                          const T *__restrict__ c, const double *__restrict__ mx_dev,
                                                          const double *__restrict__ se_dev, double lambda) {
    const T mx = (T)mx_dev[0];
    const double se = se_dev[0];
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
        const double sm = exp((double)(x[i] - mx)) / se;
        g[i] = (T)(sm + lambda * (double)(x[i] - c[i]));
    }
}

// ------------------------------------------------------------------ decorators (legacy :219-296)
template <typename T>
__global__ __launch_bounds__(kBlock) void box_clamp_kernel(int64_t n, T *__restrict__ x, T lo, T hi) {
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
        const T v = x[i];
        x[i] = v < lo ? lo : (v > hi ? hi : v);              // clamp(x[i], lo, hi) :269
    }
}
// L2GradientWrapper (:247) then UniformBoxGradientWrapper (:289-294), one pass over g
template <typename T>
__global__ __launch_bounds__(kBlock) void grad_decorate_kernel(int64_t n, T *__restrict__ g, const T *__restrict__ x,
                                                               T two_lambda, int box, T lo, T hi) {
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) {
        T gi = g[i];
        const T xi = x[i];
        if (two_lambda != (T)0) gi = dfma(two_lambda, xi, gi);
        if (box && ((xi <= lo && gi >= (T)0) || (xi >= hi && gi <= (T)0))) gi = (T)0;
        g[i] = gi;
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void sumsq_kernel(int64_t n, const T *__restrict__ x, double *__restrict__ partials) {
    __shared__ double lds[kWaves];
    double acc = 0;
    const int64_t nthreads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthreads) acc = __builtin_fma((double)x[i], (double)x[i], acc);
    const double r = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}
// result[0] = f + lambda * norm2(x)  (:232), in T arithmetic
__global__ __launch_bounds__(kBlock) void l2_finish_kernel(const double *__restrict__ partials, int count, double lambda,
                                                           int to_f32, double *__restrict__ result) {
    __shared__ double lds[kWaves];
    const double ss = reduce_partials_all(partials, count, lds);
    if (threadIdx.x == 0) {
        if (to_f32) result[0] = (double)((float)result[0] + (float)lambda * (float)ss);
        else result[0] = result[0] + lambda * ss;
    }
}

int32_t box_clamp_async(hipStream_t s, int64_t n, int32_t dtype, void *x, double lo, double hi) {
    DZO_TIMED("box_clamp", s);
    const int grid = stream_grid(n, 4);
    DZO_DISPATCH(dtype, hipLaunchKernelGGL(box_clamp_kernel<T>, dim3(grid), dim3(kBlock), 0, s, n, (T *)x, (T)lo, (T)hi));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

// ------------------------------------------------------------------ host side
// f(T{}) with T the problem's element type, for launches in functions that do not return a status (DZO_DISPATCH's
// error branch returns an int32_t)
template <typename F> static inline void with_dtype(int32_t dtype, F &&f) {
    if (dtype == DZO_F64) f(double{}); else f(float{});
}
// one block per column (or group of columns) of the dense quadratic's A
static inline int quad_grid(int64_t columns) { return (int)(columns < 65535 ? columns : 65535); }

// The three objectives whose value is a plain scaled sum of per-block partials: their profile name (null for every
// other kind) and the launch that leaves the partials.
static const char *scaled_sum_objective(int32_t kind) {
    switch (kind) {
    case DZO_PROBLEM_ROSENBROCK_CHAIN: return "objective_rosenbrock_chain";
    case DZO_PROBLEM_QUADRATIC: return "objective_quadratic";
    case DZO_PROBLEM_QUADRATIC_CHAIN: return "objective_quadratic_chain";
    default: return nullptr;
    }
}
template <typename T>
static void eval_partials_t(dzo_problem_s *p, hipStream_t s, const T *x, const double **partials, int64_t *count, double *scale) {
    const int64_t n = p->n;
    *partials = p->scratch; *scale = 1.0;
    if (p->kind == DZO_PROBLEM_ROSENBROCK_CHAIN) {
        const int grid = stream_grid(n, Vec16<T>::N * 2);
        hipLaunchKernelGGL(rosen_chain_eval_kernel<T>, dim3(grid), dim3(kBlock), 0, s, n, x, p->scratch);
        *count = grid;
    } else if (p->kind == DZO_PROBLEM_QUADRATIC_CHAIN) {
        const int grid = stream_grid(n, 4);
        hipLaunchKernelGGL(qchain_eval_kernel<T>, dim3(grid), dim3(kBlock), 0, s, n, x, (T)p->lambda, p->scratch);
        *count = grid;
    } else {                                                     // DZO_PROBLEM_QUADRATIC
        hipLaunchKernelGGL((quadratic_kernel<T, false>), dim3(quad_grid(n)), dim3(kBlock), 0, s, n, (const T *)p->A, x,
                           (T *)nullptr, p->scratch);
        *count = n; *scale = 0.5;
    }
}

// The scalars of the log-sum-exp objective, shared by its value and its gradient: max, its finish, the two sums, their finish.
struct LseScalars { double *mx, *res; };                         // [mx], [f, se], behind the partials in the problem's scratch
template <typename T> static LseScalars lse_scalars_launch(dzo_problem_s *p, hipStream_t s, const T *x, int grid) {
    const LseScalars k = {p->scratch + 2 * kMaxPartialBlocks, p->scratch + 2 * kMaxPartialBlocks + 2};
    hipLaunchKernelGGL(lse_max_kernel<T>, dim3(grid), dim3(kBlock), 0, s, p->n, x, p->scratch);
    hipLaunchKernelGGL(lse_finish_max_kernel, dim3(1), dim3(kBlock), 0, s, p->scratch, grid, k.mx);
    hipLaunchKernelGGL(lse_sums_kernel<T>, dim3(grid), dim3(kBlock), 0, s, p->n, x, (const T *)p->c, k.mx, p->scratch);
    hipLaunchKernelGGL(lse_finish_kernel, dim3(1), dim3(kBlock), 0, s, p->scratch, grid, k.mx, p->lambda, k.res);
    return k;
}

template <typename T> static int32_t eval_async_t(dzo_problem_s *p, hipStream_t s, const T *x, double *result_dev) {
    const int64_t n = p->n;
    switch (p->kind) {
    case DZO_PROBLEM_ROSENBROCK2D: {
        DZO_TIMED("objective_rosenbrock2d", s);
        hipLaunchKernelGGL(rosen2d_eval_kernel<T>, dim3(1), dim3(64), 0, s, x, result_dev);
        break;
    }
    case DZO_PROBLEM_ROSENBROCK_CHAIN:
    case DZO_PROBLEM_QUADRATIC:
    case DZO_PROBLEM_QUADRATIC_CHAIN: {
        DZO_TIMED(scaled_sum_objective(p->kind), s);
        const double *partials; int64_t count; double scale;
        eval_partials_t<T>(p, s, x, &partials, &count, &scale);
        hipLaunchKernelGGL(finish_scaled_sum_kernel, dim3(1), dim3(kBlock), 0, s, partials, count, scale, result_dev);
        break;
    }
    case DZO_PROBLEM_LSE: {
        DZO_TIMED("objective_lse", s);
        const LseScalars k = lse_scalars_launch<T>(p, s, x, stream_grid(n, 4));
        DZO_HIP(hipMemcpyAsync(result_dev, k.res, sizeof(double), hipMemcpyDeviceToDevice, s));
        break;
    }
    case DZO_PROBLEM_PAIRWISE_LJ: {                          // point = [x | y | z], N = n / 3 (dzo_pairwise.hip)
        DZO_TIMED("objective_pairwise_lj", s);
        const int64_t N = n / 3;
        DZO_TRY(pairwise_energy_async(s, DZO_RADIAL_LENNARD_JONES, N, p->dtype, x, x + N, x + 2 * N, p->scratch, result_dev));
        break;
    }
    default:
        set_error("unknown problem kind %d", p->kind);
        return DZO_ERR_INVALID;
    }
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

template <typename T> static int32_t grad_async_t(dzo_problem_s *p, hipStream_t s, T *g, const T *x) {
    const int64_t n = p->n;
    switch (p->kind) {
    case DZO_PROBLEM_ROSENBROCK2D: {
        DZO_TIMED("gradient_rosenbrock2d", s);
        hipLaunchKernelGGL(rosen2d_grad_kernel<T>, dim3(1), dim3(64), 0, s, g, x);
        break;
    }
    case DZO_PROBLEM_ROSENBROCK_CHAIN: {
        DZO_TIMED("gradient_rosenbrock_chain", s);
        hipLaunchKernelGGL(rosen_chain_grad_kernel<T>, dim3(stream_grid(n, Vec16<T>::N * 2)), dim3(kBlock), 0, s, n,
                           g, x);
        break;
    }
    case DZO_PROBLEM_QUADRATIC: {
        DZO_TIMED("gradient_quadratic", s);
        hipLaunchKernelGGL((quadratic_kernel<T, true>), dim3(quad_grid(n)), dim3(kBlock), 0, s, n, (const T *)p->A, x, g,
                           (double *)nullptr);
        break;
    }
    case DZO_PROBLEM_QUADRATIC_CHAIN: {
        DZO_TIMED("gradient_quadratic_chain", s);
        hipLaunchKernelGGL(qchain_grad_kernel<T>, dim3(stream_grid(n, 4)), dim3(kBlock), 0, s, n, g, x, (T)p->lambda);
        break;
    }
    case DZO_PROBLEM_LSE: {
        DZO_TIMED("gradient_lse", s);
        const int grid = stream_grid(n, 4);
        const LseScalars k = lse_scalars_launch<T>(p, s, x, grid);
        hipLaunchKernelGGL(lse_grad_kernel<T>, dim3(grid), dim3(kBlock), 0, s, n, g, x, (const T *)p->c, k.mx, k.res + 1,
                           p->lambda);
        break;
    }
    case DZO_PROBLEM_PAIRWISE_LJ: {
        DZO_TIMED("gradient_pairwise_lj", s);
        const int64_t N = n / 3;
        DZO_TRY(pairwise_gradient_async(s, DZO_RADIAL_LENNARD_JONES, N, p->dtype, g, g + N, g + 2 * N, x, x + N, x + 2 * N, p->scratch));
        break;
    }
    default:
        set_error("unknown problem kind %d", p->kind);
        return DZO_ERR_INVALID;
    }
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

bool problem_has_fused_post(const dzo_problem_s *p, const void *x, const void *dx, const void *g, const void *dg) {
    auto al = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    return p && p->kind == DZO_PROBLEM_ROSENBROCK_CHAIN && p->l2 == 0.0 && !p->bg_on && al(x) && al(dx) && al(g) && al(dg);
}

int32_t problem_fused_post_async(dzo_problem_s *p, hipStream_t s, const void *x, void *dx, void *g, void *dg,
                                 double *partials, int *grid_out, const int32_t *gate, const void *xold_src, const void *gold_src) {
    const int64_t n = p->n;
    DZO_TIMED("lbfgs_fused_accept_grad_delta", s);
    const int vecn = p->dtype == DZO_F64 ? 2 : 4;
    const int grid = stream_grid(n, vecn * 2);
    const void *xo = xold_src ? xold_src : dx, *go = gold_src ? gold_src : g;
    with_dtype(p->dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(rosen_accept_grad_delta_kernel<T>, dim3(grid), dim3(kBlock), 0, s, n, (const T *)x, (T *)dx, (T *)g, (T *)dg,
                           partials, gate, (const T *)xo, (const T *)go);
    });
    *grid_out = grid;
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

// Fused trial point + objective partials (chained Rosenbrock, 16-B aligned operands, no decorators).
bool problem_trial_eval_async(dzo_problem_s *p, hipStream_t s, void *x, void *backup, const void *d, double t,
                              bool first, int32_t *changed, const double **partials, int64_t *count, double *scale) {
    if (!p || p->kind != DZO_PROBLEM_ROSENBROCK_CHAIN || p->l2 != 0.0 || p->cons_on) return false;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(backup) | reinterpret_cast<uintptr_t>(d)) & 15u) != 0) return false;
    const int64_t n = p->n;
    const int vecn = p->dtype == DZO_F64 ? 2 : 4;
    const int grid = stream_grid(n, vecn * 4);
    const int64_t rows = (n / vecn + 63) / 64;
    int egrid = (int)((rows + kBlock - 1) / kBlock);
    if (egrid < 1) egrid = 1;
    if ((int64_t)grid + egrid > 2 * kMaxPartialBlocks) return false;    // partials live in p->scratch
    with_dtype(p->dtype, [&](auto tag) {
        using T = decltype(tag);
        {
            DZO_TIMED("lbfgs_trial_objective", s);
            hipLaunchKernelGGL((first ? rosen_trial_eval_kernel<T, true> : rosen_trial_eval_kernel<T, false>), dim3(grid), dim3(kBlock), 0, s,
                               n, (T *)x, (T *)backup, (const T *)d, (T)t, changed, p->scratch);
        }
        {
            DZO_TIMED("objective_edge_terms", s);
            hipLaunchKernelGGL(rosen_edge_terms_kernel<T>, dim3(egrid), dim3(kBlock), 0, s, n, (const T *)x, p->scratch + grid);
        }
    });
    *partials = p->scratch; *count = grid + egrid; *scale = 1.0;
    return true;
}

// f(x + ts*dir) of the dense quadratic in one launch; also materialises the trial point.  false when
// this objective / these options have no such kernel.
bool problem_phi_async(dzo_problem_s *p, hipStream_t s, const void *x, const void *dir, double ts, void *point_out,
                       int32_t *flags, double *result_dev, const void *ref) {
    if (!p || p->kind != DZO_PROBLEM_QUADRATIC || p->l2 != 0.0 || p->cons_on) return false;
    const int64_t n = p->n;
    DZO_TIMED("objective_quadratic_phi", s);
    with_dtype(p->dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(quadratic_phi_kernel<T>, dim3(quad_grid(n)), dim3(kBlock), 0, s, n, (const T *)p->A, (const T *)x,
                           (const T *)dir, (T)ts, (T *)point_out, p->scratch, flags, (const T *)ref);
    });
    hipLaunchKernelGGL(finish_phi_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)p->scratch, n, 0.5, result_dev, flags);
    return true;
}

// Up to three step sizes along each of two directions in one pass over A.  req[side] describes the
// requests (inactive ones are skipped); values and flags land in result_dev (>= 17 doubles, may be
// pinned host memory): values [0..5], int32 flags from [8].  `flags`: 18 zeroed int32 on the device.
bool problem_phi6_async(dzo_problem_s *p, hipStream_t s, const void *x, const PhiDirHost req[2], int32_t *flags, double *result_dev, double ticket,
                        const PhiReqDev *dreq) {
    if (!p || p->kind != DZO_PROBLEM_QUADRATIC || p->l2 != 0.0 || p->cons_on) return false;
    const int64_t n = p->n;
    if (p->scratch_doubles < 6 * n) return false;
    DZO_TIMED("objective_quadratic_phi", s);
    with_dtype(p->dtype, [&](auto tag) {
        using T = decltype(tag);
        PhiDir<T> d[2];
        for (int side = 0; side < 2; ++side) {
            d[side].dir = (const T *)req[side].dir;
            for (int r = 0; r < 3; ++r) {
                d[side].ts[r] = (T)req[side].ts[r];
                d[side].point_out[r] = (T *)req[side].point_out[r];
                d[side].ref[r] = (const T *)req[side].ref[r];
                d[side].ref_req[r] = req[side].ref_req[r];
                d[side].grad_out[r] = (T *)req[side].grad_out[r];
                d[side].active[r] = req[side].active[r] ? 1 : 0;
            }
        }
        // DZO_TUNE_PHI6_COLS=1: the one-column kernel everywhere (32.4 us per round at config 2 against 27.3); it is the
        // only form for a ragged or a small n
        const bool one_col = n % Vec16<T>::N != 0 || n < 64 || tune_int("DZO_TUNE_PHI6_COLS", 0) == 1;
        const int ggrid = quad_grid(one_col ? n : (n + kPhi6Cols - 1) / kPhi6Cols);
        hipLaunchKernelGGL(one_col ? quadratic_phi6_kernel<T> : quadratic_phi6_cols_kernel<T>, dim3(ggrid), dim3(kBlock), 0, s, n,
                           (const T *)p->A, (const T *)x, d[0], d[1], p->scratch, flags, dreq);
    });
    if (dreq) return true;                                       // (the caller's finish kernel sums, advances the searches and posts the next requests)
    hipLaunchKernelGGL(finish_phi6_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)p->scratch, n, 0.5, result_dev, flags, ticket);
    return true;
}

// Objective WITHOUT its final one-block sum: leaves per-block partials so that the caller's
// decision kernel can do the sum itself (one launch fewer per trial).  Returns false for the
// objectives whose finish is not a plain scaled sum.
bool problem_eval_partials_async(dzo_problem_s *p, hipStream_t s, const void *x, const double **partials,
                                 int64_t *count, double *scale) {
    if (p->l2 != 0.0 || !scaled_sum_objective(p->kind)) return false;
    DZO_TIMED(scaled_sum_objective(p->kind), s);
    with_dtype(p->dtype, [&](auto tag) {
        using T = decltype(tag);
        eval_partials_t<T>(p, s, (const T *)x, partials, count, scale);
    });
    return true;
}

int32_t problem_eval_async(dzo_problem_s *p, hipStream_t s, const void *x, double *result_dev) {
    DZO_DISPATCH(p->dtype, DZO_TRY(eval_async_t<T>(p, s, (const T *)x, result_dev)));
    if (p->l2 != 0.0) {                                      // L2RegularizationWrapper (:231-232)
        DZO_TIMED("objective_l2_term", s);
        const int grid = stream_grid(p->n, 4);
        double *part = p->scratch;                           // the base evaluation's partials are consumed
        DZO_DISPATCH(p->dtype, hipLaunchKernelGGL(sumsq_kernel<T>, dim3(grid), dim3(kBlock), 0, s, p->n, (const T *)x, part));
        hipLaunchKernelGGL(l2_finish_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)part, grid, p->l2,
                           p->dtype == DZO_F32 ? 1 : 0, result_dev);
        DZO_HIP(hipGetLastError());
    }
    return DZO_OK;
}
int32_t problem_grad_async(dzo_problem_s *p, hipStream_t s, void *g, const void *x) {
    DZO_DISPATCH(p->dtype, DZO_TRY(grad_async_t<T>(p, s, (T *)g, (const T *)x)));
    if (p->l2 != 0.0 || p->bg_on) {                          // L2GradientWrapper, UniformBoxGradientWrapper
        DZO_TIMED("gradient_decorators", s);
        const int grid = stream_grid(p->n, 4);
        const double l2 = p->dtype == DZO_F32 ? (double)((float)p->l2 + (float)p->l2) : p->l2 + p->l2;   // :247 lambda + lambda
        DZO_DISPATCH(p->dtype, hipLaunchKernelGGL(grad_decorate_kernel<T>, dim3(grid), dim3(kBlock), 0, s, p->n, (T *)g,
                                                  (const T *)x, (T)l2, p->bg_on ? 1 : 0, (T)p->bg_lo, (T)p->bg_hi));
        DZO_HIP(hipGetLastError());
    }
    return DZO_OK;
}

static int32_t problem_alloc_workspace(dzo_problem_s *p) {
    const int64_t n = p->n;
    int64_t scratch = (p->kind == DZO_PROBLEM_QUADRATIC ? (6 * n > 2 * kMaxPartialBlocks ? 6 * n : 2 * kMaxPartialBlocks)
                                                        : 2 * kMaxPartialBlocks) + 16;
    if (p->kind == DZO_PROBLEM_PAIRWISE_LJ) {                // row partials of a split j range, energy partials
        const int64_t pw = pairwise_workspace_doubles(n / 3);
        if (pw + 16 > scratch) scratch = pw + 16;
    }
    p->scratch_doubles = scratch - 16;
    hipError_t e = hipMalloc((void **)&p->scratch, sizeof(double) * (size_t)scratch);
    if (e != hipSuccess) { p->scratch = nullptr; return hip_fail(e, "hipMalloc(problem scratch)", __FILE__, __LINE__); }
    e = hipHostMalloc((void **)&p->host, sizeof(double) * 4, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipFree(p->scratch); p->scratch = nullptr; p->host = nullptr; return hip_fail(e, "hipHostMalloc", __FILE__, __LINE__); }
    p->result = p->scratch + scratch - 8;
    return DZO_OK;
}
static void problem_free_workspace(dzo_problem_s *p) {
    if (p->scratch) (void)hipFree(p->scratch);
    if (p->host) (void)hipHostFree(p->host);
}

int32_t problem_view_create(dzo_problem_s *parent, dzo_problem_s **out) {
    dzo_problem_s *root = parent->parent ? parent->parent : parent;
    dzo_problem_s *v = new dzo_problem_s(*root);
    v->parent = root; v->scratch = nullptr; v->result = nullptr; v->host = nullptr;
    const int32_t rc = problem_alloc_workspace(v);
    if (rc != DZO_OK) { delete v; return rc; }
    *out = v;
    return DZO_OK;
}

void problem_view_sync(dzo_problem_s *v) {
    if (!v || !v->parent) return;
    const dzo_problem_s *r = v->parent;
    v->kind = r->kind; v->n = r->n; v->dtype = r->dtype; v->A = r->A; v->c = r->c; v->lambda = r->lambda;
    v->l2 = r->l2; v->bg_on = r->bg_on; v->bg_lo = r->bg_lo; v->bg_hi = r->bg_hi;
    v->cons_on = r->cons_on; v->cons_lo = r->cons_lo; v->cons_hi = r->cons_hi;
}

void problem_view_destroy(dzo_problem_s *v) {
    if (!v || !v->parent) return;                            // only views are owned by optimizers
    problem_free_workspace(v);
    delete v;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_problem_create(int32_t kind, int64_t n, int32_t dtype, const void *A_dev, const void *c_dev,
                           double lambda, dzo_problem_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null out");
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(kind >= 0 && kind <= DZO_PROBLEM_PAIRWISE_LJ, DZO_ERR_INVALID, "unknown problem kind %d", kind);
    DZO_REQUIRE(kind != DZO_PROBLEM_PAIRWISE_LJ || (n >= 3 && n % 3 == 0 && n / 3 <= ((int64_t)1 << 28)), DZO_ERR_INVALID,
                "the pairwise Lennard-Jones objective needs n = 3 N, the point being [x | y | z] (got n = %lld)", (long long)n);
    DZO_REQUIRE(kind != DZO_PROBLEM_QUADRATIC_CHAIN || lambda > 0, DZO_ERR_INVALID, "the chained quadratic needs lambda > 0 (it is what makes it strictly convex)");
    DZO_REQUIRE(n >= 1, DZO_ERR_INVALID, "n must be >= 1");
    DZO_REQUIRE(kind != DZO_PROBLEM_ROSENBROCK2D || n == 2, DZO_ERR_INVALID, "2-D Rosenbrock needs n == 2");
    DZO_REQUIRE(kind != DZO_PROBLEM_QUADRATIC || A_dev, DZO_ERR_INVALID, "quadratic problem needs A");
    DZO_REQUIRE(kind != DZO_PROBLEM_LSE || c_dev, DZO_ERR_INVALID, "LSE problem needs c");
    dzo_problem_s *p = new dzo_problem_s();
    p->kind = kind; p->n = n; p->dtype = dtype; p->A = A_dev; p->c = c_dev; p->lambda = lambda;
    const int32_t rc = problem_alloc_workspace(p);
    if (rc != DZO_OK) { delete p; return rc; }
    *out = p;
    return DZO_OK;
}

int32_t dzo_problem_set_l2(dzo_problem_t p, double lambda) {
    DZO_REQUIRE(p, DZO_ERR_INVALID, "null problem");
    p->l2 = lambda;
    return DZO_OK;
}

int32_t dzo_problem_set_box_gradient(dzo_problem_t p, int32_t enable, double lower_bound, double upper_bound) {
    DZO_REQUIRE(p, DZO_ERR_INVALID, "null problem");
    DZO_REQUIRE(!enable || lower_bound <= upper_bound, DZO_ERR_INVALID, "lower_bound > upper_bound");
    p->bg_on = enable != 0; p->bg_lo = lower_bound; p->bg_hi = upper_bound;
    return DZO_OK;
}

int32_t dzo_problem_set_box_constraint(dzo_problem_t p, int32_t enable, double lower_bound, double upper_bound) {
    DZO_REQUIRE(p, DZO_ERR_INVALID, "null problem");
    DZO_REQUIRE(!enable || lower_bound <= upper_bound, DZO_ERR_INVALID, "lower_bound > upper_bound");
    p->cons_on = enable != 0; p->cons_lo = lower_bound; p->cons_hi = upper_bound;
    return DZO_OK;
}

int32_t dzo_box_clamp(int64_t n, int32_t dtype, void *x_dev, double lower_bound, double upper_bound) {
    DZO_TRY(require_init());
    DZO_REQUIRE(n >= 0 && (x_dev || n == 0), DZO_ERR_INVALID, "bad argument");
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    if (n > 0) DZO_TRY(box_clamp_async(ctx().stream, n, dtype, x_dev, lower_bound, upper_bound));
    DZO_HIP(hipStreamSynchronize(ctx().stream));
    return DZO_OK;
}

int32_t dzo_problem_destroy(dzo_problem_t p) {
    if (!p) return DZO_OK;
    problem_free_workspace(p);
    delete p;
    return DZO_OK;
}

int32_t dzo_problem_eval(dzo_problem_t p, const void *x_dev, double *f) {
    DZO_TRY(require_init());
    DZO_REQUIRE(p && x_dev && f, DZO_ERR_INVALID, "null argument");
    hipStream_t s = ctx().stream;
    DZO_TRY(problem_eval_async(p, s, x_dev, p->result));
    DZO_HIP(hipMemcpyAsync(p->host, p->result, sizeof(double), hipMemcpyDeviceToHost, s));
    DZO_HIP(hipStreamSynchronize(s));
    *f = p->dtype == DZO_F32 ? (double)(float)p->host[0] : p->host[0];
    return DZO_OK;
}

int32_t dzo_problem_grad(dzo_problem_t p, void *g_dev, const void *x_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(p && x_dev && g_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(problem_grad_async(p, ctx().stream, g_dev, x_dev));
    DZO_HIP(hipStreamSynchronize(ctx().stream));
    return DZO_OK;
}

// the built-in objectives in the shape of the reference's callbacks (src/DZOptimization.jl:323-325); ctx = dzo_problem_t
double dzo_problem_objective_cb(void *problem, const void *x_dev) {
    double f = 0;
    if (dzo_problem_eval(static_cast<dzo_problem_t>(problem), x_dev, &f) != DZO_OK) return std::numeric_limits<double>::infinity();
    return f;
}
void dzo_problem_gradient_cb(void *problem, void *g_dev, const void *x_dev) {
    dzo_problem_t p = static_cast<dzo_problem_t>(problem);
    if (dzo_problem_grad(p, g_dev, x_dev) != DZO_OK && p && g_dev)
        (void)hipMemset(g_dev, 0xff, (size_t)p->n * dtype_size(p->dtype));    // NaN in both element types
}
int32_t dzo_problem_constraint_cb(void *problem, void *x_dev) {
    dzo_problem_t p = static_cast<dzo_problem_t>(problem);
    if (!p || !x_dev) return 0;
    if (!p->cons_on) return 1;
    return dzo_box_clamp(p->n, p->dtype, x_dev, p->cons_lo, p->cons_hi) == DZO_OK ? 1 : 0;
}

}  // extern "C"
