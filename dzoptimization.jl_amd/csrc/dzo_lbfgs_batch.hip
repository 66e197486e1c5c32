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
// Per pair the arithmetic is dzo_pairwise.hip's: pw_pair of dzo_pairwise.h (the self term removed by a select);
// energy and gradient of a trial come out of ONE pair loop (they share the reciprocal).  Row sums over j run j = 0 .. N-1 in T,
// rows are added in fp64 by the fixed trees of dzo_common.h, one rounding back to T; dots accumulate in fp64 in a fixed order
// that depends on N only.  No floating-point atomic.  The recursion is the chain form of :430-451.
#include "dzo_pairwise.h"

#include <cmath>
#include <new>

namespace dzo {

constexpr int kQuenchMaxN = DZO_LBFGS_BATCH_MAX_PARTICLES;
constexpr int kQuenchMaxM = DZO_LBFGS_BATCH_MAX_HISTORY;
constexpr int kQuenchPer = kQuenchMaxN / kBlock;             // particles a thread of the BLOCK shape owns at most
constexpr size_t kQuenchLdsMax = 160 * 1024 - 1024;          // dynamic LDS of a step launch: the CU's 160 KiB less room for the static part

template <typename T> struct QuenchArgs {
    int N, m, steps;
    int init;                  // eval kernels: also build the constructor's state (:381-397)
    int64_t max_halvings;
    T step_length;
    T *x, *g, *d, *dx, *dg;    // (3N, batch)
    T *f, *df;                 // batch
    int32_t *stuck, *hcount, *halv;
    int64_t *iters;
    T *S, *Y;                  // (3N, m, batch), newest first
    double *rho;               // (m, batch), newest first
    T *slab;                   // BLOCK shape without room in LDS: 2 m 3N elements per instance
};

// a lane's / thread's share of a dot over one particle, in fp64
template <typename T> __device__ __forceinline__ double q_dot3(T ax, T ay, T az, T bx, T by, T bz) {
    double p = (double)ax * (double)bx;
    p = __builtin_fma((double)ay, (double)by, p);
    return __builtin_fma((double)az, (double)bz, p);
}

// one (i, j) term: energy (:137-146) and gradient (:245-257) from the same r2 (dzo_pairwise.h); `drop` = self term or padding
template <typename T, typename F>
__device__ __forceinline__ void q_pair(bool drop, T xi, T yi, T zi, T xj, T yj, T zj, T &row, T &ax, T &ay, T &az) {
    pw_pair<T, F, kPwEnergyGradient>(drop, PwPoint<T>{xi, yi, zi}, PwPoint<T>{xj, yj, zj}, ax, ay, az, &row);
}

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
// energy in every lane, gradient of particle `lane` (zero in the lanes without a particle)
template <typename T, typename F>
__device__ __forceinline__ void q_wave_eval(int N, int lane, T x, T y, T z, T &E, T &gx, T &gy, T &gz) {
    T row = T(0), ax = T(0), ay = T(0), az = T(0);
    // four independent pairs per trip; j4 + k <= 63 is a lane of the wave, the padding is dropped like the self term
    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j4 + k;
            q_pair<T, F>(j == lane || j >= N, x, y, z, lane_read(x, j), lane_read(y, j), lane_read(z, j), row, ax, ay, az);
        }
    }
    const bool live = lane < N;
    E = (T)(0.5 * wave_sum_all(live ? (double)row : 0.0));
    gx = live ? pw_twice(ax) : T(0);
    gy = live ? pw_twice(ay) : T(0);
    gz = live ? pw_twice(az) : T(0);
}

template <typename T, typename F> __global__ __launch_bounds__(64) void quench_wave_eval_kernel(QuenchArgs<T> a) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    const bool live = lane < N;
    const T x = live ? a.x[base + lane] : T(0), y = live ? a.x[base + N + lane] : T(0), z = live ? a.x[base + 2 * N + lane] : T(0);
    T E, gx, gy, gz;
    q_wave_eval<T, F>(N, lane, x, y, z, E, gx, gy, gz);
    if (lane == 0) a.f[b] = E;
    if (a.g && live) { a.g[base + lane] = gx; a.g[base + N + lane] = gy; a.g[base + 2 * N + lane] = gz; }
    if (!a.init) return;
    const double gg = wave_sum_all(q_dot3(gx, gy, gz, gx, gy, gz));
    const bool stuck = gg == 0.0;                            // iszero(norm), :382
    const T sc = (T)(-((double)a.step_length / ::sqrt(gg))); // :387
    if (live) {
        a.d[base + lane] = stuck ? T(0) : sc * gx;
        a.d[base + N + lane] = stuck ? T(0) : sc * gy;
        a.d[base + 2 * N + lane] = stuck ? T(0) : sc * gz;
    }
    if (lane == 0) a.stuck[b] = stuck ? 1 : 0;
}

extern __shared__ __attribute__((aligned(16))) double quench_smem[];

template <typename T, typename F> __global__ __launch_bounds__(64) void quench_wave_step_kernel(QuenchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // :456, the whole wave
    const int lane = threadIdx.x, N = a.N, m = a.m;
    const int64_t base = (int64_t)3 * N * b;
    const bool live = lane < N;
    auto ld = [&](const T *p, int c) { return live ? p[base + c * N + lane] : T(0); };
    T x = ld(a.x, 0), y = ld(a.x, 1), z = ld(a.x, 2);
    T gx = ld(a.g, 0), gy = ld(a.g, 1), gz = ld(a.g, 2);
    T px = ld(a.d, 0), py = ld(a.d, 1), pz = ld(a.d, 2);
    T sx = ld(a.dx, 0), sy = ld(a.dx, 1), sz = ld(a.dx, 2);
    T yx = ld(a.dg, 0), yy = ld(a.dg, 1), yz = ld(a.dg, 2);
    T E = a.f[b], dE = a.df[b];
    int64_t it = a.iters[b];
    int hc = a.hcount[b], halv = a.halv[b], head = 0;
    // LDS: rho[m] | alpha[m] | S ring | Y ring; element (slot p, component c) of this lane at (p * 3 + c) * 64 + lane
    double *rho = quench_smem, *alpha = rho + m;
    T *hS = reinterpret_cast<T *>(alpha + m), *hY = hS + m * 3 * 64;
    const int64_t hbase = (int64_t)3 * N * m * b;
    for (int k = 0; k < hc; ++k) {
        rho[k] = a.rho[(int64_t)m * b + k];                  // every lane the same value to the same address
        for (int c = 0; c < 3; ++c) {
            hS[(k * 3 + c) * 64 + lane] = live ? a.S[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
            hY[(k * 3 + c) * 64 + lane] = live ? a.Y[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
        }
    }
    bool stuck = false;
    for (int s = 0; s < a.steps && !stuck; ++s) {
        if (it > 0) {                                        // compute_lbfgs_step_direction!, :430-451
            T qx = gx, qy = gy, qz = gz;
            for (int k = 0; k < hc; ++k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * 3 * 64 + lane, *yp = hY + p * 3 * 64 + lane;
                const T al = (T)(wave_sum_all(q_dot3(sp[0], sp[64], sp[128], qx, qy, qz)) / rho[p]);   // :440
                alpha[p] = (double)al;
                qx = dfma<T>(-al, yp[0], qx); qy = dfma<T>(-al, yp[64], qy); qz = dfma<T>(-al, yp[128], qz);   // :441
            }
            if (hc > 0) {
                const T *yp = hY + head * 3 * 64 + lane;
                const T gm = (T)(-(rho[head] / wave_sum_all(q_dot3(yp[0], yp[64], yp[128], yp[0], yp[64], yp[128]))));   // :444
                qx *= gm; qy *= gm; qz *= gm;
            }
            for (int k = hc - 1; k >= 0; --k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * 3 * 64 + lane, *yp = hY + p * 3 * 64 + lane;
                const T beta = (T)(wave_sum_all(q_dot3(yp[0], yp[64], yp[128], qx, qy, qz)) / rho[p]);   // :447
                const T cf = -((T)alpha[p] + beta);
                qx = dfma<T>(cf, sp[0], qx); qy = dfma<T>(cf, sp[64], qy); qz = dfma<T>(cf, sp[128], qz);   // :448
            }
            px = qx; py = qy; pz = qz;
        }
        // take_backtracking_step!, :107-154, from t = 1
        const T x0 = x, y0 = y, z0 = z;                      // :118
        T t = T(1);
        int h = 0;
        for (;;) {
            const T xt = dfma<T>(t, px, x0), yt = dfma<T>(t, py, y0), zt = dfma<T>(t, pz, z0);   // :124
            if (__all(is_equal(xt, x0) && is_equal(yt, y0) && is_equal(zt, z0))) { stuck = true; break; }   // :128
            T Et, tx, ty, tz;
            q_wave_eval<T, F>(N, lane, xt, yt, zt, Et, tx, ty, tz);
            if (Et < E) {                                    // :139
                dE = Et - E; E = Et;                         // :142-144
                sx = xt - x0; sy = yt - y0; sz = zt - z0;    // :145
                yx = tx - gx; yy = ty - gy; yz = tz - gz;    // :478-480
                x = xt; y = yt; z = zt;
                gx = tx; gy = ty; gz = tz;
                break;
            }
            t *= T(0.5);                                     // :152 (the point was never overwritten: :151)
            if (++h >= a.max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (stuck) { sx = x0; sy = y0; sz = z0; break; }     // delta_point keeps the copy of :118
        head = head == 0 ? m - 1 : head - 1;                 // pushfirst!, :482-496
        T *sp = hS + head * 3 * 64 + lane, *yp = hY + head * 3 * 64 + lane;
        sp[0] = sx; sp[64] = sy; sp[128] = sz;
        yp[0] = yx; yp[64] = yy; yp[128] = yz;
        rho[head] = wave_sum_all(q_dot3(sx, sy, sz, yx, yy, yz));   // :505
        if (hc < m) ++hc;
        ++it;                                                // :507
    }
    if (live) {
        auto st = [&](T *p, int c, T v) { p[base + c * N + lane] = v; };
        st(a.x, 0, x); st(a.x, 1, y); st(a.x, 2, z);
        st(a.g, 0, gx); st(a.g, 1, gy); st(a.g, 2, gz);
        st(a.d, 0, px); st(a.d, 1, py); st(a.d, 2, pz);
        st(a.dx, 0, sx); st(a.dx, 1, sy); st(a.dx, 2, sz);
        st(a.dg, 0, yx); st(a.dg, 1, yy); st(a.dg, 2, yz);
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
        a.f[b] = E; a.df[b] = dE;
        a.stuck[b] = stuck ? 1 : 0;
        a.iters[b] = it;
        a.hcount[b] = hc; a.halv[b] = halv;
    }
}

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
// a block-wide sum in EVERY thread, fixed order (wave trees, then the four waves in wave order).  `red` holds 2 * kWaves doubles
// used alternately, so that one barrier per sum is enough (a wave can be at most one sum ahead of the slowest).
__device__ __forceinline__ double q_block_sum_all(double v, double *red, int &par) {
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

// energy in every thread and the gradients of the thread's own particles, from the point X = [x | y | z] in LDS (complete and
// visible: the caller's barrier)
template <typename T, typename F>
__device__ __forceinline__ void q_block_eval(int N, int tid, const T *X, double *red, int &par, T &E, T (&gx)[kQuenchPer], T (&gy)[kQuenchPer],
                                             T (&gz)[kQuenchPer]) {
    double rows = 0;
#pragma unroll
    for (int q = 0; q < kQuenchPer; ++q) {
        const int i = tid + kBlock * q;
        gx[q] = gy[q] = gz[q] = T(0);
        if (i < N) {
            const T xi = X[i], yi = X[N + i], zi = X[2 * N + i];
            T row = T(0), ax = T(0), ay = T(0), az = T(0);
            for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j4 + k, jc = j < N ? j : N - 1;   // the padding re-reads the last particle and is dropped
                    q_pair<T, F>(j == i || j >= N, xi, yi, zi, X[jc], X[N + jc], X[2 * N + jc], row, ax, ay, az);
                }
            }
            rows += (double)row;
            gx[q] = pw_twice(ax); gy[q] = pw_twice(ay); gz[q] = pw_twice(az);
        }
    }
    E = (T)(0.5 * q_block_sum_all(rows, red, par));
}

template <typename T, typename F> __global__ __launch_bounds__(kBlock) void quench_block_eval_kernel(QuenchArgs<T> a) {
    __shared__ T X[3 * kQuenchMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    for (int e = tid; e < 3 * N; e += kBlock) X[e] = a.x[base + e];
    __syncthreads();
    int par = 0;
    T E, gx[kQuenchPer], gy[kQuenchPer], gz[kQuenchPer];
    q_block_eval<T, F>(N, tid, X, red, par, E, gx, gy, gz);
    if (tid == 0) a.f[b] = E;
    double part = 0;
#pragma unroll
    for (int q = 0; q < kQuenchPer; ++q) {
        const int i = tid + kBlock * q;
        if (i < N) {
            if (a.g) { a.g[base + i] = gx[q]; a.g[base + N + i] = gy[q]; a.g[base + 2 * N + i] = gz[q]; }
            part += q_dot3(gx[q], gy[q], gz[q], gx[q], gy[q], gz[q]);
        }
    }
    if (!a.init) return;
    const double gg = q_block_sum_all(part, red, par);
    const bool stuck = gg == 0.0;
    const T sc = (T)(-((double)a.step_length / ::sqrt(gg)));
#pragma unroll
    for (int q = 0; q < kQuenchPer; ++q) {
        const int i = tid + kBlock * q;
        if (i < N) {
            a.d[base + i] = stuck ? T(0) : sc * gx[q];
            a.d[base + N + i] = stuck ? T(0) : sc * gy[q];
            a.d[base + 2 * N + i] = stuck ? T(0) : sc * gz[q];
        }
    }
    if (tid == 0) a.stuck[b] = stuck ? 1 : 0;
}

// the body for every particle i the thread owns (thread t owns the particles t + 256 q; `tid` and `N` are the caller's): every
// element of a vector in LDS is touched by its owner only
#define DZO_Q_OWN(i, ...)                                   \
    _Pragma("unroll") for (int q = 0; q < kQuenchPer; ++q) { \
        const int i = tid + kBlock * q;                     \
        if (i < N) { __VA_ARGS__ }                          \
    }

// HL: the history ring is in LDS (else in a.slab)
template <typename T, typename F, bool HL> __global__ __launch_bounds__(kBlock) void quench_block_step_kernel(QuenchArgs<T> a) {
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
    int hc = *ghc_, halv = *ghalv_, head = 0, par = 0;
    int64_t it = *git_;
    T E = *gf_, dE = *gdf_;
    DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        X[e] = gx_[e]; G[e] = gg_[e]; D[e] = gd_[e]; DX[e] = gdx_[e]; DG[e] = gdg_[e];
        for (int k = 0; k < hc; ++k) { hS[k * n3 + e] = gS_[(int64_t)n3 * k + e]; hY[k * n3 + e] = gY_[(int64_t)n3 * k + e]; }
    })
    for (int k = 0; k < hc; ++k) rho[k] = grho_[k];   // every thread the same value to the same address
    bool stuck = false;
    for (int s = 0; s < a.steps && !stuck; ++s) {
        if (it > 0) {                                        // compute_lbfgs_step_direction!, :430-451, on D
            DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = G[c * N + i];)
            for (int k = 0; k < hc; ++k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * n3, *yp = hY + p * n3;
                double part = 0;
                DZO_Q_OWN(i, part += q_dot3(sp[i], sp[N + i], sp[2 * N + i], D[i], D[N + i], D[2 * N + i]);)
                const T al = (T)(q_block_sum_all(part, red, par) / rho[p]);
                alpha[p] = (double)al;
                DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = dfma<T>(-al, yp[c * N + i], D[c * N + i]);)
            }
            if (hc > 0) {
                const T *yp = hY + head * n3;
                double part = 0;
                DZO_Q_OWN(i, part += q_dot3(yp[i], yp[N + i], yp[2 * N + i], yp[i], yp[N + i], yp[2 * N + i]);)
                const T gm = (T)(-(rho[head] / q_block_sum_all(part, red, par)));
                DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] *= gm;)
            }
            for (int k = hc - 1; k >= 0; --k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * n3, *yp = hY + p * n3;
                double part = 0;
                DZO_Q_OWN(i, part += q_dot3(yp[i], yp[N + i], yp[2 * N + i], D[i], D[N + i], D[2 * N + i]);)
                const T beta = (T)(q_block_sum_all(part, red, par) / rho[p]);
                const T cf = -((T)alpha[p] + beta);
                DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = dfma<T>(cf, sp[c * N + i], D[c * N + i]);)
            }
        }
        // take_backtracking_step!, :107-154: DX keeps the old point (:118), X is the trial (:124)
        DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) DX[c * N + i] = X[c * N + i];)
        T t = T(1);
        int h = 0;
        bool accepted = false;
        T tx[kQuenchPer], ty[kQuenchPer], tz[kQuenchPer];
        for (;;) {
            bool same = true;
            DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
                const T v = dfma<T>(t, D[c * N + i], DX[c * N + i]);
                X[c * N + i] = v;
                same = same && is_equal(v, DX[c * N + i]);
            })
            if (__syncthreads_and(same ? 1 : 0)) { stuck = true; break; }   // :128; the barrier also publishes the trial point
            T Et;
            q_block_eval<T, F>(N, tid, X, red, par, Et, tx, ty, tz);       // its barrier: every thread has read X
            if (Et < E) { dE = Et - E; E = Et; accepted = true; break; }   // :139-144
            t *= T(0.5);                                                    // :152
            if (++h >= a.max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (!accepted) {                                     // :151 / the copy of :118 stays in DX
            DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) X[c * N + i] = DX[c * N + i];)
            break;
        }
        head = head == 0 ? m - 1 : head - 1;                 // pushfirst!, :482-496
        T *sp = hS + head * n3, *yp = hY + head * n3;
        double part = 0;
#pragma unroll
        for (int q = 0; q < kQuenchPer; ++q) {
            const int i = tid + kBlock * q;
            if (i < N) {
                const T tg[3] = {tx[q], ty[q], tz[q]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int e = c * N + i;
                    const T dxv = X[e] - DX[e], dgv = tg[c] - G[e];   // :145, :478-480
                    DX[e] = dxv; DG[e] = dgv; G[e] = tg[c];
                    sp[e] = dxv; yp[e] = dgv;
                }
                part += q_dot3(DX[i], DX[N + i], DX[2 * N + i], DG[i], DG[N + i], DG[2 * N + i]);
            }
        }
        rho[head] = q_block_sum_all(part, red, par);         // :505
        if (hc < m) ++hc;
        ++it;
    }
    DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        gx_[e] = X[e]; gg_[e] = G[e]; gd_[e] = D[e]; gdx_[e] = DX[e]; gdg_[e] = DG[e];
    })
    DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        for (int k = 0; k < hc; ++k) {
            const int p = head + k < m ? head + k : head + k - m;
            gS_[(int64_t)n3 * k + e] = hS[p * n3 + e];
            gY_[(int64_t)n3 * k + e] = hY[p * n3 + e];
        }
    })
    if (tid < hc) grho_[tid] = rho[head + tid < m ? head + tid : head + tid - m];
    if (tid == 0) {
        *gf_ = E; *gdf_ = dE;
        *gstuck_ = stuck ? 1 : 0;
        *git_ = it;
        *ghc_ = hc; *ghalv_ = halv;
    }
}

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

struct dzo_lbfgs_batch_s {
    int device = -1;
    int32_t dtype = DZO_F64;
    int N = 0, m = 0;
    int64_t B = 0, max_halvings = 4096;
    void *x = nullptr;               // the caller's
    void *g = nullptr, *d = nullptr, *dx = nullptr, *dg = nullptr, *f = nullptr, *df = nullptr, *S = nullptr, *Y = nullptr, *slab = nullptr;
    int32_t *stuck = nullptr, *hcount = nullptr, *halv = nullptr;
    int64_t *iters = nullptr, *active_dev = nullptr, *active_host = nullptr;
    double *rho = nullptr;
    size_t lds_bytes = 0;
    bool hist_lds = true;
};

namespace dzo {

static void qb_free(dzo_lbfgs_batch_s *h) {
    void *p[] = {h->g, h->d, h->dx, h->dg, h->f, h->df, h->S, h->Y, h->slab, h->stuck, h->hcount, h->halv, h->iters, h->active_dev, h->rho};
    for (void *q : p)
        if (q) (void)hipFree(q);
    if (h->active_host) (void)hipHostFree(h->active_host);
    delete h;
}

static int32_t qb_alloc(void **p, size_t bytes) { return device_alloc(p, bytes, "the batched L-BFGS state", true); }

static int32_t qb_check_common(int32_t radial, int64_t N, int64_t batch, int32_t dtype) {
    return pw_check_args(radial, dtype, N, batch, "batch", kQuenchMaxN, DZO_ERR_UNSUPPORTED, "the batched kernels hold an instance in one block");
}

template <typename T> static QuenchArgs<T> qb_args(const dzo_lbfgs_batch_s *h, int steps, int init, double step_length) {
    QuenchArgs<T> a;
    a.N = h->N; a.m = h->m; a.steps = steps; a.init = init;
    a.max_halvings = h->max_halvings;
    a.step_length = (T)step_length;
    a.x = (T *)h->x; a.g = (T *)h->g; a.d = (T *)h->d; a.dx = (T *)h->dx; a.dg = (T *)h->dg;
    a.f = (T *)h->f; a.df = (T *)h->df;
    a.stuck = h->stuck; a.hcount = h->hcount; a.halv = h->halv; a.iters = h->iters;
    a.S = (T *)h->S; a.Y = (T *)h->Y; a.rho = h->rho; a.slab = (T *)h->slab;
    return a;
}

template <typename T> static void qb_launch_eval(hipStream_t s, int64_t batch, const QuenchArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((quench_wave_eval_kernel<T, LJRadial<T>>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((quench_block_eval_kernel<T, LJRadial<T>>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

template <typename T> static const void *qb_step_kernel(const dzo_lbfgs_batch_s *h) {
    if (h->N <= 64) return (const void *)quench_wave_step_kernel<T, LJRadial<T>>;
    return h->hist_lds ? (const void *)quench_block_step_kernel<T, LJRadial<T>, true> : (const void *)quench_block_step_kernel<T, LJRadial<T>, false>;
}

template <typename T> static void qb_launch_step(hipStream_t s, const dzo_lbfgs_batch_s *h, int steps) {
    const QuenchArgs<T> a = qb_args<T>(h, steps, 0, 0.0);
    const dim3 grid((unsigned)h->B);
    if (h->N <= 64) hipLaunchKernelGGL((quench_wave_step_kernel<T, LJRadial<T>>), grid, dim3(64), h->lds_bytes, s, a);
    else if (h->hist_lds) hipLaunchKernelGGL((quench_block_step_kernel<T, LJRadial<T>, true>), grid, dim3(kBlock), h->lds_bytes, s, a);
    else hipLaunchKernelGGL((quench_block_step_kernel<T, LJRadial<T>, false>), grid, dim3(kBlock), h->lds_bytes, s, a);
}

// H: either batched handle (B, stuck, active_dev, active_host)
template <typename H> static int32_t qb_count(H *h, hipStream_t s, int64_t *active) {
    hipLaunchKernelGGL(quench_count_active_kernel, dim3(1), dim3(kBlock), 0, s, h->B, (const int32_t *)h->stuck, h->active_dev);
    DZO_HIP(hipGetLastError());
    DZO_HIP(hipMemcpyAsync(h->active_host, h->active_dev, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DZO_HIP(hipStreamSynchronize(s));
    *active = h->active_host[0];
    return DZO_OK;
}

// `what` -> device address, bytes
static int32_t qb_array(dzo_lbfgs_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const size_t es = dtype_size(h->dtype), B = (size_t)h->B, n3 = 3 * (size_t)h->N, m = (size_t)h->m;
    switch (what) {
    case DZO_LBFGS_BATCH_POINTS: *p = h->x; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_GRADIENTS: *p = h->g; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DIRECTIONS: *p = h->d; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DELTA_POINTS: *p = h->dx; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DELTA_GRADIENTS: *p = h->dg; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_OBJECTIVES: *p = h->f; *bytes = es * B; break;
    case DZO_LBFGS_BATCH_DELTA_OBJECTIVES: *p = h->df; *bytes = es * B; break;
    case DZO_LBFGS_BATCH_IS_STUCK: *p = h->stuck; *bytes = 4 * B; break;
    case DZO_LBFGS_BATCH_ITERATION_COUNTS: *p = h->iters; *bytes = 8 * B; break;
    case DZO_LBFGS_BATCH_HISTORY_COUNTS: *p = h->hcount; *bytes = 4 * B; break;
    case DZO_LBFGS_BATCH_S: *p = h->S; *bytes = es * n3 * m * B; break;
    case DZO_LBFGS_BATCH_Y: *p = h->Y; *bytes = es * n3 * m * B; break;
    case DZO_LBFGS_BATCH_RHO: *p = h->rho; *bytes = 8 * m * B; break;
    case DZO_LBFGS_BATCH_LAST_HALVINGS: *p = h->halv; *bytes = 4 * B; break;
    default: set_error("unknown batched L-BFGS array %d", what); return DZO_ERR_INVALID;
    }
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
    DZO_TRY(qb_check_common(radial, n_particles, batch, dtype));
    DZO_REQUIRE(history_length >= 1, DZO_ERR_INVALID, "history_length must be at least 1 (got %d)", history_length);
    DZO_REQUIRE(history_length <= kQuenchMaxM, DZO_ERR_UNSUPPORTED, "history_length = %d: the batched kernels keep up to %d pairs", history_length,
                kQuenchMaxM);
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:380)");
    DZO_TRY(require_same_backend("LBFGSOptimizer", "src/DZOptimization.jl:363-364", points_dev, "initial_point", nullptr, ""));
    Context &c = ctx();
    dzo_lbfgs_batch_s *h = new (std::nothrow) dzo_lbfgs_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    h->device = c.device; h->dtype = dtype; h->N = (int)n_particles; h->m = history_length; h->B = batch; h->x = points_dev;
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles, m = (size_t)history_length;
    const size_t small = 16 * m;                              // rho | alpha
    if (n_particles <= 64) {
        h->lds_bytes = small + 2 * m * 3 * 64 * es;
    } else {
        const size_t vectors = small + 16 * kWaves + 5 * n3 * es;
        h->hist_lds = vectors + 2 * m * n3 * es <= kQuenchLdsMax;
        h->lds_bytes = h->hist_lds ? vectors + 2 * m * n3 * es : vectors;
    }
    int32_t rc = DZO_OK;
    if ((rc = qb_alloc(&h->g, es * n3 * B)) || (rc = qb_alloc(&h->d, es * n3 * B)) || (rc = qb_alloc(&h->dx, es * n3 * B)) ||
        (rc = qb_alloc(&h->dg, es * n3 * B)) || (rc = qb_alloc(&h->f, es * B)) || (rc = qb_alloc(&h->df, es * B)) ||
        (rc = qb_alloc(&h->S, es * n3 * m * B)) || (rc = qb_alloc(&h->Y, es * n3 * m * B)) ||
        (!h->hist_lds && (rc = qb_alloc(&h->slab, 2 * es * n3 * m * B))) || (rc = qb_alloc((void **)&h->stuck, 4 * B)) ||
        (rc = qb_alloc((void **)&h->hcount, 4 * B)) || (rc = qb_alloc((void **)&h->halv, 4 * B)) || (rc = qb_alloc((void **)&h->iters, 8 * B)) ||
        (rc = qb_alloc((void **)&h->active_dev, 8)) || (rc = qb_alloc((void **)&h->rho, 8 * m * B))) {
        qb_free(h);
        return rc;
    }
    hipError_t e = hipHostMalloc((void **)&h->active_host, sizeof(int64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipDeviceSynchronize();          // the memsets above ran on the null stream
    if (e == hipSuccess && h->lds_bytes > 48 * 1024) {
        // gfx950 has 160 KiB of LDS per CU; dynamic requests above the default need the attribute.  It belongs to the kernel, not
        // to the handle: it is raised to the limit, so that a later handle with a smaller request does not lower it for this one
        const void *k = dtype == DZO_F64 ? qb_step_kernel<double>(h) : qb_step_kernel<float>(h);
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQuenchLdsMax);
    }
    if (e != hipSuccess) { qb_free(h); return hip_fail(e, "batched L-BFGS state", __FILE__, __LINE__); }
    {
        DZO_TIMED("lbfgs_batch_init", c.stream);
        DZO_DISPATCH(dtype, qb_launch_eval<T>(c.stream, batch, qb_args<T>(h, 0, 1, initial_step_length)));
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { qb_free(h); return hip_fail(e, "batched L-BFGS constructor", __FILE__, __LINE__); }
    *out = h;
    return DZO_OK;
}

int32_t dzo_lbfgs_batch_destroy(dzo_lbfgs_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->device);
    (void)hipStreamSynchronize(ctx().stream);
    qb_free(h);
    return DZO_OK;
}

// the project's bounded-halvings escape of the loop of :121-153 (dzo_lbfgs_set_max_halvings); at least 1 here
int32_t dzo_lbfgs_batch_set_max_halvings(dzo_lbfgs_batch_t h, int64_t max_halvings) {
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(max_halvings >= 1, DZO_ERR_INVALID, "max_halvings must be at least 1 (got %lld): a launch cannot search without bound", (long long)max_halvings);
    h->max_halvings = max_halvings;
    return DZO_OK;
}

// step!(::LBFGSOptimizer), src/DZOptimization.jl:454-509, `steps` times per instance
int32_t dzo_lbfgs_batch_step(dzo_lbfgs_batch_t h, int32_t steps, int32_t *all_stuck) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(steps >= 0, DZO_ERR_INVALID, "steps must not be negative (got %d)", steps);
    DeviceScope scope(h->device);
    hipStream_t s = ctx().stream;
    if (steps > 0) {
        DZO_TIMED("lbfgs_batch_step", s);
        DZO_DISPATCH(h->dtype, qb_launch_step<T>(s, h, steps));
        DZO_HIP(hipGetLastError());
    }
    if (all_stuck) {
        int64_t active = 0;
        DZO_TRY(qb_count(h, s, &active));
        *all_stuck = active == 0 ? 1 : 0;
    }
    return DZO_OK;
}

int32_t dzo_lbfgs_batch_count_active(dzo_lbfgs_batch_t h, int64_t *active) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && active, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    return qb_count(h, ctx().stream, active);
}

int32_t dzo_lbfgs_batch_get_ptr(dzo_lbfgs_batch_t h, int32_t what, void **ptr_dev) {
    DZO_REQUIRE(h && ptr_dev, DZO_ERR_INVALID, "null argument");
    size_t bytes = 0;
    return qb_array(h, what, ptr_dev, &bytes);
}

int32_t dzo_lbfgs_batch_read(dzo_lbfgs_batch_t h, int32_t what, void *out_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && out_host, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(qb_array(h, what, &p, &bytes));
    return copy_blocking(out_host, p, bytes, hipMemcpyDeviceToHost);
}

// objective_function and gradient_function! of every instance (:416-421), by the optimizer's own device routine
int32_t dzo_pairwise_batch_energy_gradient(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                           void *energies_dev, void *gradients_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && energies_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(qb_check_common(radial, n_particles, batch, dtype));
    const char *where = "LBFGSOptimizer", *cite = "src/DZOptimization.jl:410-420";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", energies_dev, "energies"));
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", gradients_dev, "gradients"));
    Context &c = ctx();
    dzo_lbfgs_batch_s tmp;
    tmp.N = (int)n_particles; tmp.m = 1; tmp.B = batch;
    tmp.x = const_cast<void *>(points_dev); tmp.f = energies_dev; tmp.g = gradients_dev;
    {
        DZO_TIMED("pairwise_batch_energy_gradient", c.stream);
        DZO_DISPATCH(dtype, qb_launch_eval<T>(c.stream, batch, qb_args<T>(&tmp, 0, 0, 0.0)));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

}  // extern "C"

// ================================================================================================================
// Batched AdGDOptimizer (src/DZOptimization.jl:179-312, constraint_function! = nothing) over the same clusters: dzo_adgd_batch_*.
//
// The second live optimizer on the launch shapes above.  It keeps no history, so an instance is four vectors (point, gradient,
// delta_point, delta_gradient), two step sizes and a few scalars.  The trial's energy and gradient come from q_wave_eval /
// q_block_eval, the block sums from q_block_sum_all, the sums of squares from q_dot3: one definition with the quench, the same
// bits.  The step-size rule (:285-299) is evaluated in T, operation by operation as adgd_next_state of dzo_adgd.hip does.
//
//   * WAVE (N <= 64): point, gradient, both deltas, the trial and its gradient are registers; no LDS beyond the sums'.
//   * BLOCK (65 <= N <= 1024): dynamic LDS red[2 kWaves] | X | G | DX | DG | XT (the trial point, which the pair loop reads as
//     a broadcast); the trial gradient in registers.  5 * 3N elements: 120 KiB at N = 1024 in fp64.
// ================================================================================================================
namespace dzo {

constexpr int kAdgdBatchMaxN = DZO_ADGD_BATCH_MAX_PARTICLES;
static_assert(kAdgdBatchMaxN == kQuenchMaxN, "the batched AdGD kernels use the quench's evaluation routines and their particle bound");

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
        part += q_dot3(gx, gy, gz, gx, gy, gz);
    }
    int par = 0;
    const double ss = q_block_sum_all(part, red, par);       // :230
    if (tid == 0) {
        const bool stuck = ss == 0.0;                        // :231
        const T s0 = stuck ? T(0) : a.step_length / (T)::sqrt(ss);   // :232-233
        a.cur[b] = s0; a.prev[b] = s0;                       // :241
        a.stuck[b] = stuck ? 1 : 0;
    }
}

template <typename T, typename F> __global__ __launch_bounds__(64) void adgd_batch_wave_step_kernel(AdgdBatchArgs<T> a) {
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
            const double dg2 = wave_sum_all(q_dot3(yx, yy, yz, yx, yy, yz));
            const double dx2 = wave_sum_all(q_dot3(sx, sy, sz, sx, sy, sz));
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
            q_wave_eval<T, F>(N, lane, xt, yt, zt, Et, tx, ty, tz);
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

template <typename T, typename F> __global__ __launch_bounds__(kBlock) void adgd_batch_block_step_kernel(AdgdBatchArgs<T> a) {
    const int64_t b = blockIdx.x;
    if (a.stuck[b]) return;                                  // the whole block
    const int tid = threadIdx.x, N = a.N, n3 = 3 * N;
    const int64_t base = (int64_t)n3 * b;
    // LDS: red[2 kWaves] | X | G | DX | DG | XT
    double *red = quench_smem;
    T *X = reinterpret_cast<T *>(red + 2 * kWaves), *G = X + n3, *DX = G + n3, *DG = DX + n3, *XT = DG + n3;
    T *const gx_ = pw_pin_ptr(a.x + base), *const gg_ = pw_pin_ptr(a.g + base), *const gdx_ = pw_pin_ptr(a.dx + base);
    T *const gdg_ = pw_pin_ptr(a.dg + base), *const gf_ = pw_pin_ptr(a.f + b), *const gdf_ = pw_pin_ptr(a.df + b);
    T *const gcur_ = pw_pin_ptr(a.cur + b), *const gprev_ = pw_pin_ptr(a.prev + b);
    int32_t *const gstuck_ = pw_pin_ptr(a.stuck + b), *const ghalv_ = pw_pin_ptr(a.halv + b);
    int64_t *const git_ = pw_pin_ptr(a.iters + b);
    int halv = *ghalv_, par = 0;
    int64_t it = *git_;
    T E = *gf_, dE = *gdf_, cur = *gcur_, prev = *gprev_;
    DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        X[e] = gx_[e]; G[e] = gg_[e]; DX[e] = gdx_[e]; DG[e] = gdg_[e];
    })
    bool stuck = false;
    for (int s = 0; s < a.steps && !stuck; ++s) {
        T next = cur;                                        // :287
        if (it > 0) {                                        // :288
            double pg = 0, px = 0;
            DZO_Q_OWN(i, pg += q_dot3(DG[i], DG[N + i], DG[2 * N + i], DG[i], DG[N + i], DG[2 * N + i]);
                      px += q_dot3(DX[i], DX[N + i], DX[2 * N + i], DX[i], DX[N + i], DX[2 * N + i]);)
            const double dg2 = q_block_sum_all(pg, red, par);
            const double dx2 = q_block_sum_all(px, red, par);
            next = ab_next_step_size<T>(cur, prev, dx2, dg2);
        }
        prev = cur; cur = next;                              // :298-299
        // take_backtracking_step!(opt, -next, current_gradient), :107-154: X keeps the old point, XT is the trial (:124)
        T t = next;
        int h = 0;
        bool accepted = false;
        T tx[kQuenchPer], ty[kQuenchPer], tz[kQuenchPer];
        for (;;) {
            bool same = true;
            DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
                const T v = dfma<T>(-t, G[c * N + i], X[c * N + i]);
                XT[c * N + i] = v;
                same = same && is_equal(v, X[c * N + i]);
            })
            if (__syncthreads_and(same ? 1 : 0)) { stuck = true; break; }   // :128; the barrier also publishes the trial point
            T Et;
            q_block_eval<T, F>(N, tid, XT, red, par, Et, tx, ty, tz);      // its barrier: every thread has read XT
            if (Et < E) { dE = Et - E; E = Et; accepted = true; break; }   // :139-144
            t *= T(0.5);                                                    // :152
            if (++h >= a.max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (!accepted) {                                     // delta_point keeps the copy of :118
            DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) DX[c * N + i] = X[c * N + i];)
            break;
        }
#pragma unroll
        for (int q = 0; q < kQuenchPer; ++q) {
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
    DZO_Q_OWN(i, for (int c = 0; c < 3; ++c) {
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

}  // namespace dzo

#undef DZO_Q_OWN

struct dzo_adgd_batch_s {
    int device = -1;
    int32_t dtype = DZO_F64;
    int N = 0;
    int64_t B = 0, max_halvings = 4096;
    void *x = nullptr;               // the caller's
    void *g = nullptr, *dx = nullptr, *dg = nullptr, *f = nullptr, *df = nullptr, *cur = nullptr, *prev = nullptr;
    int32_t *stuck = nullptr, *halv = nullptr;
    int64_t *iters = nullptr, *active_dev = nullptr, *active_host = nullptr;
    size_t lds_bytes = 0;            // BLOCK shape
};

namespace dzo {

static void ab_free(dzo_adgd_batch_s *h) {
    void *p[] = {h->g, h->dx, h->dg, h->f, h->df, h->cur, h->prev, h->stuck, h->halv, h->iters, h->active_dev};
    for (void *q : p)
        if (q) (void)hipFree(q);
    if (h->active_host) (void)hipHostFree(h->active_host);
    delete h;
}

static int32_t ab_alloc(void **p, size_t bytes) { return device_alloc(p, bytes, "the batched AdGD state", true); }

template <typename T> static AdgdBatchArgs<T> ab_args(const dzo_adgd_batch_s *h, int steps, double step_length) {
    AdgdBatchArgs<T> a;
    a.N = h->N; a.steps = steps;
    a.max_halvings = h->max_halvings;
    a.step_length = (T)step_length;
    a.x = (T *)h->x; a.g = (T *)h->g; a.dx = (T *)h->dx; a.dg = (T *)h->dg;
    a.f = (T *)h->f; a.df = (T *)h->df; a.cur = (T *)h->cur; a.prev = (T *)h->prev;
    a.stuck = h->stuck; a.halv = h->halv; a.iters = h->iters;
    return a;
}

// f0 and g0 by the evaluation kernels of dzo_pairwise_batch_energy_gradient, then the step sizes and is_stuck
template <typename T> static void ab_launch_init(hipStream_t s, const dzo_adgd_batch_s *h, double step_length) {
    dzo_lbfgs_batch_s tmp;
    tmp.N = h->N; tmp.m = 1; tmp.B = h->B;
    tmp.x = h->x; tmp.f = h->f; tmp.g = h->g;
    qb_launch_eval<T>(s, h->B, qb_args<T>(&tmp, 0, 0, 0.0));
    hipLaunchKernelGGL((adgd_batch_init_kernel<T>), dim3((unsigned)h->B), dim3(kBlock), 0, s, ab_args<T>(h, 0, step_length));
}

template <typename T> static void ab_launch_step(hipStream_t s, const dzo_adgd_batch_s *h, int steps) {
    const AdgdBatchArgs<T> a = ab_args<T>(h, steps, 0.0);
    const dim3 grid((unsigned)h->B);
    if (h->N <= 64) hipLaunchKernelGGL((adgd_batch_wave_step_kernel<T, LJRadial<T>>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((adgd_batch_block_step_kernel<T, LJRadial<T>>), grid, dim3(kBlock), h->lds_bytes, s, a);
}

// `what` -> device address, bytes
static int32_t ab_array(dzo_adgd_batch_s *h, int32_t what, void **p, size_t *bytes) {
    const size_t es = dtype_size(h->dtype), B = (size_t)h->B, n3 = 3 * (size_t)h->N;
    switch (what) {
    case DZO_ADGD_BATCH_POINTS: *p = h->x; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_GRADIENTS: *p = h->g; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_DELTA_POINTS: *p = h->dx; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_DELTA_GRADIENTS: *p = h->dg; *bytes = es * n3 * B; break;
    case DZO_ADGD_BATCH_OBJECTIVES: *p = h->f; *bytes = es * B; break;
    case DZO_ADGD_BATCH_DELTA_OBJECTIVES: *p = h->df; *bytes = es * B; break;
    case DZO_ADGD_BATCH_IS_STUCK: *p = h->stuck; *bytes = 4 * B; break;
    case DZO_ADGD_BATCH_ITERATION_COUNTS: *p = h->iters; *bytes = 8 * B; break;
    case DZO_ADGD_BATCH_CURRENT_STEP_SIZES: *p = h->cur; *bytes = es * B; break;
    case DZO_ADGD_BATCH_PREVIOUS_STEP_SIZES: *p = h->prev; *bytes = es * B; break;
    case DZO_ADGD_BATCH_LAST_HALVINGS: *p = h->halv; *bytes = 4 * B; break;
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
    DZO_TRY(qb_check_common(radial, n_particles, batch, dtype));
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:229)");
    DZO_TRY(require_same_backend("AdGDOptimizer", "src/DZOptimization.jl:216-217", points_dev, "initial_point", nullptr, ""));
    Context &c = ctx();
    dzo_adgd_batch_s *h = new (std::nothrow) dzo_adgd_batch_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    h->device = c.device; h->dtype = dtype; h->N = (int)n_particles; h->B = batch; h->x = points_dev;
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles;
    if (n_particles > 64) h->lds_bytes = 16 * kWaves + 5 * n3 * es;
    int32_t rc = DZO_OK;
    if ((rc = ab_alloc(&h->g, es * n3 * B)) || (rc = ab_alloc(&h->dx, es * n3 * B)) || (rc = ab_alloc(&h->dg, es * n3 * B)) ||
        (rc = ab_alloc(&h->f, es * B)) || (rc = ab_alloc(&h->df, es * B)) || (rc = ab_alloc(&h->cur, es * B)) || (rc = ab_alloc(&h->prev, es * B)) ||
        (rc = ab_alloc((void **)&h->stuck, 4 * B)) || (rc = ab_alloc((void **)&h->halv, 4 * B)) || (rc = ab_alloc((void **)&h->iters, 8 * B)) ||
        (rc = ab_alloc((void **)&h->active_dev, 8))) {
        ab_free(h);
        return rc;
    }
    hipError_t e = hipHostMalloc((void **)&h->active_host, sizeof(int64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipDeviceSynchronize();          // the memsets above ran on the null stream
    if (e == hipSuccess && h->lds_bytes > 48 * 1024) {
        // as in dzo_lbfgs_batch_create: the attribute belongs to the kernel, so it is raised to the limit once and for all handles
        const void *k = dtype == DZO_F64 ? (const void *)adgd_batch_block_step_kernel<double, LJRadial<double>>
                                         : (const void *)adgd_batch_block_step_kernel<float, LJRadial<float>>;
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kQuenchLdsMax);
    }
    if (e != hipSuccess) { ab_free(h); return hip_fail(e, "batched AdGD state", __FILE__, __LINE__); }
    {
        DZO_TIMED("adgd_batch_init", c.stream);
        DZO_DISPATCH(dtype, ab_launch_init<T>(c.stream, h, initial_step_length));
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { ab_free(h); return hip_fail(e, "batched AdGD constructor", __FILE__, __LINE__); }
    *out = h;
    return DZO_OK;
}

int32_t dzo_adgd_batch_destroy(dzo_adgd_batch_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->device);
    (void)hipStreamSynchronize(ctx().stream);
    ab_free(h);
    return DZO_OK;
}

// the project's bounded-halvings escape of the loop of :121-153 (dzo_lbfgs_set_max_halvings); at least 1 here
int32_t dzo_adgd_batch_set_max_halvings(dzo_adgd_batch_t h, int64_t max_halvings) {
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(max_halvings >= 1, DZO_ERR_INVALID, "max_halvings must be at least 1 (got %lld): a launch cannot search without bound", (long long)max_halvings);
    h->max_halvings = max_halvings;
    return DZO_OK;
}

// step!(::AdGDOptimizer), src/DZOptimization.jl:274-312, `steps` times per instance
int32_t dzo_adgd_batch_step(dzo_adgd_batch_t h, int32_t steps, int32_t *all_stuck) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(steps >= 0, DZO_ERR_INVALID, "steps must not be negative (got %d)", steps);
    DeviceScope scope(h->device);
    hipStream_t s = ctx().stream;
    if (steps > 0) {
        DZO_TIMED("adgd_batch_step", s);
        DZO_DISPATCH(h->dtype, ab_launch_step<T>(s, h, steps));
        DZO_HIP(hipGetLastError());
    }
    if (all_stuck) {
        int64_t active = 0;
        DZO_TRY(qb_count(h, s, &active));
        *all_stuck = active == 0 ? 1 : 0;
    }
    return DZO_OK;
}

int32_t dzo_adgd_batch_count_active(dzo_adgd_batch_t h, int64_t *active) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && active, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    return qb_count(h, ctx().stream, active);
}

int32_t dzo_adgd_batch_get_ptr(dzo_adgd_batch_t h, int32_t what, void **ptr_dev) {
    DZO_REQUIRE(h && ptr_dev, DZO_ERR_INVALID, "null argument");
    size_t bytes = 0;
    return ab_array(h, what, ptr_dev, &bytes);
}

int32_t dzo_adgd_batch_read(dzo_adgd_batch_t h, int32_t what, void *out_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && out_host, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(ab_array(h, what, &p, &bytes));
    return copy_blocking(out_host, p, bytes, hipMemcpyDeviceToHost);
}

}  // extern "C"
