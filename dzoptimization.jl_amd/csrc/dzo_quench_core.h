// dzo_quench_core.h -- the batched L-BFGS quench of ONE Lennard-Jones cluster as device functions: the constructor's first
// direction (src/DZOptimization.jl:381-387) and `steps` calls of step!() (:454-509) in the two launch shapes described in
// dzo_lbfgs_batch.hip.  The step kernels of dzo_lbfgs_batch.hip are load -> run -> store around these functions; the kernels of
// dzo_basin_hopping.hip call them once per hop on state that never leaves the CU.  One definition each, the same bits in both.
// Every name here starts with qc_ (functions) or Qc (types).  No kernel and no LDS declaration here: the caller places the state.
#pragma once
#include "dzo_cluster.h"

#include <cmath>

namespace dzo {

// ------------------------------------------------------------------------------ constraint policies
// constraint_function! of take_backtracking_step! (:133-135) as the last template argument of qc_wave_run / qc_block_run: two
// per-particle operations, both local to the lane or thread that owns the particle.  Inside a trial, as :124-139: form the trial
// by the fma, run the stuck test on the UNPROJECTED trial, project, evaluate, make the trial's gradient tangent, compare energies.
// On acceptance delta_point is projected-new minus old and delta_gradient the difference of tangent gradients.
// QcFree: constraint_function! = nothing; the two run functions compile to the code they had without the parameter.
struct QcFree {
    static constexpr bool kConstrained = false;
    template <typename T> static __device__ __forceinline__ void project(bool, T &, T &, T &) {}
    template <typename T> static __device__ __forceinline__ void tangent(T, T, T, T &, T &, T &) {}
};
// QcUnitSphere: every particle on the unit sphere.  project is p / |p| with r = sqrt(pw_r2(x, y, z)) and three IEEE divisions;
// it always reports success (a particle on the origin becomes NaN, the objective NaN, `Et < E` false: the step backtracks).
// A particle that is not `live` (the padding lanes of the WAVE shape, which hold zeros that lane_read feeds to dropped pairs) is
// left alone by a select, never by a branch around the divisions.  tangent is constrain_riesz_gradient_sphere!
// (legacy/ExampleFunctions.jl:361-374), operation for operation: overlap = x gx + y gy + z gz summed in that order, unfused;
// g -= overlap p, unfused.
struct QcUnitSphere {
    static constexpr bool kConstrained = true;
    template <typename T> static __device__ __forceinline__ void project(bool live, T &x, T &y, T &z) {
        const T r = pw_sqrt<T>(pw_r2(x, y, z));
        const T px = pw_pin(x / r), py = pw_pin(y / r), pz = pw_pin(z / r);
        x = live ? px : x;
        y = live ? py : y;
        z = live ? pz : z;
    }
    template <typename T> static __device__ __forceinline__ void tangent(T x, T y, T z, T &gx, T &gy, T &gz) {
        const T overlap = x * gx + y * gy + z * gz;
        gx = gx - overlap * x;
        gy = gy - overlap * y;
        gz = gz - overlap * z;
    }
};

// ------------------------------------------------------------------------------ WAVE shape: lane i holds particle i
// the optimizer's state of one instance: point, gradient, step_direction, delta_point, delta_gradient, the two objective values
// and the counters.  The (s, y) ring is in LDS: rho[m] | alpha[m] as doubles, element (slot p, component c) of a lane at
// (p * 3 + c) * 64 + lane of hS / hY; slot `head` is the newest pair.
template <typename T> struct QcWave {
    T x, y, z, gx, gy, gz, px, py, pz, sx, sy, sz, yx, yy, yz;
    T E, dE;
    int64_t it;
    int hc, halv, head;
};

// -initial_step_length g / |g| and is_stuck = iszero(|g0|), :381-387; returns is_stuck
template <typename T> __device__ __forceinline__ bool qc_wave_first_direction(T step_length, T gx, T gy, T gz, T &px, T &py, T &pz) {
    const double gg = wave_sum_all(cl_dot3(gx, gy, gz, gx, gy, gz));
    const bool stuck = gg == 0.0;                            // iszero(norm), :382
    const T sc = (T)(-((double)step_length / ::sqrt(gg)));   // :387
    px = stuck ? T(0) : sc * gx;
    py = stuck ? T(0) : sc * gy;
    pz = stuck ? T(0) : sc * gz;
    return stuck;
}

// up to `steps` calls of step!() of an instance that is not stuck; returns is_stuck
template <typename T, typename F, typename C = QcFree>
__device__ __forceinline__ bool qc_wave_run(int N, int m, int lane, int steps, int64_t max_halvings, QcWave<T> &w, double *rho, double *alpha,
                                            T *hS, T *hY) {
    T x = w.x, y = w.y, z = w.z, gx = w.gx, gy = w.gy, gz = w.gz, px = w.px, py = w.py, pz = w.pz;
    T sx = w.sx, sy = w.sy, sz = w.sz, yx = w.yx, yy = w.yy, yz = w.yz;
    T E = w.E, dE = w.dE;
    int64_t it = w.it;
    int hc = w.hc, halv = w.halv, head = w.head;
    bool stuck = false;
    for (int s = 0; s < steps && !stuck; ++s) {
        if (it > 0) {                                        // compute_lbfgs_step_direction!, :430-451
            T qx = gx, qy = gy, qz = gz;
            for (int k = 0; k < hc; ++k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * 3 * 64 + lane, *yp = hY + p * 3 * 64 + lane;
                const T al = (T)(wave_sum_all(cl_dot3(sp[0], sp[64], sp[128], qx, qy, qz)) / rho[p]);   // :440
                alpha[p] = (double)al;
                qx = dfma<T>(-al, yp[0], qx); qy = dfma<T>(-al, yp[64], qy); qz = dfma<T>(-al, yp[128], qz);   // :441
            }
            if (hc > 0) {
                const T *yp = hY + head * 3 * 64 + lane;
                const T gm = (T)(-(rho[head] / wave_sum_all(cl_dot3(yp[0], yp[64], yp[128], yp[0], yp[64], yp[128]))));   // :444
                qx *= gm; qy *= gm; qz *= gm;
            }
            for (int k = hc - 1; k >= 0; --k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * 3 * 64 + lane, *yp = hY + p * 3 * 64 + lane;
                const T beta = (T)(wave_sum_all(cl_dot3(yp[0], yp[64], yp[128], qx, qy, qz)) / rho[p]);   // :447
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
            T xt = dfma<T>(t, px, x0), yt = dfma<T>(t, py, y0), zt = dfma<T>(t, pz, z0);   // :124
            if (__all(is_equal(xt, x0) && is_equal(yt, y0) && is_equal(zt, z0))) { stuck = true; break; }   // :128
            if constexpr (C::kConstrained) C::template project<T>(lane < N, xt, yt, zt);   // :133-135
            T Et, tx, ty, tz;
            cl_wave_eval<T, F>(N, lane, xt, yt, zt, Et, tx, ty, tz);
            if constexpr (C::kConstrained) C::template tangent<T>(xt, yt, zt, tx, ty, tz);
            if (Et < E) {                                    // :139
                dE = Et - E; E = Et;                         // :142-144
                sx = xt - x0; sy = yt - y0; sz = zt - z0;    // :145
                yx = tx - gx; yy = ty - gy; yz = tz - gz;    // :478-480
                x = xt; y = yt; z = zt;
                gx = tx; gy = ty; gz = tz;
                break;
            }
            t *= T(0.5);                                     // :152 (the point was never overwritten: :151)
            if (++h >= max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (stuck) { sx = x0; sy = y0; sz = z0; break; }     // delta_point keeps the copy of :118
        head = head == 0 ? m - 1 : head - 1;                 // pushfirst!, :482-496
        T *sp = hS + head * 3 * 64 + lane, *yp = hY + head * 3 * 64 + lane;
        sp[0] = sx; sp[64] = sy; sp[128] = sz;
        yp[0] = yx; yp[64] = yy; yp[128] = yz;
        rho[head] = wave_sum_all(cl_dot3(sx, sy, sz, yx, yy, yz));   // :505
        if (hc < m) ++hc;
        ++it;                                                // :507
    }
    w.x = x; w.y = y; w.z = z; w.gx = gx; w.gy = gy; w.gz = gz; w.px = px; w.py = py; w.pz = pz;
    w.sx = sx; w.sy = sy; w.sz = sz; w.yx = yx; w.yy = yy; w.yz = yz;
    w.E = E; w.dE = dE;
    w.it = it;
    w.hc = hc; w.halv = halv; w.head = head;
    return stuck;
}

// ------------------------------------------------------------------------------ BLOCK shape: thread t owns particles t, t + 256, ...
// the five vectors [x | y | z] in LDS (only their owner touches an element, except the trial point X, which the pair loop reads
// as a broadcast), the ring (slot p at p * 3N of hS / hY, in LDS or in the slab), rho[m] | alpha[m] | red[2 kWaves] as doubles,
// and the values every thread holds alike
template <typename T> struct QcBlock {
    T *X, *G, *D, *DX, *DG, *hS, *hY;
    double *rho, *alpha, *red;
    T E, dE;
    int64_t it;
    int hc, halv, head, par;
};

// the scale -initial_step_length / |g| of the first direction and is_stuck = iszero(|g0|), :381-387, from the gradients of the
// thread's own particles; every thread passes the barrier of the sum
template <typename T>
__device__ __forceinline__ T qc_block_first_scale(int N, int tid, T step_length, const T (&gx)[kClPer], const T (&gy)[kClPer], const T (&gz)[kClPer],
                                                  double *red, int &par, bool &stuck) {
    double part = 0;
    CL_FOR_OWN(i, part += cl_dot3(gx[q], gy[q], gz[q], gx[q], gy[q], gz[q]);)
    const double gg = cl_block_sum(part, red, par);
    stuck = gg == 0.0;
    return (T)(-((double)step_length / ::sqrt(gg)));
}

// up to `steps` calls of step!() of an instance that is not stuck; returns is_stuck.  The caller's barrier has made X complete.
template <typename T, typename F, typename C = QcFree>
__device__ __forceinline__ bool qc_block_run(int N, int m, int tid, int steps, int64_t max_halvings, QcBlock<T> &w) {
    const int n3 = 3 * N;
    T *const X = w.X, *const G = w.G, *const D = w.D, *const DX = w.DX, *const DG = w.DG, *const hS = w.hS, *const hY = w.hY;
    double *const rho = w.rho, *const alpha = w.alpha, *const red = w.red;
    T E = w.E, dE = w.dE;
    int64_t it = w.it;
    int hc = w.hc, halv = w.halv, head = w.head, par = w.par;
    bool stuck = false;
    for (int s = 0; s < steps && !stuck; ++s) {
        if (it > 0) {                                        // compute_lbfgs_step_direction!, :430-451, on D
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = G[c * N + i];)
            for (int k = 0; k < hc; ++k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * n3, *yp = hY + p * n3;
                double part = 0;
                CL_FOR_OWN(i, part += cl_dot3(sp[i], sp[N + i], sp[2 * N + i], D[i], D[N + i], D[2 * N + i]);)
                const T al = (T)(cl_block_sum(part, red, par) / rho[p]);
                alpha[p] = (double)al;
                CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = dfma<T>(-al, yp[c * N + i], D[c * N + i]);)
            }
            if (hc > 0) {
                const T *yp = hY + head * n3;
                double part = 0;
                CL_FOR_OWN(i, part += cl_dot3(yp[i], yp[N + i], yp[2 * N + i], yp[i], yp[N + i], yp[2 * N + i]);)
                const T gm = (T)(-(rho[head] / cl_block_sum(part, red, par)));
                CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] *= gm;)
            }
            for (int k = hc - 1; k >= 0; --k) {
                const int p = head + k < m ? head + k : head + k - m;
                const T *sp = hS + p * n3, *yp = hY + p * n3;
                double part = 0;
                CL_FOR_OWN(i, part += cl_dot3(yp[i], yp[N + i], yp[2 * N + i], D[i], D[N + i], D[2 * N + i]);)
                const T beta = (T)(cl_block_sum(part, red, par) / rho[p]);
                const T cf = -((T)alpha[p] + beta);
                CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) D[c * N + i] = dfma<T>(cf, sp[c * N + i], D[c * N + i]);)
            }
        }
        // take_backtracking_step!, :107-154: DX keeps the old point (:118), X is the trial (:124)
        CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) DX[c * N + i] = X[c * N + i];)
        T t = T(1);
        int h = 0;
        bool accepted = false;
        T tx[kClPer], ty[kClPer], tz[kClPer];
        for (;;) {
            bool same = true;
            if constexpr (C::kConstrained) {
                // a thread owns all three components of its particles: it votes on the unprojected values and writes the
                // projected ones before the one barrier that publishes the trial
                CL_FOR_OWN(i, {
                    T v[3];
                    for (int c = 0; c < 3; ++c) {
                        v[c] = dfma<T>(t, D[c * N + i], DX[c * N + i]);
                        same = same && is_equal(v[c], DX[c * N + i]);
                    }
                    C::template project<T>(true, v[0], v[1], v[2]);   // :133-135
                    for (int c = 0; c < 3; ++c) X[c * N + i] = v[c];
                })
            } else {
                CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
                    const T v = dfma<T>(t, D[c * N + i], DX[c * N + i]);
                    X[c * N + i] = v;
                    same = same && is_equal(v, DX[c * N + i]);
                })
            }
            if (__syncthreads_and(same ? 1 : 0)) { stuck = true; break; }   // :128; the barrier also publishes the trial point
            T Et;
            cl_block_eval<T, F>(N, tid, X, red, par, Et, tx, ty, tz);       // its barrier: every thread has read X
            if constexpr (C::kConstrained) { CL_FOR_OWN(i, C::template tangent<T>(X[i], X[N + i], X[2 * N + i], tx[q], ty[q], tz[q]);) }
            if (Et < E) { dE = Et - E; E = Et; accepted = true; break; }   // :139-144
            t *= T(0.5);                                                    // :152
            if (++h >= max_halvings) { stuck = true; break; }
        }
        halv = h;
        if (!accepted) {                                     // :151 / the copy of :118 stays in DX
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) X[c * N + i] = DX[c * N + i];)
            break;
        }
        head = head == 0 ? m - 1 : head - 1;                 // pushfirst!, :482-496
        T *sp = hS + head * n3, *yp = hY + head * n3;
        double part = 0;
#pragma unroll
        for (int q = 0; q < kClPer; ++q) {
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
                part += cl_dot3(DX[i], DX[N + i], DX[2 * N + i], DG[i], DG[N + i], DG[2 * N + i]);
            }
        }
        rho[head] = cl_block_sum(part, red, par);            // :505
        if (hc < m) ++hc;
        ++it;
    }
    w.E = E; w.dE = dE;
    w.it = it;
    w.hc = hc; w.halv = halv; w.head = head; w.par = par;
    return stuck;
}

}  // namespace dzo
