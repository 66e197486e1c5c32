// dzo_quench_args.h -- what dzo_lbfgs_batch.hip (constraint_function! = nothing) and dzo_sphere.hip (the unit sphere) share around
// qc_wave_run / qc_block_run of dzo_quench_core.h: the arguments of the batched L-BFGS kernels, the handle (ClCore plus the ring
// arrays) with its LDS layout, allocation, kernel arguments and `what` table, and the load and store halves of a step kernel
// (load -> run -> store; the run is the caller's line, with its functor and its constraint policy).
// The step kernels of dzo_lbfgs_batch.hip keep their two halves written out: built on the functions below they store the same
// values, but 11315 of the 107522 lines of that unit's gfx950 assembly change (other register allocation; the Morse fp64 wave
// kernel parks two more scalars), and that unit's instruction stream is not this header's to choose ("Where the shared
// Lennard-Jones pieces live").  That rests on the assembly diff alone: the register and spill pins of tests/test_quench_build.py
// still hold with the shared form, and no timing of it was taken.  Until one is, a change to a half is made in both places.  Every name here starts with qa_ (functions) or is QuenchArgs / QaBlockPtrs / QaHandle.  No kernel
// and no LDS declaration here: the caller passes its dynamic LDS.
#pragma once
#include "dzo_quench_core.h"

namespace dzo {

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

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
// LDS: rho[m] | alpha[m] | S ring | Y ring; element (slot p, component c) of this lane at (p * 3 + c) * 64 + lane
template <typename T> __device__ __forceinline__ void qa_wave_lds(double *smem, int m, double *&rho, double *&alpha, T *&hS, T *&hY) {
    rho = smem; alpha = rho + m;
    hS = reinterpret_cast<T *>(alpha + m); hY = hS + m * 3 * 64;
}

// the state of instance blockIdx.x into registers (zeros in the lanes without a particle) and its ring into LDS, newest at slot 0
template <typename T> __device__ __forceinline__ void qa_wave_load(const QuenchArgs<T> &a, QcWave<T> &w, double *rho, T *hS, T *hY) {
    const int lane = threadIdx.x, N = a.N, m = a.m;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    const bool live = lane < N;
    auto ld = [&](const T *p, int c) { return live ? p[base + c * N + lane] : T(0); };
    w.x = ld(a.x, 0); w.y = ld(a.x, 1); w.z = ld(a.x, 2);
    w.gx = ld(a.g, 0); w.gy = ld(a.g, 1); w.gz = ld(a.g, 2);
    w.px = ld(a.d, 0); w.py = ld(a.d, 1); w.pz = ld(a.d, 2);
    w.sx = ld(a.dx, 0); w.sy = ld(a.dx, 1); w.sz = ld(a.dx, 2);
    w.yx = ld(a.dg, 0); w.yy = ld(a.dg, 1); w.yz = ld(a.dg, 2);
    w.E = a.f[b]; w.dE = a.df[b];
    w.it = a.iters[b];
    w.hc = a.hcount[b]; w.halv = a.halv[b]; w.head = 0;
    const int hc0 = w.hc;
    const int64_t hbase = (int64_t)3 * N * m * b;
    for (int k = 0; k < hc0; ++k) {
        rho[k] = a.rho[(int64_t)m * b + k];                  // every lane the same value to the same address
        for (int c = 0; c < 3; ++c) {
            hS[(k * 3 + c) * 64 + lane] = live ? a.S[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
            hY[(k * 3 + c) * 64 + lane] = live ? a.Y[hbase + (int64_t)3 * N * k + c * N + lane] : T(0);
        }
    }
}

// ... and back, the ring unrolled from its head
template <typename T> __device__ __forceinline__ void qa_wave_store(const QuenchArgs<T> &a, const QcWave<T> &w, bool stuck, const double *rho, const T *hS, const T *hY) {
    const int lane = threadIdx.x, N = a.N, m = a.m;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b, hbase = (int64_t)3 * N * m * b;
    const int hc = w.hc, head = w.head;
    if (lane < N) {
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

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
// the addresses of instance blockIdx.x, pinned to vector registers (pw_pin_ptr): the kernel uses them again when its loop ends
template <typename T> struct QaBlockPtrs {
    T *x, *g, *d, *dx, *dg, *S, *Y, *f, *df;
    double *rho;
    int32_t *stuck, *hc, *halv;
    int64_t *it;
};

template <typename T> __device__ __forceinline__ QaBlockPtrs<T> qa_block_pin(const QuenchArgs<T> &a) {
    const int64_t b = blockIdx.x, base = (int64_t)3 * a.N * b, hbase = (int64_t)3 * a.N * a.m * b;
    QaBlockPtrs<T> p;
    p.x = pw_pin_ptr(a.x + base); p.g = pw_pin_ptr(a.g + base); p.d = pw_pin_ptr(a.d + base);
    p.dx = pw_pin_ptr(a.dx + base); p.dg = pw_pin_ptr(a.dg + base);
    p.S = pw_pin_ptr(a.S + hbase); p.Y = pw_pin_ptr(a.Y + hbase); p.f = pw_pin_ptr(a.f + b); p.df = pw_pin_ptr(a.df + b);
    p.rho = pw_pin_ptr(a.rho + (int64_t)a.m * b);
    p.stuck = pw_pin_ptr(a.stuck + b); p.hc = pw_pin_ptr(a.hcount + b); p.halv = pw_pin_ptr(a.halv + b);
    p.it = pw_pin_ptr(a.iters + b);
    return p;
}

// LDS: rho[m] | alpha[m] | red[2 kWaves] | X | G | D | DX | DG | (S ring | Y ring); HL: the history ring is in LDS (else in a.slab).
// The scalars of the state come from the pinned addresses.
template <typename T, bool HL> __device__ __forceinline__ QcBlock<T> qa_block_place(const QuenchArgs<T> &a, const QaBlockPtrs<T> &g, double *smem) {
    const int m = a.m, n3 = 3 * a.N;
    const int64_t hbase = (int64_t)n3 * m * blockIdx.x;
    double *rho = smem, *alpha = rho + m, *red = alpha + m;
    T *X = reinterpret_cast<T *>(red + 2 * kWaves), *G = X + n3, *D = G + n3, *DX = D + n3, *DG = DX + n3;
    T *hS, *hY;
    if constexpr (HL) { hS = DG + n3; hY = hS + (size_t)m * n3; }
    else { hS = a.slab + 2 * hbase; hY = hS + (size_t)m * n3; }
    return QcBlock<T>{X, G, D, DX, DG, hS, hY, rho, alpha, red, *g.f, *g.df, *g.it, *g.hc, *g.halv, 0, 0};
}

// the vectors and the ring of the thread's own particles (only their owner touches an element before the run's first barrier)
template <typename T> __device__ __forceinline__ void qa_block_load(const QuenchArgs<T> &a, const QaBlockPtrs<T> &g, const QcBlock<T> &w) {
    const int tid = threadIdx.x, N = a.N, n3 = 3 * N;
    const int hc0 = w.hc;
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        w.X[e] = g.x[e]; w.G[e] = g.g[e]; w.D[e] = g.d[e]; w.DX[e] = g.dx[e]; w.DG[e] = g.dg[e];
        for (int k = 0; k < hc0; ++k) { w.hS[k * n3 + e] = g.S[(int64_t)n3 * k + e]; w.hY[k * n3 + e] = g.Y[(int64_t)n3 * k + e]; }
    })
    for (int k = 0; k < hc0; ++k) w.rho[k] = g.rho[k];   // every thread the same value to the same address
}

template <typename T> __device__ __forceinline__ void qa_block_store(const QuenchArgs<T> &a, const QaBlockPtrs<T> &g, const QcBlock<T> &w, bool stuck) {
    const int tid = threadIdx.x, N = a.N, m = a.m, n3 = 3 * N;
    const int hc = w.hc, head = w.head;
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        g.x[e] = w.X[e]; g.g[e] = w.G[e]; g.d[e] = w.D[e]; g.dx[e] = w.DX[e]; g.dg[e] = w.DG[e];
    })
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) {
        const int e = c * N + i;
        for (int k = 0; k < hc; ++k) {
            const int p = head + k < m ? head + k : head + k - m;
            g.S[(int64_t)n3 * k + e] = w.hS[p * n3 + e];
            g.Y[(int64_t)n3 * k + e] = w.hY[p * n3 + e];
        }
    })
    if (tid < hc) g.rho[tid] = w.rho[head + tid < m ? head + tid : head + tid - m];
    if (tid == 0) {
        *g.f = w.E; *g.df = w.dE;
        *g.stuck = stuck ? 1 : 0;
        *g.it = w.it;
        *g.hc = hc; *g.halv = w.halv;
    }
}

// ------------------------------------------------------------------------------ host side
// the handle of either unit: ClCore plus the ring arrays (dzo_lbfgs_batch_s and dzo_sphere_lbfgs_batch_s are this)
struct QaHandle {
    ClCore core;
    int m = 0;
    void *d = nullptr, *S = nullptr, *Y = nullptr, *slab = nullptr;
    int32_t *hcount = nullptr;
    double *rho = nullptr;
    bool hist_lds = true;
};

template <typename H> void qa_free(H *h) { cl_free(h, {h->d, h->S, h->Y, h->slab, h->hcount, h->rho}); }

// history_length, the dynamic LDS of a step launch, where the ring lives, and the handle's device arrays (cleared); core.N, core.B
// and core.dtype are set
inline int32_t qa_alloc(QaHandle *h, int32_t history_length) {
    ClCore &c = h->core;
    h->m = history_length;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, n3 = 3 * (size_t)c.N, m = (size_t)history_length;
    const size_t small = 16 * m;                              // rho | alpha
    if (c.N <= 64) {
        c.lds_bytes = small + 2 * m * 3 * 64 * es;
    } else {
        const size_t vectors = small + 16 * kWaves + 5 * n3 * es;
        h->hist_lds = vectors + 2 * m * n3 * es <= kClLdsMax;
        c.lds_bytes = h->hist_lds ? vectors + 2 * m * n3 * es : vectors;
    }
    return cl_alloc({{&c.g, es * n3 * B}, {&h->d, es * n3 * B}, {&c.dx, es * n3 * B}, {&c.dg, es * n3 * B}, {&c.f, es * B}, {&c.df, es * B},
                     {&h->S, es * n3 * m * B}, {&h->Y, es * n3 * m * B}, {h->hist_lds ? nullptr : &h->slab, 2 * es * n3 * m * B},
                     {(void **)&c.stuck, 4 * B}, {(void **)&h->hcount, 4 * B}, {(void **)&c.halv, 4 * B}, {(void **)&c.iters, 8 * B},
                     {(void **)&c.active_dev, 8}, {(void **)&h->rho, 8 * m * B}},
                    "the batched L-BFGS state");
}

template <typename T> QuenchArgs<T> qa_args(const QaHandle *h, int steps, int init, double step_length) {
    const ClCore &c = h->core;
    QuenchArgs<T> a;
    a.N = c.N; a.m = h->m; a.steps = steps; a.init = init;
    a.max_halvings = c.max_halvings;
    a.step_length = (T)step_length;
    a.x = (T *)c.x; a.g = (T *)c.g; a.d = (T *)h->d; a.dx = (T *)c.dx; a.dg = (T *)c.dg;
    a.f = (T *)c.f; a.df = (T *)c.df;
    a.stuck = c.stuck; a.hcount = h->hcount; a.halv = c.halv; a.iters = c.iters;
    a.S = (T *)h->S; a.Y = (T *)h->Y; a.rho = h->rho; a.slab = (T *)h->slab;
    return a;
}

// `what` (a DZO_LBFGS_BATCH_* constant) -> device address, bytes
inline int32_t qa_array(QaHandle *h, int32_t what, void **p, size_t *bytes) {
    const ClCore &c = h->core;
    const size_t es = dtype_size(c.dtype), B = (size_t)c.B, n3 = 3 * (size_t)c.N, m = (size_t)h->m;
    switch (what) {
    case DZO_LBFGS_BATCH_POINTS: *p = c.x; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_GRADIENTS: *p = c.g; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DIRECTIONS: *p = h->d; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DELTA_POINTS: *p = c.dx; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_DELTA_GRADIENTS: *p = c.dg; *bytes = es * n3 * B; break;
    case DZO_LBFGS_BATCH_OBJECTIVES: *p = c.f; *bytes = es * B; break;
    case DZO_LBFGS_BATCH_DELTA_OBJECTIVES: *p = c.df; *bytes = es * B; break;
    case DZO_LBFGS_BATCH_IS_STUCK: *p = c.stuck; *bytes = 4 * B; break;
    case DZO_LBFGS_BATCH_ITERATION_COUNTS: *p = c.iters; *bytes = 8 * B; break;
    case DZO_LBFGS_BATCH_HISTORY_COUNTS: *p = h->hcount; *bytes = 4 * B; break;
    case DZO_LBFGS_BATCH_S: *p = h->S; *bytes = es * n3 * m * B; break;
    case DZO_LBFGS_BATCH_Y: *p = h->Y; *bytes = es * n3 * m * B; break;
    case DZO_LBFGS_BATCH_RHO: *p = h->rho; *bytes = 8 * m * B; break;
    case DZO_LBFGS_BATCH_LAST_HALVINGS: *p = c.halv; *bytes = 4 * B; break;
    default: set_error("unknown batched L-BFGS array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo
