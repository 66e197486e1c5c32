// dzo_lowmode.hip -- the lowest Hessian mode of MANY small Lennard-Jones clusters on gfx950 by restarted Lanczos with full
// reorthogonalisation, the whole iteration of every instance inside ONE launch (include/dzo.h, "Batched lowest Hessian mode",
// is the specification; the letters a .. h below are its items).  The only access to the Hessian is the product
// accelerated_pairwise_radial_hvp! (src/ExampleFunctions.jl:427-468): no dense matrix is formed, so the unit serves the 1024
// particles of every other cluster unit where the dense eigensolver stops at 128.
//
// The launch shapes are those of dzo_hessian_batch.hip and the product is its row loop, a plain call of pw_pair<T, F, kPwHvp>
// per pair in the same order, so a product inside the iteration has the bits of dzo_pairwise_batch_hvp:
//
//   * WAVE shape (N <= 64): one wave per instance.  Lane i holds particle i and its three entries of the current vector in
//     registers; particle j arrives through v_readlane.  The Lanczos basis (3 * 64 * K elements) lives in dynamic LDS.
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per instance, thread t owns particles t, t + 256, ...  Point and
//     current vector are staged in dynamic LDS for the pair loop.  The basis lives in a per-call device workspace; a thread
//     reads back only the elements it wrote itself, so the workspace needs no fence.
//
// Both shapes run ONE body (lm_run): what differs is where the basis lives, how the product reaches particle j, and how many
// waves a sum spans.  Sums over the particles are fp64 in a fixed order (item a): cl_dot3 per particle, wave_sum_all, then the
// wave sums in wave order through LDS -- the order of cl_block_sum, for up to 32 values behind one barrier.  The Ritz pair of the
// small tridiagonal is a cyclic Jacobi iteration in fp64 on a K x K matrix in LDS, dealt over all threads of the block.
// Every decision is taken from values that every thread reads from the same LDS words: the control flow is block-uniform.
#include "dzo_chain.h"
#include "dzo_cluster.h"
#include "dzo_pairwise.h"
#include "dzo_pcg.h"

#include <cmath>

namespace dzo {

constexpr int kLmMaxK = DZO_LOWMODE_MAX_KRYLOV;
constexpr int kLmLd = kLmMaxK + 1;                           // odd: a Jacobi row walk touches every LDS bank
constexpr int kLmSweeps = 30;
constexpr int kLmCleanups = 4;
// the fp64 part of the dynamic LDS: wave sums (32 values x 4 waves), alpha and beta, a round's (c, s), the matrix and V
constexpr int kLmRed = 0, kLmTri = kLmRed + kLmMaxK * kWaves, kLmCs = kLmTri + 2 * kLmMaxK, kLmA = kLmCs + kLmMaxK,
              kLmV = kLmA + kLmMaxK * kLmLd, kLmDoubles = kLmV + kLmMaxK * kLmLd;
static_assert(DZO_LOWMODE_MAX_PARTICLES == kClMaxN, "the argument checks of dzo_cluster.h state the particle bound");
static_assert(kLmMaxK <= 32, "the sweep test holds one column per lane of the first wave, a Jacobi phase one row per lane of a half-wave");

template <typename T> struct LowmodeArgs {
    int N, K, max_cycles, project;
    double res_tol;
    uint64_t seed;
    const T *x;                // points (3N, batch)
    const T *start;            // (3N, batch) or null
    T *basis;                  // BLOCK: workspace (3N, K, batch); WAVE: null
    T *eig;                    // (batch)
    T *vec;                    // (3N, batch)
    double *res;               // (batch) or null
    int32_t *info;             // (3, batch) or null
};

extern __shared__ __attribute__((aligned(16))) double lowmode_smem[];

// ------------------------------------------------------------------------------ sums (item a)
// value k of up to kLmMaxK sums: the wave tree, lane 0 of every wave leaves its wave's sum; a barrier; lm_get adds the wave
// sums in wave order from +0 in EVERY thread; a barrier before `red` is written again (the caller's)
template <int W> __device__ __forceinline__ void lm_put(double v, double *red, int k) {
    const double w = wave_sum_all(v);
    if ((threadIdx.x & 63) == 0) red[k * W + (threadIdx.x >> 6)] = w;
}
template <int W> __device__ __forceinline__ double lm_get(const double *red, int k) {
    double r = 0;
#pragma unroll
    for (int wv = 0; wv < W; ++wv) r += red[k * W + wv];
    return r;
}

// ------------------------------------------------------------------------------ Ritz pair (item h)
// idx[p] of the round-robin list after `round` rounds: place 0 stays, places 1 .. m-1 turn by one per round
__device__ __forceinline__ int lm_idx(int p, int round, int m) {
    if (p == 0) return 0;
    int v = p - 1 - round;                                   // in (-(m - 1), m - 1): one conditional add is the modulus
    if (v < 0) v += m - 1;
    return v + 1;
}

// Cyclic Jacobi on the k x k matrix A (column-major, leading dimension kLmLd) with V, all threads of the block; returns the
// index of the smallest diagonal entry (the lowest among equals) in every thread.
__device__ __forceinline__ int lm_jacobi(int k, double *A, double *V, double *cs, double *flag) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int m = k + (k & 1), half = m / 2;
    for (int sweep = 0; sweep <= kLmSweeps; ++sweep) {
        if (tid < 64) {                                      // the first wave, whole
            double off = 0, dia = 0;
            if (tid < k) {
                for (int r = 0; r < k; ++r) {
                    const double v = A[r + kLmLd * tid], sq = v * v;
                    if (r == tid) dia = sq;
                    else off = off + sq;
                }
            }
            const double off2 = wave_sum_all(off), dia2 = wave_sum_all(dia);
            if (tid == 0) *flag = (off2 <= 0x1p-104 * (off2 + dia2)) ? 1.0 : 0.0;
        }
        __syncthreads();
        const bool done = *flag != 0.0 || sweep == kLmSweeps;
        __syncthreads();
        if (done) break;
        for (int round = 0; round < m - 1; ++round) {
            if (tid < half) {                                // angles, from the matrix as it stands (item 4)
                const int i0 = lm_idx(tid, round, m), i1 = lm_idx(m - 1 - tid, round, m);
                const int p = i0 < i1 ? i0 : i1, q = i0 < i1 ? i1 : i0;
                double c = 1.0, s = 0.0;
                if (q < k) {
                    const double apq = A[p + kLmLd * q];
                    if (apq != 0.0) {
                        const double tau = (A[q + kLmLd * q] - A[p + kLmLd * p]) / (apq + apq);
                        const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                    }
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            // work is dealt by (pair, row): thread t takes row t & 31 of the pairs t >> 5, t >> 5 + nt / 32, ...  (k <= 32)
            for (int pr = tid >> 5; pr < half; pr += nt >> 5) {   // columns of A and of V (item 5)
                const int r = tid & 31;
                const int i0 = lm_idx(pr, round, m), i1 = lm_idx(m - 1 - pr, round, m);
                const int p = i0 < i1 ? i0 : i1, q = i0 < i1 ? i1 : i0;
                if (q < k && r < k) {
                    const double c = cs[2 * pr], s = cs[2 * pr + 1];
                    const double ap = A[r + kLmLd * p], aq = A[r + kLmLd * q];
                    A[r + kLmLd * p] = c * ap - s * aq; A[r + kLmLd * q] = s * ap + c * aq;
                    const double vp = V[r + kLmLd * p], vq = V[r + kLmLd * q];
                    V[r + kLmLd * p] = c * vp - s * vq; V[r + kLmLd * q] = s * vp + c * vq;
                }
            }
            __syncthreads();
            for (int pr = tid >> 5; pr < half; pr += nt >> 5) {   // rows of A; the pair's own two entries end as exact zeros
                const int col = tid & 31;
                const int i0 = lm_idx(pr, round, m), i1 = lm_idx(m - 1 - pr, round, m);
                const int p = i0 < i1 ? i0 : i1, q = i0 < i1 ? i1 : i0;
                if (q < k && col < k) {
                    const double c = cs[2 * pr], s = cs[2 * pr + 1];
                    const double ap = A[p + kLmLd * col], aq = A[q + kLmLd * col];
                    A[p + kLmLd * col] = col == q ? 0.0 : c * ap - s * aq; A[q + kLmLd * col] = col == p ? 0.0 : s * ap + c * aq;
                }
            }
            __syncthreads();
        }
    }
    int best = 0;
    double low = A[0];
    for (int c = 1; c < k; ++c) {
        const double d = A[c + kLmLd * c];
        if (d < low) { low = d; best = c; }
    }
    return best;
}

// ------------------------------------------------------------------------------ the iteration, both shapes
template <typename T, typename F, bool BLOCK> __device__ __forceinline__ void lm_run(const LowmodeArgs<T> &a) {
    constexpr int PER = BLOCK ? kClPer : 1, W = BLOCK ? kWaves : 1;
    const int tid = threadIdx.x, N = a.N, K = a.K, max_cycles = a.max_cycles;
    const bool rigid = a.project != 0;
    const int64_t b = pw_pin((int64_t)blockIdx.x), base = (int64_t)3 * N * b;   // addresses only: vector registers
    double *red = lowmode_smem + kLmRed, *tri = lowmode_smem + kLmTri, *cs = lowmode_smem + kLmCs, *JA = lowmode_smem + kLmA,
           *JV = lowmode_smem + kLmV;
    T *Ts = reinterpret_cast<T *>(lowmode_smem + kLmDoubles);   // WAVE: the basis; BLOCK: the point X and the direction D
    T *X = Ts, *D = Ts + 3 * N;
    const double dN = (double)N;
    // the pointers the iteration does not touch wait in VECTOR registers: as kernel arguments they would sit in scalar registers
    // through every loop next to the scalarised pair arithmetic, and the allocator then spills scalars (dzo_pairwise.h)
    T *const out_vec = pw_pin_ptr(a.vec), *const out_eig = pw_pin_ptr(a.eig), *const basis = pw_pin_ptr(a.basis);
    double *const out_res = pw_pin_ptr(a.res);
    int32_t *const out_info = pw_pin_ptr(a.info);
    const double res_tol = pw_pin(a.res_tol);

    bool live[PER];
    T px[PER], py[PER], pz[PER], v[3][PER], w[3][PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + kBlock * q;
        live[q] = i < N;
        px[q] = live[q] ? a.x[base + i] : T(0); py[q] = live[q] ? a.x[base + N + i] : T(0); pz[q] = live[q] ? a.x[base + 2 * N + i] : T(0);
        if constexpr (BLOCK) {
            if (live[q]) { X[i] = px[q]; X[N + i] = py[q]; X[2 * N + i] = pz[q]; }
        }
    }

    // basis vector k, component c, of the thread's particle q (zero for a particle beyond N)
    auto qload = [&](int k, int c, int q) -> T {
        if constexpr (BLOCK) {
            const int i = tid + kBlock * q;
            return live[q] ? basis[(((int64_t)b * K + k) * 3 + c) * N + i] : T(0);
        } else {
            return Ts[(k * 3 + c) * 64 + tid];
        }
    };
    auto qstore = [&](int k, const T (&s)[3][PER]) {
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (BLOCK) {
                    const int i = tid + kBlock * q;
                    if (live[q]) basis[(((int64_t)b * K + k) * 3 + c) * N + i] = s[c][q];
                } else {
                    Ts[(k * 3 + c) * 64 + tid] = s[c][q];
                }
            }
    };
    // one sum / six sums over the particles in every thread (item a)
    auto sum1 = [&](double t) -> double {
        lm_put<W>(t, red, 0);
        __syncthreads();
        const double r = lm_get<W>(red, 0);
        __syncthreads();
        return r;
    };
    auto sum6 = [&](double (&t)[6]) {
#pragma unroll
        for (int k = 0; k < 6; ++k) lm_put<W>(t[k], red, k);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 6; ++k) t[k] = lm_get<W>(red, k);
        __syncthreads();
    };
    auto dot_own = [&](const T (&s)[3][PER], const T (&t)[3][PER]) -> double {
        double r = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) r += cl_dot3(s[0][q], s[1][q], s[2][q], t[0][q], t[1][q], t[2][q]);
        return r;
    };
    // s = sqrt(t.t), t = t (1 / s) (item e); returns s
    auto normalise = [&](T (&t)[3][PER]) -> double {
        const double s = sqrt(sum1(dot_own(t, t))), r = 1.0 / s;
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c][q] = (T)((double)t[c][q] * r);
        return s;
    };

    // ---- item c: the projector
    double cx = 0, cy = 0, cz = 0, I00 = 0, I01 = 0, I02 = 0, I11 = 0, I12 = 0, I22 = 0;
    bool ok = true;
    if (rigid) {
        double t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < PER; ++q) { t[0] += (double)px[q]; t[1] += (double)py[q]; t[2] += (double)pz[q]; }
        sum6(t);
        cx = t[0] / dN; cy = t[1] / dN; cz = t[2] / dN;
        double g[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const double rx = live[q] ? (double)px[q] - cx : 0.0, ry = live[q] ? (double)py[q] - cy : 0.0, rz = live[q] ? (double)pz[q] - cz : 0.0;
            const double xx = rx * rx, yy = ry * ry, zz = rz * rz;
            g[0] += yy + zz; g[1] += xx + zz; g[2] += xx + yy;
            g[3] += rx * ry; g[4] += rx * rz; g[5] += ry * rz;
        }
        sum6(g);
        const double Gxx = g[0], Gyy = g[1], Gzz = g[2], Gxy = -g[3], Gxz = -g[4], Gyz = -g[5];
        const double A00 = Gyy * Gzz - Gyz * Gyz, A01 = Gxz * Gyz - Gxy * Gzz, A02 = Gxy * Gyz - Gxz * Gyy;
        const double A11 = Gxx * Gzz - Gxz * Gxz, A12 = Gxy * Gxz - Gxx * Gyz, A22 = Gxx * Gyy - Gxy * Gxy;
        const double det = Gxx * A00 + Gxy * A01 + Gxz * A02, tr = Gxx + Gyy + Gzz;
        ok = det > 0x1p-36 * ((tr * tr) * tr);
        I00 = A00 / det; I01 = A01 / det; I02 = A02 / det; I11 = A11 / det; I12 = A12 / det; I22 = A22 / det;
    }
    // item d
    auto project = [&](T (&t)[3][PER]) {
        if (!rigid) return;
        double s[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const double rx = live[q] ? (double)px[q] - cx : 0.0, ry = live[q] ? (double)py[q] - cy : 0.0, rz = live[q] ? (double)pz[q] - cz : 0.0;
            const double tx = (double)t[0][q], ty = (double)t[1][q], tz = (double)t[2][q];
            s[0] += tx; s[1] += ty; s[2] += tz;
            s[3] += ry * tz - rz * ty; s[4] += rz * tx - rx * tz; s[5] += rx * ty - ry * tx;
        }
        sum6(s);
        const double mx = s[0] / dN, my = s[1] / dN, mz = s[2] / dN;
        const double ox = I00 * s[3] + I01 * s[4] + I02 * s[5], oy = I01 * s[3] + I11 * s[4] + I12 * s[5], oz = I02 * s[3] + I12 * s[4] + I22 * s[5];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const double rx = (double)px[q] - cx, ry = (double)py[q] - cy, rz = (double)pz[q] - cz;
            const T nx = (T)(((double)t[0][q] - mx) - (oy * rz - oz * ry)), ny = (T)(((double)t[1][q] - my) - (oz * rx - ox * rz)),
                    nz = (T)(((double)t[2][q] - mz) - (ox * ry - oy * rx));
            t[0][q] = live[q] ? nx : T(0); t[1][q] = live[q] ? ny : T(0); t[2][q] = live[q] ? nz : T(0);
        }
    };
    // item b: t = H s, the row loop of dzo_hessian_batch.hip
    auto product = [&](const T (&s)[3][PER], T (&t)[3][PER]) {
        if constexpr (BLOCK) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int i = tid + kBlock * q;
                if (live[q]) { D[i] = s[0][q]; D[N + i] = s[1][q]; D[2 * N + i] = s[2][q]; }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int i = tid + kBlock * q;
                t[0][q] = t[1][q] = t[2][q] = T(0);
                if (i < N) {
                    const PwPoint<T> pi{X[i], X[N + i], X[2 * N + i], D[i], D[N + i], D[2 * N + i]};
                    T ax = T(0), ay = T(0), az = T(0);
                    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int j = j4 + k, jc = j < N ? j : N - 1;   // the padding re-reads the last particle and is dropped
                            const PwPoint<T> pj{X[jc], X[N + jc], X[2 * N + jc], D[jc], D[N + jc], D[2 * N + jc]};
                            pw_pair<T, F, kPwHvp>(j == i || j >= N, pi, pj, ax, ay, az);
                        }
                    }
                    t[0][q] = pw_twice(ax); t[1][q] = pw_twice(ay); t[2][q] = pw_twice(az);
                }
            }
        } else {
            const PwPoint<T> pi{px[0], py[0], pz[0], s[0][0], s[1][0], s[2][0]};
            T ax = T(0), ay = T(0), az = T(0);
            for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j4 + k;
                    const PwPoint<T> pj{lane_read(pi.x, j), lane_read(pi.y, j), lane_read(pi.z, j), lane_read(pi.u, j), lane_read(pi.v, j), lane_read(pi.w, j)};
                    pw_pair<T, F, kPwHvp>(j == tid || j >= N, pi, pj, ax, ay, az);
                }
            }
            t[0][0] = live[0] ? pw_twice(ax) : T(0); t[1][0] = live[0] ? pw_twice(ay) : T(0); t[2][0] = live[0] ? pw_twice(az) : T(0);
        }
    };
    // h_k = q_k.t for k = 0 .. j, then t = t - sum h_k q_k (one pass of classical Gram-Schmidt); returns h_j
    auto orthogonalise = [&](T (&t)[3][PER], int j, bool update) -> double {
        for (int k = 0; k <= j; ++k) {
            double r = 0;
#pragma unroll
            for (int q = 0; q < PER; ++q) r += cl_dot3(qload(k, 0, q), qload(k, 1, q), qload(k, 2, q), t[0][q], t[1][q], t[2][q]);
            lm_put<W>(r, red, k);
        }
        __syncthreads();
        const double hj = lm_get<W>(red, j);
        if (update) {
            double acc[3][PER];
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c][q] = (double)t[c][q];
            for (int k = 0; k <= j; ++k) {
                const double h = lm_get<W>(red, k);
#pragma unroll
                for (int q = 0; q < PER; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c][q] = acc[c][q] - h * (double)qload(k, c, q);
            }
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) t[c][q] = (T)acc[c][q];
        }
        __syncthreads();
        return hj;
    };

    // ---- item f: the start
    const uint64_t stream = pcg_advance(kPcgInc + (a.seed + (uint64_t)b));
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + kBlock * q;
        v[0][q] = v[1][q] = v[2][q] = T(0);
        if (live[q]) {
            if (a.start) { v[0][q] = a.start[base + i]; v[1][q] = a.start[base + N + i]; v[2][q] = a.start[base + 2 * N + i]; }
            else {
                uint64_t s = pcg_jump(stream, (uint64_t)(4 * i));
                const uint32_t d1 = pcg_draw(s), d2 = pcg_draw(s), d3 = pcg_draw(s), d4 = pcg_draw(s);
                pcg_normals<T>(d1, d2, d3, d4, v[0][q], v[1][q], v[2][q]);
            }
        }
    }
    const double kNaN = __builtin_nan("");
    int status = pw_pin((int)DZO_LOWMODE_FAILED), cycles = pw_pin(0), products = pw_pin(0);   // records, not decisions: vector registers
    double alpha1 = kNaN, beta1 = kNaN, scale = 0;
    if (ok) {
        project(v);
        const double s0 = normalise(v);
        ok = s0 > 0 && s0 < INFINITY;
    }
    // ---- items g and h
    for (int cycle = 0; ok && cycle < max_cycles; ++cycle) {
        cycles = pw_pin(cycle + 1);
        qstore(0, v);
        int steps = K;
        bool finished = false;
        for (int j = 0; j < K; ++j) {
            product(v, w);
            products = pw_pin(products + 1);
            project(w);
            const double aj = orthogonalise(w, j, !(j == K - 1 && j > 0));
            if (tid == 0) tri[j] = aj;
            if (j == K - 1 && j > 0) break;
            if (j == 0) {
                alpha1 = aj;
                beta1 = sqrt(sum1(dot_own(w, w)));
                if (fabs(alpha1) > scale) scale = fabs(alpha1);
                if (beta1 <= res_tol * scale) { status = pw_pin((int)DZO_LOWMODE_CONVERGED); finished = true; break; }
                if (cycle == max_cycles - 1) { status = pw_pin((int)DZO_LOWMODE_UNFINISHED); finished = true; break; }
            }
            (void)orthogonalise(w, j, true);
            const double bj = sqrt(sum1(dot_own(w, w)));
            if (!(bj > 0)) { steps = j + 1; break; }
            {
                const double r = 1.0 / bj;
#pragma unroll
                for (int q = 0; q < PER; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) w[c][q] = (T)((double)w[c][q] * r);
            }
            bool dead = false;
            for (int pass = 0; pass < kLmCleanups; ++pass) {
                project(w);
                (void)orthogonalise(w, j, true);
                const double s = normalise(w);
                if (!(s > 0)) { dead = true; break; }
                if (s > 0.7) break;
            }
            if (dead) { steps = j + 1; break; }
            if (tid == 0) tri[kLmMaxK + j] = bj;
            qstore(j + 1, w);
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][q] = w[c][q];
        }
        if (finished) break;
        __syncthreads();                                     // tri is complete
        for (int e = tid; e < steps * steps; e += blockDim.x) {
            const int r = e % steps, c = e / steps;
            JA[r + kLmLd * c] = r == c ? tri[r] : (r == c + 1 ? tri[kLmMaxK + c] : (c == r + 1 ? tri[kLmMaxK + r] : 0.0));
            JV[r + kLmLd * c] = r == c ? 1.0 : 0.0;
        }
        __syncthreads();
        const int best = lm_jacobi(steps, JA, JV, cs, red);
        const double theta = JA[best + kLmLd * best];
        if (fabs(theta) > scale) scale = fabs(theta);
        {
            double acc[3][PER];
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c][q] = 0.0;
            for (int k = 0; k < steps; ++k) {
                const double y = JV[k + kLmLd * best];
#pragma unroll
                for (int q = 0; q < PER; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c][q] = acc[c][q] + y * (double)qload(k, c, q);
            }
#pragma unroll
            for (int q = 0; q < PER; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][q] = live[q] ? (T)acc[c][q] : T(0);
        }
        __syncthreads();                                     // the basis and V have been read: the next cycle overwrites them
        project(v);
        const double s = normalise(v);
        if (!(s > 0 && s < INFINITY)) { status = pw_pin((int)DZO_LOWMODE_FAILED); alpha1 = kNaN; beta1 = kNaN; break; }
    }
    // ---- results: every element once
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + kBlock * q;
        if (live[q]) { out_vec[base + i] = v[0][q]; out_vec[base + N + i] = v[1][q]; out_vec[base + 2 * N + i] = v[2][q]; }
    }
    if (tid == 0) {
        out_eig[b] = (T)alpha1;
        if (out_res) out_res[b] = beta1;
        if (out_info) { out_info[3 * b] = status; out_info[3 * b + 1] = cycles; out_info[3 * b + 2] = products; }
    }
}

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
template <typename T, typename F> __global__ __launch_bounds__(64) void lowmode_wave_kernel(LowmodeArgs<T> a) { lm_run<T, F, false>(a); }

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void lowmode_block_kernel(LowmodeArgs<T> a) { lm_run<T, F, true>(a); }

// ------------------------------------------------------------------------------ host side
template <typename T, typename F> static const void *lm_kernel(bool block) {
    return block ? (const void *)lowmode_block_kernel<T, F> : (const void *)lowmode_wave_kernel<T, F>;
}

static size_t lm_lds_bytes(int N, int K, int32_t dtype) {
    const size_t elems = N <= 64 ? (size_t)3 * 64 * K : (size_t)6 * N;
    return sizeof(double) * kLmDoubles + ((elems * dtype_size(dtype) + 15) & ~(size_t)15);
}

template <typename T, typename F> static void lm_launch(hipStream_t s, int64_t batch, size_t lds, const LowmodeArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((lowmode_wave_kernel<T, F>), dim3((unsigned)batch), dim3(64), lds, s, a);
    else hipLaunchKernelGGL((lowmode_block_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), lds, s, a);
}

// ------------------------------------------------------------------------------ the asynchronous path (dzo_chain.h)
// K of item g: krylov, but no more than the dimension of the range of P
static int lm_krylov(int N, int krylov, int project_rigid) {
    const int64_t range = project_rigid ? 3 * (int64_t)N - 6 : 3 * (int64_t)N;
    return (int)(krylov < range ? krylov : range);
}

// gfx950 has 160 KiB of LDS per CU; dynamic requests above the default need the attribute.  It belongs to the kernel: raised to
// the limit, so that no later call lowers it
int32_t lm_prepare(int32_t radial, int32_t dtype, int N, int krylov, int project_rigid) {
    if (lm_lds_bytes(N, lm_krylov(N, krylov, project_rigid), dtype) > 48 * 1024) {
        const void *k = nullptr;
        DZO_DISPATCH_RADIAL(radial, dtype, k = (lm_kernel<T, F>(N > 64)));
        DZO_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClLdsMax));
    }
    return DZO_OK;
}

int32_t lm_enqueue(hipStream_t s, int32_t radial, int32_t dtype, int N, int64_t batch, const void *points, int32_t project_rigid, int32_t krylov, int32_t max_cycles,
                   double res_tol, uint64_t base_seed, const void *start, void *basis, void *eigenvalues, void *vectors, double *residuals,
                   int32_t *info) {
    const int K = lm_krylov(N, krylov, project_rigid);
    const size_t lds = lm_lds_bytes(N, K, dtype);
    DZO_DISPATCH_RADIAL(radial, dtype,
                        (lm_launch<T, F>(s, batch, lds,
                                         LowmodeArgs<T>{N, K, max_cycles, project_rigid != 0, res_tol, base_seed, (const T *)points, (const T *)start,
                                                        (T *)basis, (T *)eigenvalues, (T *)vectors, residuals, info})));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_pairwise_batch_lowest_mode(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                       int32_t project_rigid, int32_t krylov, int32_t max_cycles, double res_tol, uint64_t base_seed,
                                       const void *start_dev, void *eigenvalues_dev, void *vectors_dev, double *residuals_dev, int32_t *info_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && eigenvalues_dev && vectors_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    DZO_REQUIRE(krylov >= 2 && krylov <= kLmMaxK, DZO_ERR_INVALID, "krylov must be in 2 .. %d (got %d)", kLmMaxK, krylov);
    DZO_REQUIRE(max_cycles >= 1, DZO_ERR_INVALID, "max_cycles must be at least 1 (got %d): a launch cannot iterate without bound", max_cycles);
    DZO_REQUIRE(res_tol >= 0 && std::isfinite(res_tol), DZO_ERR_INVALID, "res_tol must be finite and not negative (got %g)", res_tol);
    DZO_REQUIRE(!project_rigid || n_particles >= 3, DZO_ERR_INVALID,
                "project_rigid needs at least 3 particles (got %lld): fewer have no rotation-free subspace", (long long)n_particles);
    const char *where = "accelerated_pairwise_radial_hvp!", *cite = "src/ExampleFunctions.jl:453-461";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", start_dev, "start"));
    DZO_TRY(require_same_backend(where, cite, eigenvalues_dev, "eigenvalues", vectors_dev, "vectors"));
    DZO_TRY(require_same_backend(where, cite, residuals_dev, "residuals", info_dev, "info"));
    const int N = (int)n_particles;
    Context &c = ctx();
    void *work = nullptr;
    if (N > 64) {
        const size_t bytes = (size_t)3 * N * lm_krylov(N, krylov, project_rigid) * (size_t)batch * dtype_size(dtype);
        const hipError_t e = hipMalloc(&work, bytes);
        if (e == hipErrorOutOfMemory) {
            set_error("dzo_pairwise_batch_lowest_mode: out of device memory for the Lanczos basis (%zu bytes)", bytes);
            (void)hipGetLastError();
            return DZO_ERR_NOMEM;
        }
        DZO_HIP(e);
    }
    int32_t rc = lm_prepare(radial, dtype, N, krylov, project_rigid);
    if (rc == DZO_OK) {
        DZO_TIMED("lowmode", c.stream);
        rc = lm_enqueue(c.stream, radial, dtype, N, batch, points_dev, project_rigid, krylov, max_cycles, res_tol, base_seed, start_dev, work, eigenvalues_dev,
                        vectors_dev, residuals_dev, info_dev);
    }
    hipError_t e = hipSuccess;
    if (rc == DZO_OK) e = hipStreamSynchronize(c.stream);
    if (work) (void)hipFree(work);
    if (rc != DZO_OK) return rc;
    DZO_HIP(e);
    return DZO_OK;
}

}  // extern "C"
