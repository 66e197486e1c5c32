// dzo_hessian_batch.hip -- second-order information of MANY small Lennard-Jones clusters on gfx950: the Hessian-vector product
// accelerated_pairwise_radial_hvp! (src/ExampleFunctions.jl:367-468) with lj_second_derivative (:50-72) of every instance in one
// launch, and the dense 3N x 3N Hessian of every instance from one pass over its pairs.
//
// The launch shapes are those of dzo_cluster.h, which also holds the dots and the block sum used here:
//
//   * WAVE shape (N <= 64): one wave per instance (a block of 64 threads).  Lane i holds particle i and its direction in
//     registers; particle j arrives from lane j through v_readlane, four independent pairs per trip.  No barrier, no LDS.
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per instance, thread t owns particles t, t + 256, ...  Point and
//     direction are staged in static LDS (6 * 1024 elements at most: 48 KiB in fp64) and read as broadcasts by the pair loop.
//
// Per pair the arithmetic is pw_pair<T, F, kPwHvp> of dzo_pairwise.h and nothing else: the self term and the padding are
// dropped by its select.  The row sum of particle i runs j = 0 .. N-1 sequentially in T from +0 and is doubled once, the order
// of the quench's gradient.  u.Hu and u.u are fp64 dots: per particle cl_dot3 (a product and two fused multiply-adds), a
// thread's particles in order, then the wave tree, then the block's four wave sums in wave order (cl_block_sum2).
//
// The Hessian kernels do not run 3N products.  Column (b, j) of the Hessian is the product with the unit direction e_(b,j), and
// in that product every pair term but one is an exact zero (du = dv = dw = 0 gives overlap = 0, g = 0 and a term 0 * f + 0 * d):
//
//   * row block i != j keeps the single term of the pair (i, j) with du = -e_b.  Here it is computed with du = +e_b and its sign
//     is flipped: negation commutes with every rounding of the term (products, sums and the doubling), so the bits are those of
//     the term with -e_b;
//   * row block i == j keeps every term k != i, each with du = +e_b: the sequential sum over k, doubled once.
//
// So a lane calls the pair term three times per pair (b = x, y, z; the radial values of the three calls are one computation),
// writes the nine entries of block (i, j) and adds them to the nine accumulators of block (i, i), which stay in registers and
// are stored once at the end.  For a fixed column and row component the lanes' addresses a N + i are consecutive: every store
// instruction of the pair loop is coalesced.  The kernel is bound by its writes, 9 N^2 elements per instance against N^2 pair
// terms.  Nothing is accumulated in memory: an entry is written once, by one lane.
#include "dzo_chain.h"
#include "dzo_cluster.h"
#include "dzo_pairwise.h"

namespace dzo {

constexpr int kHessMaxN = DZO_HESSIAN_BATCH_MAX_PARTICLES;
constexpr int kHessPer = kHessMaxN / kBlock;                 // particles a thread of the BLOCK shape owns at most
static_assert(kHessMaxN == kClMaxN, "the argument checks of dzo_cluster.h state the particle bound");

template <typename T> struct HessBatchArgs {
    int N;
    int64_t point_stride;      // elements between the points of consecutive instances: 3N, or 0 for one shared point
    const T *x;                // points, instance b at point_stride b
    const T *u;                // hvp: directions (3N, batch)
    T *out;                    // hvp: products (3N, batch); hessian: (3N, 3N, batch), column-major per instance
    double *curv;              // hvp: (2, batch) u.Hu and u.u, or null
};

// (each kernel of this file is its body as a __device__ function and the entry point that calls it: written into the
// __global__ function itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
// ------------------------------------------------------------------------------ products, WAVE shape: grid batch, block 64
template <typename T, typename F> __device__ __forceinline__ void hess_batch_wave_hvp_body(HessBatchArgs<T> a) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b, pbase = a.point_stride * b;
    const bool live = lane < N;
    PwPoint<T> pi;
    pi.x = live ? a.x[pbase + lane] : T(0); pi.y = live ? a.x[pbase + N + lane] : T(0); pi.z = live ? a.x[pbase + 2 * N + lane] : T(0);
    pi.u = live ? a.u[base + lane] : T(0); pi.v = live ? a.u[base + N + lane] : T(0); pi.w = live ? a.u[base + 2 * N + lane] : T(0);
    T ax = T(0), ay = T(0), az = T(0);
    // four independent pairs per trip; j4 + k <= 63 is a lane of the wave, the padding is dropped like the self term
    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j4 + k;
            const PwPoint<T> pj{lane_read(pi.x, j), lane_read(pi.y, j), lane_read(pi.z, j), lane_read(pi.u, j), lane_read(pi.v, j), lane_read(pi.w, j)};
            pw_pair<T, F, kPwHvp>(j == lane || j >= N, pi, pj, ax, ay, az);
        }
    }
    const T px = live ? pw_twice(ax) : T(0), py = live ? pw_twice(ay) : T(0), pz = live ? pw_twice(az) : T(0);   // :421-423
    if (live) { a.out[base + lane] = px; a.out[base + N + lane] = py; a.out[base + 2 * N + lane] = pz; }
    if (!a.curv) return;                                     // the same in every lane
    const double uhu = wave_sum_all(cl_dot3(pi.u, pi.v, pi.w, px, py, pz));
    const double uu = wave_sum_all(cl_dot3(pi.u, pi.v, pi.w, pi.u, pi.v, pi.w));
    if (lane == 0) { a.curv[2 * b] = uhu; a.curv[2 * b + 1] = uu; }
}
template <typename T, typename F> __global__ __launch_bounds__(64) void hess_batch_wave_hvp_kernel(HessBatchArgs<T> a) { hess_batch_wave_hvp_body<T, F>(a); }

// ------------------------------------------------------------------------------ products, BLOCK shape: grid batch, block 256
template <typename T, typename F> __device__ __forceinline__ void hess_batch_block_hvp_body(HessBatchArgs<T> a) {
    __shared__ T XD[6 * kHessMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b, pbase = a.point_stride * b;
    T *X = XD, *D = XD + 3 * N;
    for (int e = tid; e < 3 * N; e += kBlock) { X[e] = a.x[pbase + e]; D[e] = a.u[base + e]; }
    __syncthreads();
    double uhu = 0, uu = 0;
#pragma unroll
    for (int q = 0; q < kHessPer; ++q) {
        const int i = tid + kBlock * q;
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
            const T px = pw_twice(ax), py = pw_twice(ay), pz = pw_twice(az);
            a.out[base + i] = px; a.out[base + N + i] = py; a.out[base + 2 * N + i] = pz;
            uhu += cl_dot3(pi.u, pi.v, pi.w, px, py, pz);
            uu += cl_dot3(pi.u, pi.v, pi.w, pi.u, pi.v, pi.w);
        }
    }
    if (!a.curv) return;                                     // the same in every thread
    cl_block_sum2(uhu, uu, red);
    if (tid == 0) { a.curv[2 * b] = uhu; a.curv[2 * b + 1] = uu; }
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void hess_batch_block_hvp_kernel(HessBatchArgs<T> a) { hess_batch_block_hvp_body<T, F>(a); }

// ------------------------------------------------------------------------------ dense Hessians
// The pair (i, j) seen from particle i at (x, y, z): t[b][a] = the term of row component a for the direction +e_b of particle i
// (pw_pair on a zero accumulator; `drop` = self term or padding gives zeros).
template <typename T, typename F> __device__ __forceinline__ void hb_pair_block(bool drop, T x, T y, T z, T xj, T yj, T zj, T (&t)[3][3]) {
    const PwPoint<T> pj{xj, yj, zj, T(0), T(0), T(0)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t[c][0] = t[c][1] = t[c][2] = T(0);
        const PwPoint<T> pi{x, y, z, c == 0 ? T(1) : T(0), c == 1 ? T(1) : T(0), c == 2 ? T(1) : T(0)};
        pw_pair<T, F, kPwHvp>(drop, pi, pj, t[c][0], t[c][1], t[c][2]);
    }
}

// The three columns (c N + j, c = x, y, z) of the current j as seen by this lane: cx/cy/cz point at row component 0 of particle i.
// They are kept in VECTOR registers and advanced by one column per pair: as scalar expressions of j the 36 store addresses of a
// trip are hoisted into scalar registers next to the scalarised pair arithmetic, and the allocator then spills scalars.
template <typename T> struct HbColumns {
    T *cx, *cy, *cz;
    __device__ __forceinline__ HbColumns(T *col0, int64_t n3, int N)
        : cx(pw_pin_ptr(col0)), cy(pw_pin_ptr(col0 + n3 * N)), cz(pw_pin_ptr(col0 + 2 * n3 * N)) {}
    // block (i, j), i != j: entry (a N + i, c N + j) = the term with du = -e_c, doubled
    __device__ __forceinline__ void store(int N, const T (&t)[3][3]) const {
        using G = __attribute__((address_space(1))) T;    // a pinned pointer has lost its address space: say "global" again
        G *col[3] = {(G *)cx, (G *)cy, (G *)cz};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) col[c][r * N] = -pw_twice(t[c][r]);
    }
    __device__ __forceinline__ void next(int64_t n3) {
        cx = pw_pin_ptr(cx + n3); cy = pw_pin_ptr(cy + n3); cz = pw_pin_ptr(cz + n3);
    }
};

template <typename T> __device__ __forceinline__ void hb_store_diagonal(T *col0, int64_t n3, int N, int i, const T (&acc)[3][3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        T *col = col0 + n3 * ((int64_t)c * N + i);
#pragma unroll
        for (int r = 0; r < 3; ++r) col[r * N] = pw_twice(acc[c][r]);
    }
}

// WAVE shape: grid batch, block 64
template <typename T, typename F> __device__ __forceinline__ void hess_batch_wave_hessian_body(HessBatchArgs<T> a) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, n3 = (int64_t)3 * N, pbase = n3 * b;
    const bool live = lane < N;
    const T x = live ? a.x[pbase + lane] : T(0), y = live ? a.x[pbase + N + lane] : T(0), z = live ? a.x[pbase + 2 * N + lane] : T(0);
    T *col0 = a.out + n3 * n3 * b + lane;
    T acc[3][3] = {};
    HbColumns<T> cols(col0, n3, N);
    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j4 + k;
            const bool drop = j == lane || j >= N;
            T t[3][3];
            hb_pair_block<T, F>(drop, x, y, z, lane_read(x, j), lane_read(y, j), lane_read(z, j), t);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 3; ++r) acc[c][r] += t[c][r];
            if (live && !drop) cols.store(N, t);
            cols.next(n3);
        }
    }
    if (live) hb_store_diagonal<T>(col0, n3, N, lane, acc);
}
template <typename T, typename F> __global__ __launch_bounds__(64) void hess_batch_wave_hessian_kernel(HessBatchArgs<T> a) { hess_batch_wave_hessian_body<T, F>(a); }

// BLOCK shape: grid batch, block 256
template <typename T, typename F> __device__ __forceinline__ void hess_batch_block_hessian_body(HessBatchArgs<T> a) {
    __shared__ T X[3 * kHessMaxN];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, n3 = (int64_t)3 * N, pbase = n3 * b;
    for (int e = tid; e < 3 * N; e += kBlock) X[e] = a.x[pbase + e];
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < kHessPer; ++q) {
        const int i = tid + kBlock * q;
        if (i < N) {
            const T x = X[i], y = X[N + i], z = X[2 * N + i];
            T *col0 = a.out + n3 * n3 * b + i;
            T acc[3][3] = {};
            HbColumns<T> cols(col0, n3, N);
            for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j4 + k, jc = j < N ? j : N - 1;   // the padding re-reads the last particle and is dropped
                    const bool drop = j == i || j >= N;
                    T t[3][3];
                    hb_pair_block<T, F>(drop, x, y, z, X[jc], X[N + jc], X[2 * N + jc], t);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int r = 0; r < 3; ++r) acc[c][r] += t[c][r];
                    if (!drop) cols.store(N, t);
                    cols.next(n3);
                }
            }
            hb_store_diagonal<T>(col0, n3, N, i, acc);
        }
    }
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void hess_batch_block_hessian_kernel(HessBatchArgs<T> a) { hess_batch_block_hessian_body<T, F>(a); }

// ------------------------------------------------------------------------------ host side
template <typename T, typename F> static void hb_launch_hvp(hipStream_t s, int64_t batch, const HessBatchArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((hess_batch_wave_hvp_kernel<T, F>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hess_batch_block_hvp_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

template <typename T, typename F> static void hb_launch_hessian(hipStream_t s, int64_t batch, const HessBatchArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((hess_batch_wave_hessian_kernel<T, F>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((hess_batch_block_hessian_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

// dzo_chain.h: the launch of dzo_pairwise_batch_hessian on `s`, checked arguments, no wait
int32_t hb_enqueue_hessian(hipStream_t s, int32_t radial, int32_t dtype, int N, int64_t batch, const void *points, void *hessians) {
    DZO_DISPATCH_RADIAL(radial, dtype,
                        (hb_launch_hessian<T, F>(s, batch, HessBatchArgs<T>{N, (int64_t)3 * N, (const T *)points, nullptr, (T *)hessians, nullptr})));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

// accelerated_pairwise_radial_hvp! (:427-468) of every instance
int32_t dzo_pairwise_batch_hvp(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev, int64_t point_stride,
                               const void *directions_dev, void *products_dev, double *curvatures_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && directions_dev && products_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    DZO_REQUIRE(point_stride == 0 || point_stride >= 3 * n_particles, DZO_ERR_INVALID,
                "point_stride must be 0 (one shared point) or at least 3 n_particles = %lld (got %lld)", (long long)(3 * n_particles),
                (long long)point_stride);
    const char *where = "accelerated_pairwise_radial_hvp!", *cite = "src/ExampleFunctions.jl:453-461";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", directions_dev, "directions"));
    DZO_TRY(require_same_backend(where, cite, products_dev, "products", curvatures_dev, "curvatures"));
    Context &c = ctx();
    {
        DZO_TIMED("hess_batch_hvp", c.stream);
        DZO_DISPATCH_RADIAL(radial, dtype,
                            (hb_launch_hvp<T, F>(c.stream, batch,
                                                 HessBatchArgs<T>{(int)n_particles, point_stride, (const T *)points_dev, (const T *)directions_dev,
                                                                  (T *)products_dev, curvatures_dev})));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// the dense Hessian of every instance: column c is the product above with the unit direction e_c
int32_t dzo_pairwise_batch_hessian(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev, void *hessians_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && hessians_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(cl_check_args(radial, n_particles, batch, dtype));
    DZO_TRY(require_same_backend("accelerated_pairwise_radial_hvp!", "src/ExampleFunctions.jl:453-461", points_dev, "points", hessians_dev, "hessians"));
    Context &c = ctx();
    {
        DZO_TIMED("hess_batch_hessian", c.stream);
        DZO_TRY(hb_enqueue_hessian(c.stream, radial, dtype, (int)n_particles, batch, points_dev, hessians_dev));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

}  // extern "C"
