// dzo_structure.hip -- which of MANY small Lennard-Jones clusters are the same structure, on gfx950: a fingerprint of every
// instance that does not change under rotation, translation, reflection or a relabelling of the particles, and a classifier
// of fingerprints (include/dzo.h has the contract of both).
//
// The fingerprint of an instance is [e sorted ascending | d sorted ascending]: e_i the energy of particle i (the `row` of the
// evaluation routines of dzo_cluster.h: pw_pair of dzo_pairwise.h summed over j ascending in the element type, the self term
// dropped by its select) and d_i its squared distance from the centroid.  The launch shapes are those of dzo_cluster.h:
//
//   * WAVE shape (N <= 64): one wave per instance (a block of 64 threads).  Lane i holds particle i; particle j arrives from
//     lane j through v_readlane, four independent pairs per trip.  The two sorts are bitonic networks across the lanes.  No
//     barrier, no LDS.
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per instance, thread t owns particles t, t + 256, ...  The point is
//     staged in static LDS (3 * 1024 elements: 24 KiB in fp64) and read as broadcasts by the pair loop.  When every thread has
//     its e and d in registers the same LDS becomes the two sort buffers (2 * P keys, P the next power of two >= N).
//
// Sums over the particles (the total energy, the three centroid coordinates) are fp64 sums in the fixed order of
// wave_sum_all / cl_block_sum: a thread's particles in order, the wave tree, the four waves in wave order.  The total energy
// therefore has the bits of dzo_pairwise_batch_energy_gradient.
//
// The sort works on integer keys whose unsigned order is the order of the values: the bits of a non-negative value with the
// sign bit set, the complement of the bits of a negative value.  A value that is not a number gets the key below the largest
// one and comes back as the canonical quiet NaN; the padding has the largest key and is never written out.  So NaNs sort last
// among the N values, behind +inf, whatever their sign or payload.
//
// The classifier is two launches.  structcmp_kernel fills the lower triangle of a batch x batch bit matrix, 64 pairs per wave
// (one ballot, one 64-bit word written once by one lane): bit (k, j), j < k, says that k and j match, bit (k, k) that every
// element of k is finite.  A pair's comparison leaves at the first failing element.  structlabel_kernel is ONE wave that walks
// k = 0 .. batch-1: the mask of representatives so far lives in registers (lane l holds words l, l + 64, l + 128, l + 192 of
// it: 16384 bits), a row is masked by it, and the lowest surviving bit is found by a wave-wide minimum.  Nothing depends on
// the grid size or on the order in which waves run.
#include "dzo_cluster.h"
#include "dzo_pairwise.h"

#include <cmath>

namespace dzo {

constexpr int kStructMaxN = DZO_STRUCTURE_MAX_PARTICLES;
constexpr int kStructPer = kStructMaxN / kBlock;             // particles a thread of the BLOCK shape owns at most
constexpr int64_t kStructMaxBatch = DZO_STRUCTURE_MAX_BATCH;
constexpr int kStructRepWords = (int)(kStructMaxBatch / 64 / 64);   // words of the representative mask a lane holds
static_assert(kStructMaxN == kClMaxN, "the launch shapes of dzo_cluster.h state the particle bound");
static_assert(kStructRepWords * 64 * 64 == kStructMaxBatch, "the label kernel holds the representative mask in one wave's registers");

template <typename T> struct StructFpArgs {
    int N;
    const T *x;                // points (3N, batch)
    T *fp;                     // fingerprints (2N, batch)
    T *energy;                 // batch, or null
};

// ------------------------------------------------------------------------------ sort keys
template <typename T> struct StructKey;
template <> struct StructKey<double> {
    using type = unsigned long long;
    static __device__ __forceinline__ type bits(double v) { return (type)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(type k) { return __longlong_as_double((long long)k); }
    static constexpr type kSign = 0x8000000000000000ull, kNan = 0x7FF8000000000000ull;
};
template <> struct StructKey<float> {
    using type = unsigned int;
    static __device__ __forceinline__ type bits(float v) { return (type)__float_as_int(v); }
    static __device__ __forceinline__ float value(type k) { return __int_as_float((int)k); }
    static constexpr type kSign = 0x80000000u, kNan = 0x7FC00000u;
};

template <typename T> __device__ __forceinline__ typename StructKey<T>::type sk_pad() { return ~(typename StructKey<T>::type)0; }

template <typename T> __device__ __forceinline__ typename StructKey<T>::type sk_key(T v) {
    using K = StructKey<T>;
    const typename K::type b = K::bits(v);
    const typename K::type k = (b & K::kSign) ? ~b : (b | K::kSign);
    return v != v ? (typename K::type)(sk_pad<T>() - 1) : k;
}

template <typename T> __device__ __forceinline__ T sk_value(typename StructKey<T>::type k) {
    using K = StructKey<T>;
    const typename K::type b = (k & K::kSign) ? (k ^ K::kSign) : ~k;
    return K::value(k == (typename K::type)(sk_pad<T>() - 1) ? K::kNan : b);
}

__device__ __forceinline__ unsigned int sk_lane_xor(unsigned int v, int j) { return (unsigned int)__shfl_xor((int)v, j, 64); }
__device__ __forceinline__ unsigned long long sk_lane_xor(unsigned long long v, int j) {
    return (unsigned long long)__shfl_xor((long long)v, j, 64);
}

// ascending bitonic sort of two keys per lane across the first P lanes (P a power of two, 2 .. 64); all 64 lanes take part
template <typename K> __device__ __forceinline__ void sk_wave_sort2(int lane, int P, K &a, K &b) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const K oa = sk_lane_xor(a, j), ob = sk_lane_xor(b, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            a = keep_min ? (oa < a ? oa : a) : (oa > a ? oa : a);
            b = keep_min ? (ob < b ? ob : b) : (ob > b ? ob : b);
        }
    }
}

__host__ __device__ __forceinline__ int sk_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// ------------------------------------------------------------------------------ fingerprints, WAVE shape: grid batch, block 64
// (a fingerprint kernel is its body as a __device__ function and the entry point that calls it: written into the __global__
// function itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
template <typename T, typename F> __device__ __forceinline__ void structfp_wave_body(StructFpArgs<T> a) {
    using Key = typename StructKey<T>::type;
    const int lane = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b, obase = (int64_t)2 * N * b;
    const bool live = lane < N;
    const PwPoint<T> pi{live ? a.x[base + lane] : T(0), live ? a.x[base + N + lane] : T(0), live ? a.x[base + 2 * N + lane] : T(0), T(0), T(0), T(0)};
    T row = T(0), unused_y = T(0), unused_z = T(0);
    // four independent pairs per trip; j4 + k <= 63 is a lane of the wave, the padding is dropped like the self term
    for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j4 + k;
            const PwPoint<T> pj{lane_read(pi.x, j), lane_read(pi.y, j), lane_read(pi.z, j), T(0), T(0), T(0)};
            pw_pair<T, F, kPwEnergy>(j == lane || j >= N, pi, pj, row, unused_y, unused_z);
        }
    }
    const T E = (T)(0.5 * wave_sum_all(live ? (double)row : 0.0));
    const double n = (double)N;
    const T cx = (T)(wave_sum_all(live ? (double)pi.x : 0.0) / n);
    const T cy = (T)(wave_sum_all(live ? (double)pi.y : 0.0) / n);
    const T cz = (T)(wave_sum_all(live ? (double)pi.z : 0.0) / n);
    const T d = pw_r2(pi.x - cx, pi.y - cy, pi.z - cz);
    Key ke = live ? sk_key<T>(row) : sk_pad<T>(), kd = live ? sk_key<T>(d) : sk_pad<T>();
    sk_wave_sort2<Key>(lane, sk_pow2(N), ke, kd);
    if (live) { a.fp[obase + lane] = sk_value<T>(ke); a.fp[obase + N + lane] = sk_value<T>(kd); }
    if (a.energy && lane == 0) a.energy[b] = E;
}
template <typename T, typename F> __global__ __launch_bounds__(64) void structfp_wave_kernel(StructFpArgs<T> a) { structfp_wave_body<T, F>(a); }

// ------------------------------------------------------------------------------ fingerprints, BLOCK shape: grid batch, block 256
template <typename T, typename F> __device__ __forceinline__ void structfp_block_body(StructFpArgs<T> a) {
    using Key = typename StructKey<T>::type;
    static_assert(sizeof(Key) == sizeof(T), "the sort buffers take the place of the point");
    __shared__ T X[3 * kStructMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b, obase = (int64_t)2 * N * b;
    for (int e = tid; e < 3 * N; e += kBlock) X[e] = a.x[base + e];
    __syncthreads();
    int par = 0;
    double sx = 0, sy = 0, sz = 0;
    CL_FOR_OWN(i, sx += (double)X[i]; sy += (double)X[N + i]; sz += (double)X[2 * N + i];)
    const double n = (double)N;
    const T cx = (T)(cl_block_sum(sx, red, par) / n);
    const T cy = (T)(cl_block_sum(sy, red, par) / n);
    const T cz = (T)(cl_block_sum(sz, red, par) / n);
    T e_own[kStructPer], d_own[kStructPer];
    double rows = 0;
#pragma unroll
    for (int q = 0; q < kStructPer; ++q) {
        const int i = tid + kBlock * q;
        e_own[q] = d_own[q] = T(0);
        if (i < N) {
            const PwPoint<T> pi{X[i], X[N + i], X[2 * N + i], T(0), T(0), T(0)};
            T row = T(0), unused_y = T(0), unused_z = T(0);
            for (int j4 = 0; j4 < N; j4 += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j4 + k, jc = j < N ? j : N - 1;   // the padding re-reads the last particle and is dropped
                    const PwPoint<T> pj{X[jc], X[N + jc], X[2 * N + jc], T(0), T(0), T(0)};
                    pw_pair<T, F, kPwEnergy>(j == i || j >= N, pi, pj, row, unused_y, unused_z);
                }
            }
            rows += (double)row;
            e_own[q] = row;
            d_own[q] = pw_r2(pi.x - cx, pi.y - cy, pi.z - cz);
        }
    }
    const T E = (T)(0.5 * cl_block_sum(rows, red, par));
    __syncthreads();                                         // every thread is done with the point: its place becomes the keys
    const int P = sk_pow2(N);                                // 128 .. 1024: 2 P keys fit in the 3 * 1024 elements of X
    Key *KE = reinterpret_cast<Key *>(X), *KD = KE + P;
    CL_FOR_OWN(i, KE[i] = sk_key<T>(e_own[q]); KD[i] = sk_key<T>(d_own[q]);)
    for (int i = N + tid; i < P; i += kBlock) { KE[i] = sk_pad<T>(); KD[i] = sk_pad<T>(); }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kBlock) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;   // bit j of lo is clear; lo < hi < P
                const bool up = (lo & k) == 0;
                const Key ea = KE[lo], eb = KE[hi], da = KD[lo], db = KD[hi];
                if ((ea > eb) == up) { KE[lo] = eb; KE[hi] = ea; }
                if ((da > db) == up) { KD[lo] = db; KD[hi] = da; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < N; i += kBlock) { a.fp[obase + i] = sk_value<T>(KE[i]); a.fp[obase + N + i] = sk_value<T>(KD[i]); }
    if (a.energy && tid == 0) a.energy[b] = E;
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void structfp_block_kernel(StructFpArgs<T> a) { structfp_block_body<T, F>(a); }

// ------------------------------------------------------------------------------ the match matrix: grid (words / 4, batch), block 256
// wave (k, w) forms word w of row k: bit l is the pair (k, j = 64 w + l)
template <typename T> __global__ __launch_bounds__(kBlock) void structcmp_kernel(int64_t length, int batch, int words, double tol, const T *fp,
                                                                                 unsigned long long *bits) {
    const int lane = threadIdx.x & 63, w = (int)blockIdx.x * kWaves + (threadIdx.x >> 6), k = blockIdx.y;
    if (w >= words || 64 * w > k) return;                    // the whole wave: the word is above the diagonal
    const int j = 64 * w + lane;
    bool ok = j <= k;                                        // j <= k < batch
    if (ok) {
        const T *pa = fp + length * k, *pb = fp + length * j;
        for (int64_t i = 0; i < length; ++i) {
            const double va = (double)pa[i], vb = (double)pb[i];
            const double fa = __builtin_fabs(va), fb = __builtin_fabs(vb);
            const double big = fa > fb ? fa : fb, scale = big > 1.0 ? big : 1.0;
            ok = fa < __builtin_inf() && fb < __builtin_inf() && __builtin_fabs(va - vb) <= tol * scale;
            if (!ok) break;
        }
    }
    const unsigned long long word = __ballot(ok);
    if (lane == 0) bits[(int64_t)k * words + w] = word;
}

// ------------------------------------------------------------------------------ greedy leader labels: grid 1, block 64
__global__ __launch_bounds__(64) void structlabel_kernel(int batch, int words, const unsigned long long *bits, int32_t *labels, int32_t *n_classes) {
    const int lane = threadIdx.x;
    unsigned long long rep[kStructRepWords] = {};
    int32_t count = 0;
    for (int k = 0; k < batch; ++k) {
        const int wk = k >> 6;
        const unsigned long long self = 1ull << (k & 63);
        int first = 0x7FFFFFFF;
        bool finite = false;
#pragma unroll
        for (int q = kStructRepWords - 1; q >= 0; --q) {
            const int w = lane + 64 * q;
            if (w <= wk) {                                   // w < words, and the word has been written
                const unsigned long long row = bits[(int64_t)k * words + w];
                if (w == wk) finite = (row & self) != 0;
                const unsigned long long m = row & rep[q];   // k itself is not a representative yet
                if (m) first = 64 * w + __builtin_ctzll(m);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int other = __shfl_xor(first, off, 64);
            first = other < first ? other : first;
        }
        const bool is_finite = __ballot(finite) != 0;
        const bool leader = first == 0x7FFFFFFF && is_finite;
        if (leader) {
            ++count;
#pragma unroll
            for (int q = 0; q < kStructRepWords; ++q)
                if (lane + 64 * q == wk) rep[q] |= self;
        }
        if (lane == 0) labels[k] = first != 0x7FFFFFFF ? first : (is_finite ? k : -1);
    }
    if (lane == 0) n_classes[0] = count;
}

// ------------------------------------------------------------------------------ host side
template <typename T, typename F> static void sf_launch(hipStream_t s, int64_t batch, const StructFpArgs<T> &a) {
    if (a.N <= 64) hipLaunchKernelGGL((structfp_wave_kernel<T, F>), dim3((unsigned)batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((structfp_block_kernel<T, F>), dim3((unsigned)batch), dim3(kBlock), 0, s, a);
}

template <typename T> static void sf_launch_cmp(hipStream_t s, int64_t length, int batch, int words, double tol, const void *fp, unsigned long long *bits) {
    hipLaunchKernelGGL(structcmp_kernel<T>, dim3((unsigned)((words + kWaves - 1) / kWaves), (unsigned)batch), dim3(kBlock), 0, s, length, batch, words,
                       tol, (const T *)fp, bits);
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_structure_batch_fingerprint(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, const void *points_dev,
                                        void *fingerprints_dev, void *energies_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(points_dev && fingerprints_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_args(radial, dtype, n_particles, batch, "batch", kStructMaxN, DZO_ERR_UNSUPPORTED,
                          "the fingerprint kernels hold an instance in one block"));
    const char *where = "dzo_structure_batch_fingerprint", *cite = "include/dzo.h";
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", fingerprints_dev, "fingerprints"));
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", energies_dev, "energies"));
    Context &c = ctx();
    {
        DZO_TIMED("structure_fingerprint", c.stream);
        DZO_DISPATCH_RADIAL(radial, dtype,
                            (sf_launch<T, F>(c.stream, batch, StructFpArgs<T>{(int)n_particles, (const T *)points_dev, (T *)fingerprints_dev, (T *)energies_dev})));
        DZO_HIP(hipGetLastError());
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

int32_t dzo_structure_batch_classify(int64_t length, int64_t batch, int32_t dtype, const void *fingerprints_dev, double tol, int32_t *labels_dev,
                                     int32_t *n_classes) {
    DZO_TRY(require_init());
    DZO_REQUIRE(fingerprints_dev && labels_dev && n_classes, DZO_ERR_INVALID, "null argument");
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(length >= 1 && length <= ((int64_t)1 << 30), DZO_ERR_INVALID, "length must be in 1 .. 2^30 (got %lld)", (long long)length);
    DZO_REQUIRE(batch >= 1, DZO_ERR_INVALID, "batch must be at least 1 (got %lld)", (long long)batch);
    DZO_REQUIRE(tol >= 0, DZO_ERR_INVALID, "tol must be a number that is not negative (got %g)", tol);   // false for NaN
    DZO_REQUIRE(batch <= kStructMaxBatch, DZO_ERR_UNSUPPORTED, "batch = %lld: the match matrix is batch^2 bits, up to %lld instances", (long long)batch,
                (long long)kStructMaxBatch);
    DZO_TRY(require_same_backend("dzo_structure_batch_classify", "include/dzo.h", fingerprints_dev, "fingerprints", labels_dev, "labels"));
    Context &c = ctx();
    const int B = (int)batch, words = (B + 63) / 64;
    void *ws = nullptr;
    const size_t matrix_bytes = (size_t)B * words * sizeof(unsigned long long);
    DZO_TRY(device_alloc(&ws, matrix_bytes + 16, "the match matrix of the structure classifier", false));
    unsigned long long *bits = (unsigned long long *)ws;
    int32_t *count_dev = (int32_t *)((char *)ws + matrix_bytes);
    int32_t rc = [&]() -> int32_t {
        {
            DZO_TIMED("structure_compare", c.stream);
            DZO_DISPATCH(dtype, sf_launch_cmp<T>(c.stream, length, B, words, tol, fingerprints_dev, bits));
            DZO_HIP(hipGetLastError());
        }
        {
            DZO_TIMED("structure_label", c.stream);
            hipLaunchKernelGGL(structlabel_kernel, dim3(1), dim3(64), 0, c.stream, B, words, (const unsigned long long *)bits, labels_dev, count_dev);
            DZO_HIP(hipGetLastError());
        }
        return copy_blocking(n_classes, count_dev, sizeof(int32_t), hipMemcpyDeviceToHost);
    }();
    (void)hipFree(ws);
    return rc;
}

}  // extern "C"
