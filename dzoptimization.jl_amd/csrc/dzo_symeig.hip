// dzo_symeig.hip -- eigenvalues and eigenvectors of MANY small symmetric matrices on gfx950: the dense Hessians that
// dzo_pairwise_batch_hessian leaves on the device, diagonalised where they are.  Two-sided cyclic Jacobi in a round-robin
// ordering; include/dzo.h states the arithmetic operation by operation (tests/symeig_twin.py replays it on the CPU).
//
// One 256-thread block per instance, one kernel body, two storages (dzo_symeig_plan.h decides):
//
//   * LDS storage: the matrix lives in dynamic LDS for the whole iteration, n columns of ld elements, ld odd.  An fp64
//     114 x 114 matrix (N = 38) is 102 KiB of the CU's 160: one block per CU, the matrix is read from memory once.
//   * MEMORY storage (above that, up to DZO_SYMEIG_MAX_N): the same body on a per-call workspace copy in device memory, which
//     stays in L2.  Functional, not fast: the row phase is a strided walk.
//
// A round rotates m / 2 disjoint pairs (p, q).  Work is dealt by pair to the four waves (pair k to wave k % 4: p, q, c and s
// are wave-uniform) and by row or column to the lanes.  In the column phase the lanes walk down two columns (stride 1); in the
// row phase along two rows (stride ld: conflict-free for odd ld).  A wave works out the angles of its own pairs at the head of
// its column phase, a pair per lane, and rotates eight pairs at a time, all loads ahead of the first store and no branch between
// them: with one wave per SIMD nothing else hides the latency of the storage.  The pairs of a round are disjoint, so every
// element has one writer per phase: two barriers per round, no atomics.  V is updated in the output array, with the column phase.
#include "dzo_chain.h"
#include "dzo_common.h"
#include "dzo_symeig_plan.h"

namespace dzo {

template <typename T> struct SymeigArgs {
    int n, ld, max_sweeps;
    const T *A;                // (n, n, batch), column-major per instance; read only
    T *work;                   // MEMORY storage: (n, n, batch), the iterated copies; null on LDS storage
    T *w;                      // (n, batch) eigenvalues
    T *V;                      // (n, n, batch) eigenvectors, or null
    int32_t *sweeps;           // (batch), or null
};

template <typename T> struct SymeigEps;
template <> struct SymeigEps<double> { static constexpr double value = 2.220446049250313e-16; };   // 2^-52
template <> struct SymeigEps<float> { static constexpr double value = 1.1920928955078125e-07; };   // 2^-23

template <typename T> __device__ __forceinline__ T se_sqrt(T x);
template <> __device__ __forceinline__ double se_sqrt<double>(double x) { return __builtin_sqrt(x); }
template <> __device__ __forceinline__ float se_sqrt<float>(float x) { return __builtin_sqrtf(x); }
template <typename T> __device__ __forceinline__ T se_abs(T x);
template <> __device__ __forceinline__ double se_abs<double>(double x) { return __builtin_fabs(x); }
template <> __device__ __forceinline__ float se_abs<float>(float x) { return __builtin_fabsf(x); }
template <typename T> __device__ __forceinline__ T se_copysign(T x, T y);
template <> __device__ __forceinline__ double se_copysign<double>(double x, double y) { return __builtin_copysign(x, y); }
template <> __device__ __forceinline__ float se_copysign<float>(float x, float y) { return __builtin_copysignf(x, y); }

// a block-wide fp64 sum, the same bits in every thread: wave trees, then the four wave sums in wave order from +0
__device__ __forceinline__ double se_block_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_sum_all(v);
    if (lane == 0) red[wv] = v;
    __syncthreads();
    double r = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) r += red[k];
    __syncthreads();                                         // red is used again
    return r;
}

// position j of the round-robin list in round `round` of a sweep (0 .. m - 2): position 0 stays, the others turn by one per round
__device__ __forceinline__ int se_list(int j, int round, int m) {
    if (j == 0) return 0;
    int v = j - 1 - round;
    if (v < 0) v += m - 1;
    return 1 + v;
}
// pair k of a round: p < q; q == n is the padding of an odd n, the pair is dropped
__device__ __forceinline__ void se_pair(int k, int round, int m, int &p, int &q) {
    const int i = se_list(k, round, m), j = se_list(m - 1 - k, round, m);
    p = i < j ? i : j;
    q = i < j ? j : i;
}

// A wave rotates its pairs kSymeigGroup at a time: the pairs of a round are disjoint, so the loads of a whole group are issued
// before its first store, and a group costs one round trip to the storage per 64 elements of a line instead of one per pair.
constexpr int kSymeigGroup = 8;
template <typename T> struct SePairs {
    int p[kSymeigGroup], q[kSymeigGroup];                    // wave-uniform; p = q = 0 where on[j] is not set
    bool on[kSymeigGroup];                                   // the pair exists and is not the dropped one
    T c[kSymeigGroup], s[kSymeigGroup];                      // the same in every lane, as LDS broadcasts leave them
};

// the pairs k0, k0 + 4, ... of a wave's group in this round, with their angles from `cs`
template <typename T> __device__ __forceinline__ void se_group_pairs(SePairs<T> &g, const T *cs, int k0, int round, int m, int n) {
#pragma unroll
    for (int j = 0; j < kSymeigGroup; ++j) {
        const int k = k0 + kWaves * j;
        int p = 0, q = n;
        if (k < (m >> 1)) se_pair(k, round, m, p, q);
        g.on[j] = q < n;
        g.p[j] = g.on[j] ? p : 0; g.q[j] = g.on[j] ? q : 0;
        const int kc = g.on[j] ? k : k0;                     // (a cell that exists, and is this wave's)
        g.c[j] = cs[2 * kc]; g.s[j] = cs[2 * kc + 1];
    }
}

// The plane rotations of a group on its lines of n elements: line i starts at line * i, element e of it is at elem * e, lane l
// takes e = l, l + 64, ...: (x, y) = (line p, line q) becomes (c x - s y, s x + c y).  ZERO (the row phase): element q of line p
// and element p of line q become exact zeros.  The loads are unconditional -- a pair that is not on reads line 0 and stores
// nothing -- because a branch between two loads makes the compiler wait for the first before it issues the second, and sixteen
// round trips in a row were most of a round.
template <typename T, bool ZERO> __device__ __forceinline__ void se_rotate_group(T *a, int line, int elem, int n, int lane, const SePairs<T> &g) {
    for (int e = lane; e < n; e += 64) {
        T x[kSymeigGroup], y[kSymeigGroup];
        const int oe = elem * e;                             // (int offsets from one base pointer)
#pragma unroll
        for (int j = 0; j < kSymeigGroup; ++j) { x[j] = a[oe + line * g.p[j]]; y[j] = a[oe + line * g.q[j]]; }
#pragma unroll
        for (int j = 0; j < kSymeigGroup; ++j)
            if (g.on[j]) {
                const T nx = g.c[j] * x[j] - g.s[j] * y[j], ny = g.s[j] * x[j] + g.c[j] * y[j];
                a[oe + line * g.p[j]] = ZERO && e == g.q[j] ? T(0) : nx;
                a[oe + line * g.q[j]] = ZERO && e == g.p[j] ? T(0) : ny;
            }
    }
}

// grid batch, block 256
template <typename T, int STORAGE> __global__ __launch_bounds__(kBlock) void symeig_jacobi_kernel(SymeigArgs<T> g) {
    extern __shared__ double symeig_lds[];
    double *red = symeig_lds;                                // kSymeigRedBytes
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = g.n, m = n + (n & 1), half = m >> 1;
    const int64_t b = blockIdx.x, nn = (int64_t)n * n;
    T *cs = reinterpret_cast<T *>(symeig_lds + kSymeigRedBytes / 8);   // (c, s) of pair k at 2 k; the ranks at the end
    T *dg = cs + m;                                          // the diagonal, for the rank count
    T *a;
    if constexpr (STORAGE == DZO_SYMEIG_STORAGE_LDS) a = dg + m;
    else a = g.work + nn * b;
    const int ld = g.ld;
    const T *A = g.A + nn * b;
    T *V = g.V ? g.V + nn * b : nullptr;

    // load: the symmetric part, its Frobenius norm, V = I
    double fro2 = 0;
    for (int c = wv; c < n; c += kWaves)
        for (int r = lane; r < n; r += 64) {
            const T v = T(0.5) * (A[r + (int64_t)n * c] + A[c + (int64_t)n * r]);
            a[r + ld * c] = v;
            const double dv = (double)v;
            fro2 += dv * dv;
            if (V) V[r + n * c] = r == c ? T(1) : T(0);
        }
    fro2 = se_block_sum(fro2, red);                          // (its barriers also publish a and V)
    const double threshold = SymeigEps<T>::value * __builtin_sqrt(fro2);

    int sweeps = 0, verdict;
    for (;;) {
        // sweep test: the off-diagonal norm from the off-diagonal entries themselves
        double off2 = 0;
        for (int c = wv; c < n; c += kWaves)
            for (int r = lane; r < n; r += 64) {
                const double dv = (double)a[r + ld * c];
                const double sq = dv * dv;
                off2 += r == c ? 0.0 : sq;
            }
        off2 = se_block_sum(off2, red);
        if (__builtin_sqrt(off2) <= threshold && threshold < __builtin_inf()) { verdict = sweeps; break; }   // the same in every thread
        if (sweeps == g.max_sweeps) { verdict = -1; break; }
        for (int round = 0; round < m - 1; ++round) {
            // columns, all rows; V with them.  A wave takes the angles of its own pairs first, from the matrix as it stands at
            // the start of the round: a_pq, a_pp and a_qq sit in columns p and q, which no other wave writes in this phase, and
            // which this wave has not written yet.  Lane l works out pair wv + 4 l: one pass serves the wave's 48 pairs at most.
            static_assert(DZO_SYMEIG_MAX_N / 2 <= 64 * kWaves, "one angle pass per wave and round");
            {
                const int kl = wv + kWaves * lane;
                if (kl < half) {
                    int p, q;
                    se_pair(kl, round, m, p, q);
                    T c = T(1), s = T(0);
                    if (q < n) {
                        const T apq = a[p + ld * q], app = a[p + ld * p], aqq = a[q + ld * q];
                        const T tau = (aqq - app) / (apq + apq);
                        const T t = se_copysign(T(1), tau) / (se_abs(tau) + se_sqrt(T(1) + tau * tau));
                        const T cc = T(1) / se_sqrt(T(1) + t * t);
                        const T ss = t * cc;
                        c = apq == T(0) ? T(1) : cc;
                        s = apq == T(0) ? T(0) : ss;
                    }
                    cs[2 * kl] = c; cs[2 * kl + 1] = s;
                }
                // the angles reach every lane through LDS: the wave's own stores, read back by the wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            for (int k0 = wv; k0 < half; k0 += kWaves * kSymeigGroup) {
                SePairs<T> grp;
                se_group_pairs(grp, cs, k0, round, m, n);
                se_rotate_group<T, false>(a, ld, 1, n, lane, grp);
                if (V) se_rotate_group<T, false>(V, n, 1, n, lane, grp);
            }
            __syncthreads();
            // rows, all columns; the rotated element is zero exactly
            for (int k0 = wv; k0 < half; k0 += kWaves * kSymeigGroup) {
                SePairs<T> grp;
                se_group_pairs(grp, cs, k0, round, m, n);
                se_rotate_group<T, true>(a, 1, ld, n, lane, grp);
            }
            __syncthreads();
        }
        ++sweeps;
    }

    // finish: the diagonal, ascending and stable by a rank count
    int *rank = reinterpret_cast<int *>(cs);
    for (int k = tid; k < n; k += kBlock) dg[k] = a[k + ld * k];
    __syncthreads();
    T *w = g.w + (int64_t)n * b;
    for (int k = tid; k < n; k += kBlock) {
        const T dk = dg[k];
        int rk = 0;
        for (int j = 0; j < n; ++j) {
            const T dj = dg[j];
            rk += (dj < dk || (dj == dk && j < k)) ? 1 : 0;
        }
        w[rk] = dk;                                          // 0 <= rk <= n - 1 whatever the values (NaN: ranks may coincide)
        rank[k] = rk;
    }
    if (tid == 0 && g.sweeps) g.sweeps[b] = verdict;
    if (!V) return;                                          // the same in every thread
    __syncthreads();
    // the columns of V follow their eigenvalues, through the storage the matrix no longer needs
    for (int c = wv; c < n; c += kWaves)
        for (int r = lane; r < n; r += 64) a[r + ld * c] = V[r + n * c];
    __syncthreads();
    for (int c = wv; c < n; c += kWaves) {
        T *dst = V + n * rank[c];
        for (int r = lane; r < n; r += 64) dst[r] = a[r + ld * c];
    }
}

template <typename T> static const void *se_kernel(int32_t storage) {
    return storage == DZO_SYMEIG_STORAGE_LDS ? (const void *)symeig_jacobi_kernel<T, DZO_SYMEIG_STORAGE_LDS>
                                             : (const void *)symeig_jacobi_kernel<T, DZO_SYMEIG_STORAGE_MEMORY>;
}

template <typename T> static void se_launch(hipStream_t s, int64_t batch, const SymeigPlan &plan, const SymeigArgs<T> &a) {
    if (plan.storage == DZO_SYMEIG_STORAGE_LDS)
        hipLaunchKernelGGL((symeig_jacobi_kernel<T, DZO_SYMEIG_STORAGE_LDS>), dim3((unsigned)batch), dim3(kBlock), (size_t)plan.lds_bytes, s, a);
    else
        hipLaunchKernelGGL((symeig_jacobi_kernel<T, DZO_SYMEIG_STORAGE_MEMORY>), dim3((unsigned)batch), dim3(kBlock), (size_t)plan.lds_bytes, s, a);
}

static int32_t se_check_size(int64_t n, int32_t dtype) {
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(n >= 1, DZO_ERR_INVALID, "n must be at least 1 (got %lld)", (long long)n);
    DZO_REQUIRE(n <= DZO_SYMEIG_MAX_N, DZO_ERR_UNSUPPORTED, "n = %lld: one block iterates on an instance, up to n = %d", (long long)n,
                DZO_SYMEIG_MAX_N);
    return DZO_OK;
}

// dzo_chain.h: raises the LDS attribute of the kernel this (n, dtype) launches; once per handle, no launch
int32_t se_prepare(int64_t n, int32_t dtype) {
    const SymeigPlan plan = symeig_plan(n, dtype);
    if (plan.lds_bytes > 48 * 1024)
        DZO_HIP(hipFuncSetAttribute(dtype == DZO_F64 ? se_kernel<double>(plan.storage) : se_kernel<float>(plan.storage),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSymeigLdsLimit));
    return DZO_OK;
}

// dzo_chain.h: the launch of dzo_symmetric_batch_eigen on `s`, checked arguments, no wait
int32_t se_enqueue(hipStream_t s, int64_t n, int64_t batch, int32_t dtype, const void *matrices, void *work, void *eigenvalues, void *eigenvectors,
                   int32_t *sweeps, int32_t max_sweeps) {
    const SymeigPlan plan = symeig_plan(n, dtype);
    const int limit = max_sweeps <= 0 ? DZO_SYMEIG_DEFAULT_SWEEPS : max_sweeps;
    DZO_DISPATCH(dtype, se_launch<T>(s, batch, plan, SymeigArgs<T>{(int)n, (int)plan.ld, limit, (const T *)matrices, (T *)work, (T *)eigenvalues,
                                                                  (T *)eigenvectors, sweeps}));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_symeig_plan(int64_t n, int32_t dtype, int32_t *storage, int64_t *ld, int64_t *lds_bytes) {
    DZO_TRY(se_check_size(n, dtype));
    const SymeigPlan plan = symeig_plan(n, dtype);
    if (storage) *storage = plan.storage;
    if (ld) *ld = plan.ld;
    if (lds_bytes) *lds_bytes = plan.lds_bytes;
    return DZO_OK;
}

int32_t dzo_symmetric_batch_eigen(int64_t n, int64_t batch, int32_t dtype, const void *matrices_dev, void *eigenvalues_dev,
                                  void *eigenvectors_dev, int32_t *sweeps_dev, int32_t max_sweeps) {
    DZO_TRY(require_init());
    DZO_REQUIRE(matrices_dev && eigenvalues_dev, DZO_ERR_INVALID, "null argument");
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(n >= 1, DZO_ERR_INVALID, "n must be at least 1 (got %lld)", (long long)n);
    DZO_REQUIRE(batch >= 1 && batch <= ((int64_t)1 << 30), DZO_ERR_INVALID, "batch must be in 1 .. 2^30 (got %lld)", (long long)batch);
    DZO_TRY(se_check_size(n, dtype));
    const char *where = "dzo_symmetric_batch_eigen", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, matrices_dev, "matrices", eigenvalues_dev, "eigenvalues"));
    DZO_TRY(require_same_backend(where, cite, eigenvectors_dev, "eigenvectors", sweeps_dev, "sweeps"));
    Context &c = ctx();
    const SymeigPlan plan = symeig_plan(n, dtype);
    void *work = nullptr;
    if (plan.storage == DZO_SYMEIG_STORAGE_MEMORY) {
        const size_t bytes = (size_t)n * (size_t)n * (size_t)batch * dtype_size(dtype);
        const hipError_t e = hipMalloc(&work, bytes);
        if (e == hipErrorOutOfMemory) {
            set_error("dzo_symmetric_batch_eigen: out of device memory for the workspace (%zu bytes)", bytes);
            (void)hipGetLastError();
            return DZO_ERR_NOMEM;
        }
        DZO_HIP(e);
    }
    hipError_t e = hipSuccess;
    if (plan.lds_bytes > 48 * 1024) {
        // gfx950 has 160 KiB of LDS per CU; dynamic requests above the default need the attribute.  It belongs to the kernel:
        // raised to the limit, so that no later call lowers it
        e = hipFuncSetAttribute(dtype == DZO_F64 ? se_kernel<double>(plan.storage) : se_kernel<float>(plan.storage),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSymeigLdsLimit);
    }
    if (e == hipSuccess) {
        DZO_TIMED("symeig", c.stream);
        const int sweeps = max_sweeps <= 0 ? DZO_SYMEIG_DEFAULT_SWEEPS : max_sweeps;
        if (dtype == DZO_F64)
            se_launch<double>(c.stream, batch, plan, SymeigArgs<double>{(int)n, (int)plan.ld, sweeps, (const double *)matrices_dev, (double *)work,
                                                                       (double *)eigenvalues_dev, (double *)eigenvectors_dev, sweeps_dev});
        else
            se_launch<float>(c.stream, batch, plan, SymeigArgs<float>{(int)n, (int)plan.ld, sweeps, (const float *)matrices_dev, (float *)work,
                                                                     (float *)eigenvalues_dev, (float *)eigenvectors_dev, sweeps_dev});
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (work) (void)hipFree(work);
    DZO_HIP(e);
    return DZO_OK;
}

}  // extern "C"
