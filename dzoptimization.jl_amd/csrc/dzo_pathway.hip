// dzo_pathway.hip -- the transition-state candidates of MANY elastic bands on gfx950: dzo_pathway_batch_candidates.  The connect
// cycle of Carr, Trygubenko & Wales 2005 does not wait for a band to converge: every local maximum of its energy profile is a
// candidate, with the band's tangent there as the first mode of the refinement.  This unit takes the candidates out of a batch
// of bands and compacts them, band-major, into arrays a refinement handle can start from.  include/dzo.h, "Transition-state
// candidates of many bands", states the rule operation by operation (tests/pathway_twin.py replays it on the CPU).
//
// Three launches on one stream, one host wait at the end (for the count):
//   1. pathcand_count_kernel: one thread per band, the number of its candidates from its energies alone;
//   2. pathcand_scan_kernel: ONE 256-thread block turns the counts into exclusive offsets in place, thread t taking the bands
//      t per .. (t + 1) per - 1 with per = ceil(batch / 256), so that any batch up to DZO_PATHWAY_MAX_BATCH is one pass;
//   3. pathcand_wave_kernel (N <= 64) / pathcand_block_kernel (65 <= N <= 1024): one 256-thread block per band forms the tangents
//      of its candidates and writes its slice.  WAVE: candidate k of the band goes to wave k % 4, lane i holds particle i.
//      BLOCK: the block takes the candidates one after another, thread t owns particles t, t + 256, ...
// The tangent is item 2 of the band rule restated against the shared helpers, with the sums of dzo_neb.hip for the same N
// (cl_dot3 per particle, wave_sum_all, cl_block_sum): bit for bit the tangent dzo_neb_batch_apply records for that image.
// Integer counts only in launches 1 and 2: nothing there depends on an order.  No read-modify-write on memory, one writer per element, every loop
// bounded by an argument; the control flow around the barriers of launch 3 is block-uniform (taken from energies every thread
// reads from LDS behind a barrier).
#include "dzo_cluster.h"

namespace dzo {

static_assert(DZO_PATHWAY_MAX_PARTICLES == kClMaxN, "the argument checks of dzo_cluster.h state the particle bound");
static_assert(DZO_PATHWAY_MAX_IMAGES == DZO_NEB_MAX_IMAGES, "a band of the elastic-band unit is a band here");
// the count is an int32: at most (M - 1) / 2 candidates per band
static_assert((int64_t)DZO_PATHWAY_MAX_BATCH * ((DZO_PATHWAY_MAX_IMAGES - 1) / 2) < ((int64_t)1 << 31), "offsets are int32");

// interior image m is a candidate: plain comparisons in T, so a plateau yields its first image and a NaN yields nothing
template <typename T> __device__ __forceinline__ bool pathcand_is(T El, T Em, T Er) { return Em > El && Em >= Er; }

template <typename T> struct PathcandArgs {
    int N, M;
    int64_t capacity;
    const T *band;             // (3N, M batch)
    const T *E;                // (M, batch)
    const int32_t *offsets;    // (batch + 1), exclusive
    T *points, *tangents;      // (3N, capacity)
    T *energies;               // (capacity)
    int32_t *band_index, *image_index;   // (capacity)
};

// ------------------------------------------------------------------------------ 1: counts, one thread per band
template <typename T> __global__ __launch_bounds__(kBlock) void pathcand_count_kernel(int M, int64_t batch, const T *E, int32_t *counts) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= batch) return;
    const T *e = E + (int64_t)M * b;
    int32_t c = 0;
    T El = e[0], Em = e[1];
    for (int m = 1; m < M - 1; ++m) {
        const T Er = e[m + 1];
        c += pathcand_is(El, Em, Er) ? 1 : 0;
        El = Em;
        Em = Er;
    }
    counts[b] = c;
}

// ------------------------------------------------------------------------------ 2: exclusive scan in place, ONE block
// v[0 .. batch) holds the counts and receives the offsets, v[batch] the total
__global__ __launch_bounds__(kBlock) void pathcand_scan_kernel(int64_t batch, int32_t *v) {
    __shared__ int32_t part[kBlock];
    const int tid = threadIdx.x;
    const int64_t per = (batch + kBlock - 1) / kBlock;
    const int64_t lo = per * tid < batch ? per * tid : batch;
    const int64_t hi = lo + per < batch ? lo + per : batch;
    int32_t own = 0;
    for (int64_t i = lo; i < hi; ++i) own += v[i];
    part[tid] = own;
    __syncthreads();
    // Hillis-Steele over the 256 run sums: eight rounds, a read and a write phase each
    for (int d = 1; d < kBlock; d <<= 1) {
        const int32_t left = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += left;
        __syncthreads();
    }
    int32_t run = part[tid] - own;                           // what lies before the thread's first band
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t c = v[i];
        v[i] = run;
        run += c;
    }
    if (tid == kBlock - 1) v[batch] = part[tid];
}

// ------------------------------------------------------------------------------ 3: tangents and the band's slice
template <typename T, bool BLOCK> __device__ __forceinline__ void pathcand_run(const PathcandArgs<T> &a, double *red, T *Es) {
    constexpr int PER = BLOCK ? kClPer : 1;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, wv = tid >> 6;
    const int own = BLOCK ? tid : (tid & 63);                // first particle of the thread
    const int N = a.N, n = 3 * N, M = a.M;
    const T *X = a.band + (int64_t)n * M * b;
    int par = 0;

    if (tid < M) Es[tid] = a.E[(int64_t)M * b + tid];
    __syncthreads();

    bool live[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) live[q] = own + kBlock * q < N;

    // a sum over the particles of one image in every thread that works on it, in the order of the sums (dzo_neb.hip)
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

    const int64_t first = a.offsets[b];
    int k = 0;                                               // candidates of the band so far: the same in every thread
    for (int m = 1; m < M - 1; ++m) {
        const T El = Es[m - 1], Em = Es[m], Er = Es[m + 1];
        if (!pathcand_is(El, Em, Er)) continue;
        const int64_t o = first + k;
        const bool mine = BLOCK || (k % kWaves) == wv;
        k += 1;
        if (o >= a.capacity) break;                          // nothing beyond the capacity is written
        if (!mine) continue;                                 // WAVE: another wave's candidate (no barrier below in that shape)

        // item 2 of the band rule.  E neither rises nor falls through a candidate (Em > El and Em >= Er exclude both), so of
        // the rule's three cases only the energy-weighted mix can occur: t = wp d+ + wm d-
        const T ar = cl_abs(Er - Em), al = cl_abs(El - Em);
        const T hiw = ar > al ? ar : al, low = ar > al ? al : ar;
        const T wp = Er > El ? hiw : low, wm = Er > El ? low : hiw;
        T x[3][PER], dp[3][PER], dn[3][PER], t[3][PER];
        load(X + (size_t)m * n, x);
        load(X + (size_t)(m + 1) * n, dp);
        load(X + (size_t)(m - 1) * n, dn);
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c][q] = dp[c][q] - x[c][q];
                dn[c][q] = x[c][q] - dn[c][q];
                t[c][q] = dfma<T>(wp, dp[c][q], wm * dn[c][q]);
            }
        const double tn = __builtin_sqrt(dot(t, t));
#pragma unroll
        for (int q = 0; q < PER; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c][q] = (T)((double)t[c][q] / tn);
        store(a.points + o * n, x);
        store(a.tangents + o * n, t);
        if (own == 0) {
            a.energies[o] = Em;
            a.band_index[o] = (int32_t)b;
            a.image_index[o] = m;
        }
    }
}

// grid batch, block 256
template <typename T> __global__ __launch_bounds__(kBlock) void pathcand_wave_kernel(PathcandArgs<T> a) {
    __shared__ double red[2 * kWaves];
    __shared__ T Es[DZO_PATHWAY_MAX_IMAGES];
    pathcand_run<T, false>(a, red, Es);
}
template <typename T> __global__ __launch_bounds__(kBlock) void pathcand_block_kernel(PathcandArgs<T> a) {
    __shared__ double red[2 * kWaves];
    __shared__ T Es[DZO_PATHWAY_MAX_IMAGES];
    pathcand_run<T, true>(a, red, Es);
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_pathway_batch_candidates(int64_t n_particles, int32_t n_images, int64_t batch, int32_t dtype, const void *band_dev,
                                     const void *energies_dev, int64_t capacity, void *points_dev, void *tangents_dev,
                                     void *candidate_energies_dev, int32_t *band_index_dev, int32_t *image_index_dev, int32_t *offsets_dev,
                                     int64_t *count) {
    DZO_TRY(require_init());
    DZO_REQUIRE(band_dev && energies_dev && offsets_dev && count, DZO_ERR_INVALID, "null argument");
    *count = 0;
    DZO_TRY(cl_check_args(DZO_RADIAL_LENNARD_JONES, n_particles, batch, dtype));
    DZO_REQUIRE(n_images >= 3 && n_images <= DZO_PATHWAY_MAX_IMAGES, DZO_ERR_INVALID,
                "n_images must be in 3 .. %d (got %d): two ends and at least one image between them", DZO_PATHWAY_MAX_IMAGES, n_images);
    DZO_REQUIRE(batch <= DZO_PATHWAY_MAX_BATCH, DZO_ERR_UNSUPPORTED, "batch must not exceed DZO_PATHWAY_MAX_BATCH = %d (got %lld)",
                DZO_PATHWAY_MAX_BATCH, (long long)batch);
    DZO_REQUIRE(capacity >= 0, DZO_ERR_INVALID, "capacity must not be negative (got %lld)", (long long)capacity);
    DZO_REQUIRE(capacity == 0 || (points_dev && tangents_dev && candidate_energies_dev && band_index_dev && image_index_dev), DZO_ERR_INVALID,
                "null argument: only a call with capacity 0 may leave the candidate arrays out");
    const char *where = "dzo_pathway_batch_candidates", *cite = "every array of a call lives on one device";
    DZO_TRY(require_same_backend(where, cite, band_dev, "band", energies_dev, "energies"));
    DZO_TRY(require_same_backend(where, cite, points_dev, "points", tangents_dev, "tangents"));
    DZO_TRY(require_same_backend(where, cite, candidate_energies_dev, "candidate_energies", band_index_dev, "band_index"));
    DZO_TRY(require_same_backend(where, cite, image_index_dev, "image_index", offsets_dev, "offsets"));
    Context &c = ctx();
    int32_t *total = (int32_t *)c.host_scalar;               // pinned
    {
        DZO_TIMED("pathway_candidates", c.stream);
        DZO_DISPATCH(dtype, hipLaunchKernelGGL((pathcand_count_kernel<T>), dim3((unsigned)((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, c.stream,
                                               (int)n_images, batch, (const T *)energies_dev, offsets_dev));
        hipLaunchKernelGGL(pathcand_scan_kernel, dim3(1), dim3(kBlock), 0, c.stream, batch, offsets_dev);
        DZO_DISPATCH(dtype, PathcandArgs<T> a{};
                     a.N = (int)n_particles; a.M = n_images; a.capacity = capacity; a.band = (const T *)band_dev; a.E = (const T *)energies_dev;
                     a.offsets = offsets_dev; a.points = (T *)points_dev; a.tangents = (T *)tangents_dev; a.energies = (T *)candidate_energies_dev;
                     a.band_index = band_index_dev; a.image_index = image_index_dev;
                     if (capacity > 0) {
                         if (n_particles <= 64) hipLaunchKernelGGL((pathcand_wave_kernel<T>), dim3((unsigned)batch), dim3(kBlock), 0, c.stream, a);
                         else hipLaunchKernelGGL((pathcand_block_kernel<T>), dim3((unsigned)batch), dim3(kBlock), 0, c.stream, a);
                     });
        DZO_HIP(hipGetLastError());
        DZO_HIP(hipMemcpyAsync(total, offsets_dev + batch, sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    *count = *total;
    DZO_REQUIRE(*count <= capacity, DZO_PATHWAY_OVERFLOW,
                "%lld candidates do not fit a capacity of %lld: the first %lld were written, offsets and the count are complete",
                (long long)*count, (long long)capacity, (long long)capacity);
    return DZO_OK;
}

}  // extern "C"
