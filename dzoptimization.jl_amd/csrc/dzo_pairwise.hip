// dzo_pairwise.hip -- the pairwise radial (Lennard-Jones) N-body objective of src/ExampleFunctions.jl on gfx950.
//
// The reference's three KernelAbstractions kernels (:117-149, :224-262, :367-424) run one thread per particle with a
// global-memory loop over j.  Here the same per-pair arithmetic (same operations, same order, every muladd an explicit
// fma, the reciprocal a correctly rounded 1 / r2, the self term removed by a select) runs in two launch shapes:
//
//   * TILE (large N): one thread per particle i with its accumulators in registers; the j coordinates come through LDS in
//     tiles of 256 (every lane of a wave reads the same address: a broadcast, no bank conflict), so the inner loop holds no
//     global load.  While ceil(N / 256) blocks would leave CUs idle the j tiles are split over gridDim.y; every (row,
//     split) partial goes to a workspace and a finish kernel adds the splits of a row in split order.
//   * WAVE (small N): one WAVE per particle, lane l takes j = l, l + 64, ...; the 64 lane sums are added by the fixed
//     DPP / permlane tree of dzo_common.h (wave_sum_all).  N = 38 (the reference's own workload) then fills 38 waves
//     instead of 38 lanes.
//
// Sums over j are in a fixed order that depends only on N and the device's CU count; there is no floating-point atomic
// anywhere, so the same input gives the same bits on every call.  Lane accumulators are in T like the reference's;
// sums ACROSS lanes / blocks are taken in fp64 (exact for fp32 terms of like magnitude, and one rounding back to T).
// Nothing here assumes that y or z are 16-byte aligned: every global access is a plain element load.
#include "dzo_pairwise.h"

#include <cstdlib>

namespace dzo {

// ------------------------------------------------------------------------------ TILE shape
// grid (ceil(N / 256), js).  Block (bx, by) owns rows 256 bx ... and the j tiles [tiles by / js, tiles (by + 1) / js).
// js == 1: the rows' results go straight to o0..o2 (twice(a), :258-260); js > 1: to part[(by * 3 + c) * N + i].
// Energy: the block's rows are summed (fp64) into epart[by * gridDim.x + bx].
template <typename T, typename F, int MODE>
__global__ __launch_bounds__(kBlock) void pairwise_tile_kernel(int64_t N, int tiles, const T *__restrict__ x, const T *__restrict__ y,
                                                               const T *__restrict__ z, const T *__restrict__ u, const T *__restrict__ v,
                                                               const T *__restrict__ w, T *__restrict__ o0, T *__restrict__ o1,
                                                               T *__restrict__ o2, T *__restrict__ part, double *__restrict__ epart) {
    constexpr int C = MODE == kPwHvp ? 6 : 3;
    __shared__ T tile[C][kBlock];
    __shared__ double red[kWaves];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
    const bool live = i < N;
    PwPoint<T> pi = {T(0), T(0), T(0), T(0), T(0), T(0)};
    if (live) {
        pi.x = x[i]; pi.y = y[i]; pi.z = z[i];
        if constexpr (MODE == kPwHvp) { pi.u = u[i]; pi.v = v[i]; pi.w = w[i]; }
    }
    const int js = (int)gridDim.y, by = (int)blockIdx.y;
    const int t0 = (int)((int64_t)tiles * by / js), t1 = (int)((int64_t)tiles * (by + 1) / js);
    T ax = T(0), ay = T(0), az = T(0);
    for (int t = t0; t < t1; ++t) {
        const int64_t j0 = (int64_t)t * kBlock;
        const int64_t jl = j0 + tid;
        __syncthreads();                                     // the previous tile has been consumed
        const bool in = jl < N;
        tile[0][tid] = in ? x[jl] : T(0);
        tile[1][tid] = in ? y[jl] : T(0);
        tile[2][tid] = in ? z[jl] : T(0);
        if constexpr (MODE == kPwHvp) {
            tile[3][tid] = in ? u[jl] : T(0);
            tile[4][tid] = in ? v[jl] : T(0);
            tile[5][tid] = in ? w[jl] : T(0);
        }
        __syncthreads();
        const int cnt = (int)(N - j0 < (int64_t)kBlock ? N - j0 : (int64_t)kBlock);   // the last tile may be partial
        const int64_t sd = i - j0;
        const int self = (sd >= 0 && sd < kBlock) ? (int)sd : -1;
        // four independent pairs per trip (kBlock is a multiple of 4); the padding of a partial tile (zeros in LDS) that a
        // trip reaches is removed by the same select as the self term
        for (int j4 = 0; j4 < cnt; j4 += 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int jj = j4 + k;
                PwPoint<T> pj;
                pj.x = tile[0][jj]; pj.y = tile[1][jj]; pj.z = tile[2][jj];
                if constexpr (MODE == kPwHvp) { pj.u = tile[3][jj]; pj.v = tile[4][jj]; pj.w = tile[5][jj]; }
                else { pj.u = pj.v = pj.w = T(0); }
                pw_pair<T, F, MODE>(jj == self || jj >= cnt, pi, pj, ax, ay, az);
            }
        }
    }
    if constexpr (MODE == kPwEnergy) {
        const double r = block_sum(live ? (double)ax : 0.0, red);
        if (tid == 0) epart[(int64_t)by * gridDim.x + blockIdx.x] = r;
    } else {
        if (live) {
            if (js == 1) {
                o0[i] = pw_twice(ax); o1[i] = pw_twice(ay); o2[i] = pw_twice(az);
            } else {
                part[((int64_t)by * 3 + 0) * N + i] = ax;
                part[((int64_t)by * 3 + 1) * N + i] = ay;
                part[((int64_t)by * 3 + 2) * N + i] = az;
            }
        }
    }
}

// rows of a split j range: o_c[i] = twice(sum_s part[(s * 3 + c) * N + i]), splits added in split order
template <typename T>
__global__ __launch_bounds__(kBlock) void pairwise_finish_rows_kernel(int64_t N, int js, const T *__restrict__ part, T *__restrict__ o0,
                                                                      T *__restrict__ o1, T *__restrict__ o2) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    T a0 = T(0), a1 = T(0), a2 = T(0);
    for (int s = 0; s < js; ++s) {
        a0 += part[((int64_t)s * 3 + 0) * N + i];
        a1 += part[((int64_t)s * 3 + 1) * N + i];
        a2 += part[((int64_t)s * 3 + 2) * N + i];
    }
    o0[i] = pw_twice(a0); o1[i] = pw_twice(a1); o2[i] = pw_twice(a2);
}

// E = 1/2 sum of `count` fp64 partials (rows or blocks), one block, fixed order (_half * energy, :147, taken once:
// halving is exact)
__global__ __launch_bounds__(kBlock) void pairwise_finish_energy_kernel(const double *__restrict__ partials, int64_t count,
                                                                        double *__restrict__ result) {
    __shared__ double lds[kWaves];
    double v = 0;
    for (int64_t k = threadIdx.x; k < count; k += kBlock) v += partials[k];
    const double r = block_sum(v, lds);
    if (threadIdx.x == 0) result[0] = 0.5 * r;
}

// ------------------------------------------------------------------------------ WAVE shape
// grid ceil(N / 4): wave `wv` of block b owns particle i = 4 b + wv, lane l the terms j = l, l + 64, ...
template <typename T, typename F, int MODE>
__global__ __launch_bounds__(kBlock) void pairwise_wave_kernel(int64_t N, const T *__restrict__ x, const T *__restrict__ y,
                                                               const T *__restrict__ z, const T *__restrict__ u, const T *__restrict__ v,
                                                               const T *__restrict__ w, T *__restrict__ o0, T *__restrict__ o1,
                                                               T *__restrict__ o2, double *__restrict__ erow) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kWaves + wv;
    if (i >= N) return;                                      // a whole wave leaves; no barrier in this kernel
    PwPoint<T> pi = {x[i], y[i], z[i], T(0), T(0), T(0)};
    if constexpr (MODE == kPwHvp) { pi.u = u[i]; pi.v = v[i]; pi.w = w[i]; }
    T ax = T(0), ay = T(0), az = T(0);
    for (int64_t j = lane; j < N; j += 64) {
        PwPoint<T> pj = {x[j], y[j], z[j], T(0), T(0), T(0)};
        if constexpr (MODE == kPwHvp) { pj.u = u[j]; pj.v = v[j]; pj.w = w[j]; }
        pw_pair<T, F, MODE>(j == i, pi, pj, ax, ay, az);
    }
    // all 64 lanes are here again (lanes without a j hold zeros)
    const double sx = wave_sum_all((double)ax);
    if constexpr (MODE == kPwEnergy) {
        if (lane == 0) erow[i] = sx;
    } else {
        const double sy = wave_sum_all((double)ay);
        const double sz = wave_sum_all((double)az);
        if (lane == 0) { o0[i] = pw_twice((T)sx); o1[i] = pw_twice((T)sy); o2[i] = pw_twice((T)sz); }
    }
}

// ------------------------------------------------------------------------------ energy_delta (:477-534)
// one block; thread t takes j = t, t + 256, ...; result[0] = energy_new - energy_old (in T)
template <typename T, typename F>
__global__ __launch_bounds__(kBlock) void pairwise_energy_delta_kernel(int64_t N, const T *__restrict__ x, const T *__restrict__ y,
                                                                       const T *__restrict__ z, int64_t i, T x_new, T y_new, T z_new,
                                                                       double *__restrict__ result) {
    __shared__ double lds[2 * kWaves];
    const T x_old = x[i], y_old = y[i], z_old = z[i];
    T e_old = T(0), e_new = T(0);
    for (int64_t j = threadIdx.x; j < N; j += kBlock) {
        const T xj = x[j], yj = y[j], zj = z[j];
        const bool self = j == i;
        const T eo = pw_pair_energy<T, F>(x_old, y_old, z_old, xj, yj, zj);
        e_old += self ? T(0) : eo;
        const T en = pw_pair_energy<T, F>(x_new, y_new, z_new, xj, yj, zj);
        e_new += self ? T(0) : en;
    }
    const double in[2] = {(double)e_old, (double)e_new};
    double out[2];
    block_sum_multi<2>(in, lds, out);
    if (threadIdx.x == 0) result[0] = (double)((T)out[1] - (T)out[0]);
}

// ------------------------------------------------------------------------------ fma calibration
// register-only: 16 independent chains per lane, a = fma(a, b, c), nothing dependent between the chains
template <typename T>
__global__ __launch_bounds__(kBlock) void calib_fma_kernel(int64_t iters, T b, T c, T *__restrict__ sink) {
    T a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = (T)(threadIdx.x + k) * T(1e-3);
    for (int64_t it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = dfma<T>(a[k], b, c);
    }
    T r = T(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) r += a[k];
    sink[(int64_t)blockIdx.x * kBlock + threadIdx.x] = r;
}

// ------------------------------------------------------------------------------ launch shapes
// Particles up to which the WAVE shape is used.  One wave per particle costs 3 (6 for the hvp) global loads per pair, which the
// caches serve; it stops paying once ceil(N / 256) * js TILE blocks fill the chip by themselves.  DZO_TUNE_PAIRWISE_WAVE_MAX
// overrides the threshold (tools/bench_pairwise.py sweeps it).
static int64_t pw_wave_max() {
    static const int64_t v = tune_int("DZO_TUNE_PAIRWISE_WAVE_MAX", 2048);
    return v;
}
constexpr int kPwMaxSplit = 64;

struct PwShape {
    bool wave = false;
    int64_t iblocks = 0;   // TILE: blocks along i (= tiles along j)
    int js = 1;            // TILE: splits of the j range
};
static PwShape pw_shape(int64_t N) {
    PwShape sh;
    sh.wave = N <= pw_wave_max();
    sh.iblocks = (N + kBlock - 1) / kBlock;
    // Split the j range (a) until there are two blocks per CU and then (b) so that the blocks fill the CUs evenly: all blocks
    // of these grids are resident at once (up to 8 per CU), a CU's time is the number of blocks it was dealt, and 553 blocks
    // on 256 CUs (N = 20000 with the smallest split, 7) leave most CUs waiting for the ones dealt a third block.  Among the
    // splits up to 8 blocks per CU take the one with the best fill = blocks / (cus * ceil(blocks / cus)); the smallest
    // within 2 % of the best, since every split costs a row of partials.
    const int64_t cus = ctx().cus > 0 ? ctx().cus : 1;
    int64_t js = 1;
    if (sh.iblocks < 2 * cus) js = (2 * cus + sh.iblocks - 1) / sh.iblocks;
    int64_t js_max = sh.iblocks < kPwMaxSplit ? sh.iblocks : kPwMaxSplit;   // at least one tile per split
    if (js > js_max) js = js_max;
    if (js < 1) js = 1;
    auto fill = [&](int64_t k) { const int64_t b = sh.iblocks * k; return (double)b / (double)(cus * ((b + cus - 1) / cus)); };
    double best = 0;
    for (int64_t k = js; k <= js_max && sh.iblocks * k <= 8 * cus; ++k) best = fill(k) > best ? fill(k) : best;
    for (int64_t k = js; k <= js_max && sh.iblocks * k <= 8 * cus; ++k)
        if (fill(k) >= 0.98 * best) { js = k; break; }
    sh.js = (int)js;
    return sh;
}

int64_t pairwise_workspace_doubles(int64_t N) {
    const PwShape sh = pw_shape(N);
    const int64_t eparts = sh.iblocks * sh.js > N ? sh.iblocks * sh.js : N;
    return 3 * N * sh.js + eparts + 8;
}

template <typename T, typename F>
static int32_t pw_energy_t(hipStream_t s, int64_t N, const T *x, const T *y, const T *z, double *ws, double *result_dev) {
    const PwShape sh = pw_shape(N);
    const T *nul = nullptr;
    T *nulo = nullptr;
    if (sh.wave) {
        const int64_t grid = (N + kWaves - 1) / kWaves;
        hipLaunchKernelGGL((pairwise_wave_kernel<T, F, kPwEnergy>), dim3((unsigned)grid), dim3(kBlock), 0, s, N, x, y, z, nul, nul, nul, nulo,
                           nulo, nulo, ws);
        hipLaunchKernelGGL(pairwise_finish_energy_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)ws, N, result_dev);
    } else {
        hipLaunchKernelGGL((pairwise_tile_kernel<T, F, kPwEnergy>), dim3((unsigned)sh.iblocks, (unsigned)sh.js), dim3(kBlock), 0, s, N,
                           (int)sh.iblocks, x, y, z, nul, nul, nul, nulo, nulo, nulo, nulo, ws);
        hipLaunchKernelGGL(pairwise_finish_energy_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)ws, sh.iblocks * sh.js, result_dev);
    }
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

template <typename T, typename F, int MODE>
static int32_t pw_rows_t(hipStream_t s, int64_t N, T *o0, T *o1, T *o2, const T *x, const T *y, const T *z, const T *u, const T *v,
                         const T *w, double *ws) {
    const PwShape sh = pw_shape(N);
    double *nule = nullptr;
    if (sh.wave) {
        const int64_t grid = (N + kWaves - 1) / kWaves;
        hipLaunchKernelGGL((pairwise_wave_kernel<T, F, MODE>), dim3((unsigned)grid), dim3(kBlock), 0, s, N, x, y, z, u, v, w, o0, o1, o2, nule);
    } else {
        T *part = reinterpret_cast<T *>(ws);
        hipLaunchKernelGGL((pairwise_tile_kernel<T, F, MODE>), dim3((unsigned)sh.iblocks, (unsigned)sh.js), dim3(kBlock), 0, s, N,
                           (int)sh.iblocks, x, y, z, u, v, w, o0, o1, o2, part, nule);
        if (sh.js > 1)
            hipLaunchKernelGGL(pairwise_finish_rows_kernel<T>, dim3((unsigned)sh.iblocks), dim3(kBlock), 0, s, N, sh.js, (const T *)part, o0, o1, o2);
    }
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

// ------------------------------------------------------------------------------ host helpers (dzo_pairwise.h)
int32_t device_alloc(void **p, size_t bytes, const char *what_for, bool zero_fill) {
    const size_t size = bytes ? bytes : 16;
    hipError_t e = hipMalloc(p, size);
    if (e == hipSuccess && zero_fill) e = hipMemset(*p, 0, size);
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        set_error("out of device memory for %s (%zu bytes)", what_for, bytes);
        return DZO_ERR_NOMEM;
    }
    return DZO_OK;
}

int32_t pw_check_args(int32_t radial, int32_t dtype, int64_t N, int64_t count, const char *count_name, int64_t max_particles, int32_t over_max,
                      const char *holder) {
    DZO_REQUIRE(radial == DZO_RADIAL_LENNARD_JONES || radial == DZO_RADIAL_MORSE_RHO6 || radial == DZO_RADIAL_MORSE_RHO14, DZO_ERR_INVALID,
                "unknown radial function %d (built in: DZO_RADIAL_LENNARD_JONES = 0, DZO_RADIAL_MORSE_RHO6 = 2, DZO_RADIAL_MORSE_RHO14 = 3)", radial);
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(N >= 1, DZO_ERR_INVALID, "n_particles must be at least 1 (got %lld)", (long long)N);
    DZO_REQUIRE(count >= 1 && count <= ((int64_t)1 << 30), DZO_ERR_INVALID, "%s must be in 1 .. 2^30 (got %lld)", count_name, (long long)count);
    DZO_REQUIRE(N <= max_particles, over_max, "n_particles = %lld: %s, up to %lld particles", (long long)N, holder, (long long)max_particles);
    return DZO_OK;
}

int32_t copy_blocking(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    hipStream_t s = ctx().stream;
    DZO_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
    DZO_HIP(hipStreamSynchronize(s));
    return DZO_OK;
}

constexpr int64_t kPwMaxParticles = (int64_t)1 << 28;       // tiles and grids stay far inside int / the grid limits

// one set of particles: the entry points below and the launchers the problem kind calls
static int32_t pw_check_common(int32_t radial, int64_t N, int32_t dtype) {
    return pw_check_args(radial, dtype, N, 1, "the number of particle sets", kPwMaxParticles, DZO_ERR_INVALID, "the launchers index tiles and grids with int");
}

int32_t pairwise_energy_async(hipStream_t s, int32_t radial, int64_t N, int32_t dtype, const void *x, const void *y, const void *z,
                              double *ws, double *result_dev) {
    DZO_TRY(pw_check_common(radial, N, dtype));
    DZO_DISPATCH_RADIAL(radial, dtype, return (pw_energy_t<T, F>(s, N, (const T *)x, (const T *)y, (const T *)z, ws, result_dev)));
    return DZO_OK;
}

int32_t pairwise_gradient_async(hipStream_t s, int32_t radial, int64_t N, int32_t dtype, void *gx, void *gy, void *gz, const void *x,
                                const void *y, const void *z, double *ws) {
    DZO_TRY(pw_check_common(radial, N, dtype));
    DZO_DISPATCH_RADIAL(radial, dtype, return (pw_rows_t<T, F, kPwGradient>(s, N, (T *)gx, (T *)gy, (T *)gz, (const T *)x, (const T *)y, (const T *)z,
                                                                            (const T *)nullptr, (const T *)nullptr, (const T *)nullptr, ws)));
    return DZO_OK;
}

// workspace of the handle-less entry points: grown on demand, kept in the device's context, freed by dzo_shutdown
static int32_t pw_ctx_workspace(int64_t N, double **ws) {
    Context &c = ctx();
    const int64_t need = pairwise_workspace_doubles(N);
    if (c.pair_ws_doubles < need) {
        if (c.pair_ws) { DZO_HIP(hipStreamSynchronize(c.stream)); (void)hipFree(c.pair_ws); c.pair_ws = nullptr; c.pair_ws_doubles = 0; }
        DZO_TRY(device_alloc((void **)&c.pair_ws, sizeof(double) * (size_t)need, "the pairwise workspace", false));
        c.pair_ws_doubles = need;
    }
    *ws = c.pair_ws;
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

// accelerated_pairwise_radial_energy, src/ExampleFunctions.jl:152-173
int32_t dzo_pairwise_energy(int32_t radial, int64_t n_particles, int32_t dtype, const void *x_dev, const void *y_dev, const void *z_dev,
                            double *energy) {
    DZO_TRY(require_init());
    DZO_REQUIRE(x_dev && y_dev && z_dev && energy, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_common(radial, n_particles, dtype));
    DZO_TRY(require_same_backend("accelerated_pairwise_radial_energy", "src/ExampleFunctions.jl:165-167", x_dev, "x", y_dev, "y"));
    DZO_TRY(require_same_backend("accelerated_pairwise_radial_energy", "src/ExampleFunctions.jl:165-167", x_dev, "x", z_dev, "z"));
    Context &c = ctx();
    double *ws = nullptr;
    DZO_TRY(pw_ctx_workspace(n_particles, &ws));
    {
        DZO_TIMED("pairwise_energy", c.stream);
        DZO_TRY(pairwise_energy_async(c.stream, radial, n_particles, dtype, x_dev, y_dev, z_dev, ws, c.scratch));
    }
    DZO_TRY(copy_blocking(c.host_scalar, c.scratch, sizeof(double), hipMemcpyDeviceToHost));
    *energy = c.host_scalar[0];
    return DZO_OK;
}

// accelerated_pairwise_radial_gradient!, src/ExampleFunctions.jl:265-294
int32_t dzo_pairwise_gradient(int32_t radial, int64_t n_particles, int32_t dtype, void *gx_dev, void *gy_dev, void *gz_dev,
                              const void *x_dev, const void *y_dev, const void *z_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(gx_dev && gy_dev && gz_dev && x_dev && y_dev && z_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_common(radial, n_particles, dtype));
    const char *where = "accelerated_pairwise_radial_gradient!", *cite = "src/ExampleFunctions.jl:284-289";
    DZO_TRY(require_same_backend(where, cite, gx_dev, "gx", gy_dev, "gy"));
    DZO_TRY(require_same_backend(where, cite, gx_dev, "gx", gz_dev, "gz"));
    DZO_TRY(require_same_backend(where, cite, gx_dev, "gx", x_dev, "x"));
    DZO_TRY(require_same_backend(where, cite, gx_dev, "gx", y_dev, "y"));
    DZO_TRY(require_same_backend(where, cite, gx_dev, "gx", z_dev, "z"));
    Context &c = ctx();
    double *ws = nullptr;
    DZO_TRY(pw_ctx_workspace(n_particles, &ws));
    {
        DZO_TIMED("pairwise_gradient", c.stream);
        DZO_TRY(pairwise_gradient_async(c.stream, radial, n_particles, dtype, gx_dev, gy_dev, gz_dev, x_dev, y_dev, z_dev, ws));
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// accelerated_pairwise_radial_hvp!, src/ExampleFunctions.jl:427-468
int32_t dzo_pairwise_hvp(int32_t radial, int64_t n_particles, int32_t dtype, void *px_dev, void *py_dev, void *pz_dev, const void *x_dev,
                         const void *y_dev, const void *z_dev, const void *u_dev, const void *v_dev, const void *w_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(px_dev && py_dev && pz_dev && x_dev && y_dev && z_dev && u_dev && v_dev && w_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_common(radial, n_particles, dtype));
    const char *where = "accelerated_pairwise_radial_hvp!", *cite = "src/ExampleFunctions.jl:453-461";
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", py_dev, "py"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", pz_dev, "pz"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", x_dev, "x"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", y_dev, "y"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", z_dev, "z"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", u_dev, "u"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", v_dev, "v"));
    DZO_TRY(require_same_backend(where, cite, px_dev, "px", w_dev, "w"));
    Context &c = ctx();
    double *ws = nullptr;
    DZO_TRY(pw_ctx_workspace(n_particles, &ws));
    {
        DZO_TIMED("pairwise_hvp", c.stream);
        DZO_DISPATCH_RADIAL(radial, dtype, DZO_TRY((pw_rows_t<T, F, kPwHvp>(c.stream, n_particles, (T *)px_dev, (T *)py_dev, (T *)pz_dev,
                                                                            (const T *)x_dev, (const T *)y_dev, (const T *)z_dev,
                                                                            (const T *)u_dev, (const T *)v_dev, (const T *)w_dev, ws))));
    }
    DZO_HIP(hipStreamSynchronize(c.stream));
    return DZO_OK;
}

// pairwise_radial_energy_delta, src/ExampleFunctions.jl:477-534 (i is 0-based here)
int32_t dzo_pairwise_energy_delta(int32_t radial, int64_t n_particles, int32_t dtype, const void *x_dev, const void *y_dev,
                                  const void *z_dev, int64_t i, double x_new, double y_new, double z_new, double *delta) {
    DZO_TRY(require_init());
    DZO_REQUIRE(x_dev && y_dev && z_dev && delta, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_common(radial, n_particles, dtype));
    DZO_REQUIRE(i >= 0 && i < n_particles, DZO_ERR_INVALID, "particle index %lld outside 0 .. %lld (i in particle_axis, src/ExampleFunctions.jl:494)",
                (long long)i, (long long)(n_particles - 1));
    DZO_TRY(require_same_backend("pairwise_radial_energy_delta", "src/ExampleFunctions.jl:490-493", x_dev, "x", y_dev, "y"));
    DZO_TRY(require_same_backend("pairwise_radial_energy_delta", "src/ExampleFunctions.jl:490-493", x_dev, "x", z_dev, "z"));
    Context &c = ctx();
    {
        DZO_TIMED("pairwise_energy_delta", c.stream);
        DZO_DISPATCH_RADIAL(radial, dtype, hipLaunchKernelGGL((pairwise_energy_delta_kernel<T, F>), dim3(1), dim3(kBlock), 0, c.stream, n_particles,
                                                              (const T *)x_dev, (const T *)y_dev, (const T *)z_dev, i, (T)x_new, (T)y_new, (T)z_new,
                                                              c.scratch));
        DZO_HIP(hipGetLastError());
    }
    DZO_TRY(copy_blocking(c.host_scalar, c.scratch, sizeof(double), hipMemcpyDeviceToHost));
    *delta = c.host_scalar[0];
    return DZO_OK;
}

// Calibration: GFLOP/s (2 per fma) of a register-only fma loop, 16 independent chains per lane, 8 blocks of 256 per CU.
// The vector-ALU ceiling the pairwise kernels are held against (tools/bench_pairwise.py).
int32_t dzo_calibrate_fma_rate(int32_t dtype, int64_t iters, double *gflops) {
    DZO_TRY(require_init());
    DZO_REQUIRE(gflops && iters >= 1, DZO_ERR_INVALID, "bad argument (at least one iteration)");
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    Context &c = ctx();
    const int grid = c.cus * 8;
    void *sink = nullptr;
    DZO_HIP(hipMalloc(&sink, sizeof(double) * (size_t)grid * kBlock));
    hipEvent_t a, b;
    DZO_HIP(hipEventCreate(&a)); DZO_HIP(hipEventCreate(&b));
    hipStream_t s = c.stream;
#define DZO_CALIB_FMA() DZO_DISPATCH(dtype, hipLaunchKernelGGL(calib_fma_kernel<T>, dim3(grid), dim3(kBlock), 0, s, iters, (T)0.999999, (T)1e-6, (T *)sink))
    DZO_CALIB_FMA();                                         // untimed pass
    DZO_HIP(hipEventRecord(a, s));
    DZO_CALIB_FMA();
    DZO_HIP(hipEventRecord(b, s));
#undef DZO_CALIB_FMA
    DZO_HIP(hipEventSynchronize(b));
    float ms = 0;
    DZO_HIP(hipEventElapsedTime(&ms, a, b));
    *gflops = 2.0 * 16.0 * (double)iters * (double)grid * kBlock / (ms * 1e-3) / 1e9;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(sink);
    return DZO_OK;
}

}  // extern "C"
