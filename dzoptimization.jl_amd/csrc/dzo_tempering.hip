// dzo_tempering.hip -- parallel-tempering Monte Carlo over Lennard-Jones replicas (scripts/MonteCarlo.jl) on gfx950.
//
// The reference runs one CPU thread per replica (:38) and, per move, one O(N) energy difference (:57-62).  Through the C
// ABI of the pairwise functions that is one launch and one host wait per move of one replica.  Here one launch runs
// num_steps moves of EVERY replica and the host is not involved between moves:
//
//   * WAVE shape (N <= 64): one wave per replica (a block of 64 threads, so 256 replicas are one wave on each of 256
//     CUs).  Lane j holds particle j in registers.  The random draws, the chosen particle, the proposal, the sphere test
//     and the decision are computed by every lane alike (wave-uniform values; nothing to broadcast, no divergence); the
//     old position comes from lane j through v_readlane; each lane evaluates its own pair twice (old, new) and two fixed
//     DPP / permlane trees (wave_sum_all) add the lanes.  No LDS, no barrier, no global access but the trace.
//   * BLOCK shape (N <= 1024): one 256-thread block per replica, coordinates in LDS (every lane reads the same address in
//     the pair loops: a broadcast), thread t takes j = t, t + 256, ...; two barriers per move (sums, coordinate update).
//
// The per-pair arithmetic is pairwise_energy_delta_kernel's: both call pw_pair_energy of dzo_pairwise.h (the self term removed by a select);
// lane sums are in T, sums across lanes / waves in fp64 in a fixed order, one rounding back to T.  No floating-point atomic.
// The random-number rule is stated in include/dzo.h; it is the specification and tests/tempering_twin.py replays it.
#include "dzo_cluster.h"
#include "dzo_pairwise.h"
#include "dzo_pcg.h"

#include <cmath>
#include <new>

namespace dzo {

constexpr int kTemperMaxN = DZO_TEMPERING_MAX_PARTICLES;

template <typename T> struct McDraws { int j; T nx, ny, nz, u; };

// the six draws of one Monte Carlo step (include/dzo.h); the generator and the Box-Muller formulas are dzo_pcg.h's
template <typename T> __device__ __forceinline__ McDraws<T> mc_draw(uint64_t &s, int N) {
    const uint32_t d0 = pcg_draw(s), d1 = pcg_draw(s), d2 = pcg_draw(s), d3 = pcg_draw(s), d4 = pcg_draw(s), d5 = pcg_draw(s);
    McDraws<T> d;
    d.j = (int)(((uint64_t)d0 * (uint64_t)N) >> 32);
    pcg_normals<T>(d1, d2, d3, d4, d.nx, d.ny, d.nz);
    d.u = pcg_uniform<T>(d5);
    return d;
}

template <typename T> struct TemperArgs {
    int N;
    int64_t num_steps;
    T *replicas;
    const T *inv_temps;
    T *radii;
    T constraining_radius, fac;
    uint64_t *rng;
    int64_t *num_accept, *num_reject;
    T *energies;            // may be null
    int64_t ld;
    int64_t rec_cap;        // 0: no record
    int32_t *rec_index;
    T *rec_normals, *rec_uniform;
    int8_t *rec_code;
};

// Where lane / thread 0 of replica k stores after every step (:75); the addresses are pinned to vector registers (pw_pin_ptr).
template <typename T> struct McOut {
    T *energies;            // null: no trace
    int32_t *rec_index;     // null: no record
    T *rec_normals, *rec_uniform;
    int8_t *rec_code;
    __device__ __forceinline__ McOut(const TemperArgs<T> &a, int64_t k) {
        energies = pw_pin_ptr(a.energies ? a.energies + a.ld * k : nullptr);
        const bool rec = a.rec_cap > 0;
        const int64_t r = a.rec_cap * k;
        rec_index = pw_pin_ptr(rec ? a.rec_index + r : nullptr);
        rec_normals = pw_pin_ptr(rec ? a.rec_normals + 3 * r : nullptr);
        rec_uniform = pw_pin_ptr(rec ? a.rec_uniform + r : nullptr);
        rec_code = pw_pin_ptr(rec ? a.rec_code + r : nullptr);
    }
    __device__ __forceinline__ void step(int64_t i, T energy, const McDraws<T> &d, int code) const {
        if (energies) energies[i] = energy;
        if (rec_index) {
            rec_index[i] = d.j;
            rec_normals[3 * i + 0] = d.nx;
            rec_normals[3 * i + 1] = d.ny;
            rec_normals[3 * i + 2] = d.nz;
            rec_uniform[i] = d.u;
            rec_code[i] = (int8_t)code;
        }
    }
};
// ... and after the last one (:77-81)
template <typename T> struct McEnd {
    T *radius_out;
    uint64_t *rng_out;
    int64_t *acc_out, *rej_out;
    T fac;
    __device__ __forceinline__ McEnd(const TemperArgs<T> &a, int64_t k) {
        radius_out = pw_pin_ptr(a.radii + k);
        rng_out = pw_pin_ptr(a.rng + k);
        acc_out = pw_pin_ptr(a.num_accept + k);
        rej_out = pw_pin_ptr(a.num_reject + k);
        fac = pw_pin(a.fac);
    }
    __device__ __forceinline__ void store(T radius, int64_t acc, int64_t rej, uint64_t s) const {
        *radius_out = mc_adapted_radius<T>(radius, acc, rej, fac);
        *rng_out = s;
        *acc_out = acc;
        *rej_out = rej;
    }
};

// ------------------------------------------------------------------------------ WAVE shape: grid R, block 64
// (each kernel of this file that evaluates pairs is its body as a __device__ function and the entry point that calls it: written
// into the __global__ function itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
template <typename T, typename F> __device__ __forceinline__ void temper_wave_body(TemperArgs<T> a) {
    const int lane = threadIdx.x, N = a.N;
    const int64_t k = blockIdx.x;
    T *rep = a.replicas + (int64_t)3 * N * k;
    const bool live = lane < N;
    T x = live ? rep[lane] : T(0), y = live ? rep[N + lane] : T(0), z = live ? rep[2 * N + lane] : T(0);
    // the full energy, :39-43: lane i adds row i over j in T, the rows are added in fp64, halved once
    T row = T(0);
    for (int j = 0; j < N; ++j) {
        const T e = pw_pair_energy<T, F>(x, y, z, lane_read(x, j), lane_read(y, j), lane_read(z, j));
        row += j == lane ? T(0) : e;
    }
    T energy = (T)(0.5 * wave_sum_all(live ? (double)row : 0.0));
    uint64_t s = a.rng[k];
    const T beta = a.inv_temps[k], radius = a.radii[k];
    const T R2 = pw_square(a.constraining_radius);
    const McOut<T> out(a, k);
    const McEnd<T> end(a, k);
    int64_t acc = 0, rej = 0;
    for (int64_t i = 0; i < a.num_steps; ++i) {
        const McDraws<T> d = mc_draw<T>(s, N);
        const int j = __builtin_amdgcn_readfirstlane(d.j);
        const T xo = lane_read(x, j), yo = lane_read(y, j), zo = lane_read(z, j);
        const T xn = xo + radius * d.nx, yn = yo + radius * d.ny, zn = zo + radius * d.nz;
        int code = 2;
        if (pw_square(xn) + pw_square(yn) + pw_square(zn) < R2) {
            const bool drop = lane == j || !live;
            const T eo = pw_pair_energy<T, F>(xo, yo, zo, x, y, z), en = pw_pair_energy<T, F>(xn, yn, zn, x, y, z);
            const double so = wave_sum_all(drop ? 0.0 : (double)eo), sn = wave_sum_all(drop ? 0.0 : (double)en);
            const T delta = (T)sn - (T)so;
            const bool accept = delta <= T(0) || d.u <= mc_exp<T>(-beta * delta);
            code = accept ? 1 : 0;
            if (accept) {
                if (lane == j) { x = xn; y = yn; z = zn; }
                energy += delta;
            }
        }
        acc += code == 1;
        rej += code != 1;
        if (lane == 0) out.step(i, energy, d, code);
    }
    if (live) { rep[lane] = x; rep[N + lane] = y; rep[2 * N + lane] = z; }
    if (lane == 0) end.store(radius, acc, rej, s);
}
template <typename T, typename F> __global__ __launch_bounds__(64) void temper_wave_kernel(TemperArgs<T> a) { temper_wave_body<T, F>(a); }

// ------------------------------------------------------------------------------ BLOCK shape: grid R, block 256
template <typename T, typename F> __device__ __forceinline__ void temper_block_body(TemperArgs<T> a) {
    __shared__ T cx[kTemperMaxN], cy[kTemperMaxN], cz[kTemperMaxN];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, N = a.N;
    const int64_t k = blockIdx.x;
    T *rep = pw_pin_ptr(a.replicas + (int64_t)3 * N * k);
    for (int j = tid; j < N; j += kBlock) { cx[j] = rep[j]; cy[j] = rep[N + j]; cz[j] = rep[2 * N + j]; }
    __syncthreads();
    double rows = 0, unused = 0;
    for (int i = tid; i < N; i += kBlock) {
        const T xi = cx[i], yi = cy[i], zi = cz[i];
        T row = T(0);
        for (int j = 0; j < N; ++j) {
            const T e = pw_pair_energy<T, F>(xi, yi, zi, cx[j], cy[j], cz[j]);
            row += j == i ? T(0) : e;
        }
        rows += (double)row;
    }
    cl_block_sum2(rows, unused, red);
    __syncthreads();
    T energy = (T)(0.5 * rows);
    uint64_t s = a.rng[k];
    // (loop invariants pinned to vector registers: see pw_pin_ptr)
    const T beta = pw_pin(a.inv_temps[k]), radius = pw_pin(a.radii[k]);
    const T R2 = pw_pin(pw_square(a.constraining_radius));
    const McOut<T> out(a, k);
    const McEnd<T> end(a, k);
    int64_t acc = 0, rej = 0;
    asm("" : "+v"(acc), "+v"(rej));
    for (int64_t i = 0; i < a.num_steps; ++i) {
        asm("" : "+v"(s));                                   // the generator's arithmetic in vector registers, too
        const McDraws<T> d = mc_draw<T>(s, N);               // the same bits in every thread
        const int j = d.j;
        const T xo = cx[j], yo = cy[j], zo = cz[j];
        const T xn = xo + radius * d.nx, yn = yo + radius * d.ny, zn = zo + radius * d.nz;
        const bool inside = pw_square(xn) + pw_square(yn) + pw_square(zn) < R2;
        T e_old = T(0), e_new = T(0);
        if (inside) {
            for (int jj = tid; jj < N; jj += kBlock) {
                const T xj = cx[jj], yj = cy[jj], zj = cz[jj];
                const T eo = pw_pair_energy<T, F>(xo, yo, zo, xj, yj, zj), en = pw_pair_energy<T, F>(xn, yn, zn, xj, yj, zj);
                e_old += jj == j ? T(0) : eo;
                e_new += jj == j ? T(0) : en;
            }
        }
        double so = (double)e_old, sn = (double)e_new;
        cl_block_sum2(so, sn, red);                         // (both barriers are passed by every thread on every step)
        int code = 2;
        if (inside) {
            const T delta = (T)sn - (T)so;
            const bool accept = delta <= T(0) || d.u <= mc_exp<T>(-beta * delta);
            code = accept ? 1 : 0;
            if (accept) {
                if (tid == 0) { cx[j] = xn; cy[j] = yn; cz[j] = zn; }
                energy += delta;
            }
        }
        acc += code == 1;
        rej += code != 1;
        if (tid == 0) out.step(i, energy, d, code);
        __syncthreads();                                     // the new coordinates are in LDS, the sums have been read
    }
    for (int j = tid; j < N; j += kBlock) { rep[j] = cx[j]; rep[N + j] = cy[j]; rep[2 * N + j] = cz[j]; }
    if (tid == 0) end.store(radius, acc, rej, s);
}
template <typename T, typename F> __global__ __launch_bounds__(kBlock) void temper_block_kernel(TemperArgs<T> a) { temper_block_body<T, F>(a); }

// ------------------------------------------------------------------------------ swap (:89-136): grid ceil(R / 2), block 256
// Block b owns the pair (a, a + 1), a = 2 b + odd, when a + 1 < R, and the record slots a and a + 1 (block 0 also slot 0 when
// odd).  Dynamic LDS: both replicas, 6 N elements (they are adjacent in memory).
extern __shared__ double tempering_smem[];

template <typename T, typename F>
__device__ __forceinline__ void swap_body(int N, int64_t R, int odd, T *__restrict__ replicas, const T *__restrict__ inv_temps,
                                          uint64_t *__restrict__ rng, int8_t *__restrict__ rec_swap, T *__restrict__ rec_logp) {
    __shared__ double red[2 * kWaves];
    T *c = reinterpret_cast<T *>(tempering_smem);
    const int tid = threadIdx.x;
    const int64_t ka = 2 * (int64_t)blockIdx.x + (odd ? 1 : 0), kb = ka + 1;
    if (tid == 0) {
        if (odd && blockIdx.x == 0) { rec_swap[0] = -1; rec_logp[0] = T(0); }
        if (ka < R && kb >= R) { rec_swap[ka] = -1; rec_logp[ka] = T(0); }
        if (kb < R) { rec_swap[kb] = -1; rec_logp[kb] = T(0); }
    }
    if (kb >= R) return;                                     // the whole block leaves
    T *ra = replicas + (int64_t)3 * N * ka;
    const int n6 = 6 * N, n3 = 3 * N;
    for (int t = tid; t < n6; t += kBlock) c[t] = ra[t];
    uint64_t s = rng[ka];
    __syncthreads();
    double sa = 0, sb = 0;
    for (int i = tid; i < N; i += kBlock) {
        const T xa = c[i], ya = c[N + i], za = c[2 * N + i];
        const T xb = c[n3 + i], yb = c[n3 + N + i], zb = c[n3 + 2 * N + i];
        T row_a = T(0), row_b = T(0);
        for (int j = 0; j < N; ++j) {
            const T ea = pw_pair_energy<T, F>(xa, ya, za, c[j], c[N + j], c[2 * N + j]);
            const T eb = pw_pair_energy<T, F>(xb, yb, zb, c[n3 + j], c[n3 + N + j], c[n3 + 2 * N + j]);
            row_a += j == i ? T(0) : ea;
            row_b += j == i ? T(0) : eb;
        }
        sa += (double)row_a;
        sb += (double)row_b;
    }
    cl_block_sum2(sa, sb, red);
    const T energy_a = (T)(0.5 * sa), energy_b = (T)(0.5 * sb);
    const T log_prob = (energy_a - energy_b) * (inv_temps[ka] - inv_temps[kb]);
    const T u = pcg_uniform<T>(pcg_draw(s));                  // always consumed
    const bool accept = log_prob >= T(0) || u <= mc_exp<T>(log_prob);
    if (tid == 0) {
        rng[ka] = s;
        rec_swap[ka] = accept ? 1 : 0;
        rec_logp[ka] = log_prob;
    }
    if (accept) {
        for (int t = tid; t < n3; t += kBlock) { ra[t] = c[n3 + t]; ra[n3 + t] = c[t]; }
    }
}
template <typename T, typename F>
__global__ __launch_bounds__(kBlock) void swap_kernel(int N, int64_t R, int odd, T *__restrict__ replicas, const T *__restrict__ inv_temps,
                                                      uint64_t *__restrict__ rng, int8_t *__restrict__ rec_swap, T *__restrict__ rec_logp) {
    swap_body<T, F>(N, R, odd, replicas, inv_temps, rng, rec_swap, rec_logp);
}

// ------------------------------------------------------------------------------ analyze (:139-180): grid R, block 256
// out[5 k ..] = cv, cv_prime, V1, V2, V3
template <typename T>
__global__ __launch_bounds__(kBlock) void analyze_kernel(int64_t n, const T *__restrict__ energies, int64_t ld, const T *__restrict__ inv_temps,
                                                         T *__restrict__ out) {
    __shared__ double lds[3 * kWaves];
    const int64_t k = blockIdx.x;
    const T *e = energies + ld * k;
    double v[3] = {0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const double E = (double)e[i];
        const double E2 = E * E;
        v[0] += E; v[1] += E2; v[2] += E2 * E;
    }
    double r[3];
    block_sum_multi<3>(v, lds, r);
    if (threadIdx.x == 0) {
        const double nn = (double)n;
        const T V1 = (T)(r[0] / nn), V2 = (T)(r[1] / nn), V3 = (T)(r[2] / nn);
        const T inv_tau = inv_temps[k];
        const T inv_tau_2 = pw_square(inv_tau);
        const T inv_tau_4 = pw_square(inv_tau_2);
        const T var = V2 - pw_square(V1);
        const T cov = V3 - V2 * V1;
        out[5 * k + 0] = inv_tau_2 * var;
        out[5 * k + 1] = inv_tau_4 * (cov - (V1 + T(1) / inv_tau) * pw_twice(var));
        out[5 * k + 2] = V1; out[5 * k + 3] = V2; out[5 * k + 4] = V3;
    }
}

}  // namespace dzo

using namespace dzo;

struct dzo_tempering_s {
    int device = -1;
    int32_t dtype = DZO_F64, radial = DZO_RADIAL_LENNARD_JONES;
    int N = 0;
    int64_t R = 0;
    void *replicas = nullptr;        // the caller's
    void *inv_temps = nullptr, *radii = nullptr, *analysis = nullptr, *rec_logp = nullptr;
    uint64_t *rng = nullptr;
    int64_t *counts = nullptr;       // num_accept[R] | num_reject[R]
    int8_t *rec_swap = nullptr;
    double constraining_radius = 0, fac = 0;
    int64_t rec_cap = 0;
    int32_t *rec_index = nullptr;
    void *rec_normals = nullptr, *rec_uniform = nullptr;
    int8_t *rec_code = nullptr;
};

namespace dzo {

static void tp_free_record(dzo_tempering_s *h) {
    if (h->rec_index) (void)hipFree(h->rec_index);
    if (h->rec_normals) (void)hipFree(h->rec_normals);
    if (h->rec_uniform) (void)hipFree(h->rec_uniform);
    if (h->rec_code) (void)hipFree(h->rec_code);
    h->rec_index = nullptr; h->rec_normals = nullptr; h->rec_uniform = nullptr; h->rec_code = nullptr;
    h->rec_cap = 0;
}

static void tp_free(dzo_tempering_s *h) {
    tp_free_record(h);
    void *p[] = {h->inv_temps, h->radii, h->analysis, h->rec_logp, h->rng, h->counts, h->rec_swap};
    for (void *q : p)
        if (q) (void)hipFree(q);
    delete h;
}

static int32_t tp_alloc(void **p, size_t bytes) { return device_alloc(p, bytes, "the tempering state", false); }

template <typename T, typename F> static int32_t tp_temper_t(dzo_tempering_s *h, hipStream_t s, int64_t num_steps, void *energies, int64_t ld) {
    TemperArgs<T> a;
    a.N = h->N;
    a.num_steps = num_steps;
    a.replicas = (T *)h->replicas;
    a.inv_temps = (const T *)h->inv_temps;
    a.radii = (T *)h->radii;
    a.constraining_radius = (T)h->constraining_radius;
    a.fac = (T)h->fac;
    a.rng = h->rng;
    a.num_accept = h->counts;
    a.num_reject = h->counts + h->R;
    a.energies = (T *)energies;
    a.ld = ld;
    a.rec_cap = h->rec_cap;
    a.rec_index = h->rec_index;
    a.rec_normals = (T *)h->rec_normals;
    a.rec_uniform = (T *)h->rec_uniform;
    a.rec_code = h->rec_code;
    if (h->N <= 64) hipLaunchKernelGGL((temper_wave_kernel<T, F>), dim3((unsigned)h->R), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((temper_block_kernel<T, F>), dim3((unsigned)h->R), dim3(kBlock), 0, s, a);
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

static int32_t tp_temper(dzo_tempering_s *h, hipStream_t s, int64_t num_steps, void *energies, int64_t ld) {
    DZO_TIMED("tempering_temper", s);
    DZO_DISPATCH_RADIAL(h->radial, h->dtype, return (tp_temper_t<T, F>(h, s, num_steps, energies, ld)));
    return DZO_OK;
}

static int32_t tp_swap(dzo_tempering_s *h, hipStream_t s, int32_t odd) {
    DZO_TIMED("tempering_swap", s);
    const unsigned grid = (unsigned)((h->R + 1) / 2);
    const size_t lds = (size_t)6 * h->N * dtype_size(h->dtype);
    DZO_DISPATCH_RADIAL(h->radial, h->dtype,
                        hipLaunchKernelGGL((swap_kernel<T, F>), dim3(grid), dim3(kBlock), lds, s, h->N, h->R, odd ? 1 : 0, (T *)h->replicas,
                                           (const T *)h->inv_temps, h->rng, h->rec_swap, (T *)h->rec_logp));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

static int32_t tp_check_trace(dzo_tempering_s *h, const char *where, int64_t rows, const void *energies_dev, int64_t ld) {
    DZO_REQUIRE(rows >= 0, DZO_ERR_INVALID, "%s: num_steps must not be negative (got %lld)", where, (long long)rows);
    if (energies_dev) {
        DZO_REQUIRE(ld >= rows && ld >= 1, DZO_ERR_INVALID, "%s: leading dimension %lld is smaller than the %lld rows of the trace", where,
                    (long long)ld, (long long)rows);
        DZO_TRY(require_same_backend(where, "scripts/MonteCarlo.jl:30-33", h->replicas, "replicas", energies_dev, "energies"));
    }
    return DZO_OK;
}

// `what` -> device address, bytes
static int32_t tp_array(dzo_tempering_s *h, int32_t what, void **p, size_t *bytes) {
    const size_t es = dtype_size(h->dtype), R = (size_t)h->R, cap = (size_t)h->rec_cap;
    const bool rec = what >= DZO_TEMPERING_REC_INDEX && what <= DZO_TEMPERING_REC_CODE;
    DZO_REQUIRE(!rec || h->rec_cap > 0, DZO_ERR_STATE, "nothing is being recorded (dzo_tempering_set_record)");
    switch (what) {
    case DZO_TEMPERING_REPLICAS: *p = h->replicas; *bytes = es * 3 * (size_t)h->N * R; break;
    case DZO_TEMPERING_RADII: *p = h->radii; *bytes = es * R; break;
    case DZO_TEMPERING_INV_TEMPS: *p = h->inv_temps; *bytes = es * R; break;
    case DZO_TEMPERING_NUM_ACCEPT: *p = h->counts; *bytes = 8 * R; break;
    case DZO_TEMPERING_NUM_REJECT: *p = h->counts + h->R; *bytes = 8 * R; break;
    case DZO_TEMPERING_RNG_STATES: *p = h->rng; *bytes = 8 * R; break;
    case DZO_TEMPERING_REC_INDEX: *p = h->rec_index; *bytes = 4 * cap * R; break;
    case DZO_TEMPERING_REC_NORMALS: *p = h->rec_normals; *bytes = es * 3 * cap * R; break;
    case DZO_TEMPERING_REC_UNIFORM: *p = h->rec_uniform; *bytes = es * cap * R; break;
    case DZO_TEMPERING_REC_CODE: *p = h->rec_code; *bytes = cap * R; break;
    case DZO_TEMPERING_REC_SWAP: *p = h->rec_swap; *bytes = R; break;
    case DZO_TEMPERING_REC_SWAP_LOGP: *p = h->rec_logp; *bytes = es * R; break;
    default: set_error("unknown tempering array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

// the arguments of parallel_temper! / parallel_swap!, scripts/MonteCarlo.jl:8-15, :89-94
int32_t dzo_tempering_create(int32_t radial, int64_t n_particles, int64_t n_replicas, int32_t dtype, void *replicas_dev,
                             const double *inverse_temperatures, const double *perturbation_radii, double constraining_radius,
                             uint64_t base_seed, dzo_tempering_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(replicas_dev && inverse_temperatures && perturbation_radii, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_args(radial, dtype, n_particles, n_replicas, "n_replicas", kTemperMaxN, DZO_ERR_UNSUPPORTED,
                          "the tempering kernels hold a replica in LDS"));
    DZO_TRY(require_same_backend("parallel_temper!", "scripts/MonteCarlo.jl:31", replicas_dev, "replicas", nullptr, ""));
    Context &c = ctx();
    dzo_tempering_s *h = new (std::nothrow) dzo_tempering_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    h->device = c.device; h->dtype = dtype; h->radial = radial; h->N = (int)n_particles; h->R = n_replicas; h->replicas = replicas_dev;
    h->constraining_radius = constraining_radius;
    h->fac = dtype == DZO_F64 ? mc_fac<double>() : mc_fac<float>();
    const size_t es = dtype_size(dtype), R = (size_t)n_replicas;
    int32_t rc = DZO_OK;
    if ((rc = tp_alloc(&h->inv_temps, es * R)) || (rc = tp_alloc(&h->radii, es * R)) || (rc = tp_alloc(&h->analysis, es * 5 * R)) ||
        (rc = tp_alloc(&h->rec_logp, es * R)) || (rc = tp_alloc((void **)&h->rng, 8 * R)) || (rc = tp_alloc((void **)&h->counts, 16 * R)) ||
        (rc = tp_alloc((void **)&h->rec_swap, R))) {
        tp_free(h);
        return rc;
    }
    std::vector<uint64_t> states(R);
    for (size_t k = 0; k < R; ++k) states[k] = pcg_advance(kPcgInc + (base_seed + (uint64_t)k));
    std::vector<double> hd(2 * R);
    std::vector<float> hf(2 * R);
    for (size_t k = 0; k < R; ++k) {
        hd[k] = inverse_temperatures[k]; hd[R + k] = perturbation_radii[k];
        hf[k] = (float)inverse_temperatures[k]; hf[R + k] = (float)perturbation_radii[k];
    }
    const void *src = dtype == DZO_F64 ? (const void *)hd.data() : (const void *)hf.data();
    hipError_t e = hipMemcpy(h->inv_temps, src, es * R, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->radii, (const char *)src + es * R, es * R, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->rng, states.data(), 8 * R, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->counts, 0, 16 * R);
    if (e == hipSuccess) e = hipMemset(h->rec_swap, 0xFF, R);
    if (e == hipSuccess) e = hipMemset(h->rec_logp, 0, es * R);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { tp_free(h); return hip_fail(e, "tempering state upload", __FILE__, __LINE__); }
    *out = h;
    return DZO_OK;
}

int32_t dzo_tempering_destroy(dzo_tempering_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->device);
    (void)hipStreamSynchronize(ctx().stream);
    tp_free(h);
    return DZO_OK;
}

// parallel_temper!, scripts/MonteCarlo.jl:8-86
int32_t dzo_tempering_temper(dzo_tempering_t h, int64_t num_steps, void *energies_dev, int64_t ld) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DeviceScope scope(h->device);
    DZO_TRY(tp_check_trace(h, "parallel_temper!", num_steps, energies_dev, ld));
    DZO_REQUIRE(h->rec_cap == 0 || num_steps <= h->rec_cap, DZO_ERR_INVALID, "%lld steps do not fit the record of %lld (dzo_tempering_set_record)",
                (long long)num_steps, (long long)h->rec_cap);
    return tp_temper(h, ctx().stream, num_steps, energies_dev, ld);
}

// parallel_swap!, scripts/MonteCarlo.jl:89-136
int32_t dzo_tempering_swap(dzo_tempering_t h, int32_t odd) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DeviceScope scope(h->device);
    return tp_swap(h, ctx().stream, odd);
}

// the loop body of main, scripts/MonteCarlo.jl:222-231
int32_t dzo_tempering_run(dzo_tempering_t h, int64_t num_steps, int64_t num_batches, void *energies_dev, int64_t ld) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(num_batches >= 0, DZO_ERR_INVALID, "num_batches must not be negative (got %lld)", (long long)num_batches);
    DeviceScope scope(h->device);
    DZO_TRY(tp_check_trace(h, "main", num_steps, energies_dev, ld));
    DZO_REQUIRE(!energies_dev || ld >= 2 * num_steps * num_batches, DZO_ERR_INVALID, "leading dimension %lld is smaller than the 2 * %lld * %lld rows of the trace",
                (long long)ld, (long long)num_steps, (long long)num_batches);
    DZO_REQUIRE(h->rec_cap == 0 || num_steps <= h->rec_cap, DZO_ERR_INVALID, "%lld steps do not fit the record of %lld (dzo_tempering_set_record)",
                (long long)num_steps, (long long)h->rec_cap);
    hipStream_t s = ctx().stream;
    const size_t es = dtype_size(h->dtype);
    for (int64_t b = 0; b < num_batches; ++b) {
        char *even_view = energies_dev ? (char *)energies_dev + es * (size_t)(num_steps * (2 * b)) : nullptr;      // :223
        char *odd_view = energies_dev ? (char *)energies_dev + es * (size_t)(num_steps * (2 * b + 1)) : nullptr;   // :224
        DZO_TRY(tp_temper(h, s, num_steps, even_view, ld));
        DZO_TRY(tp_swap(h, s, 0));
        DZO_TRY(tp_temper(h, s, num_steps, odd_view, ld));
        DZO_TRY(tp_swap(h, s, 1));
    }
    return DZO_OK;
}

// analyze, scripts/MonteCarlo.jl:139-180
int32_t dzo_tempering_analyze(dzo_tempering_t h, int64_t n_iterations, const void *energies_dev, int64_t ld, double *cv, double *cv_prime,
                              double *moments) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && energies_dev && cv && cv_prime, DZO_ERR_INVALID, "null argument");
    DZO_REQUIRE(n_iterations >= 1, DZO_ERR_INVALID, "n_iterations must be at least 1 (got %lld)", (long long)n_iterations);
    DeviceScope scope(h->device);
    DZO_TRY(tp_check_trace(h, "analyze", n_iterations, energies_dev, ld));
    hipStream_t s = ctx().stream;
    {
        DZO_TIMED("tempering_analyze", s);
        DZO_DISPATCH(h->dtype, hipLaunchKernelGGL(analyze_kernel<T>, dim3((unsigned)h->R), dim3(kBlock), 0, s, n_iterations, (const T *)energies_dev, ld,
                                                  (const T *)h->inv_temps, (T *)h->analysis));
        DZO_HIP(hipGetLastError());
    }
    const size_t R = (size_t)h->R, es = dtype_size(h->dtype);
    std::vector<char> host(es * 5 * R);
    DZO_HIP(hipMemcpyAsync(host.data(), h->analysis, host.size(), hipMemcpyDeviceToHost, s));
    DZO_HIP(hipStreamSynchronize(s));
    for (size_t k = 0; k < R; ++k)
        for (int q = 0; q < 5; ++q) {
            const double v = h->dtype == DZO_F64 ? ((const double *)host.data())[5 * k + q] : (double)((const float *)host.data())[5 * k + q];
            if (q == 0) cv[k] = v;
            else if (q == 1) cv_prime[k] = v;
            else if (moments) moments[3 * k + (q - 2)] = v;
        }
    return DZO_OK;
}

int32_t dzo_tempering_set_record(dzo_tempering_t h, int64_t capacity_steps) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(capacity_steps >= 0 && capacity_steps <= ((int64_t)1 << 24), DZO_ERR_INVALID, "capacity_steps must be in 0 .. 2^24 (got %lld)",
                (long long)capacity_steps);
    DeviceScope scope(h->device);
    DZO_HIP(hipStreamSynchronize(ctx().stream));
    tp_free_record(h);
    if (capacity_steps == 0) return DZO_OK;
    const size_t es = dtype_size(h->dtype), n = (size_t)capacity_steps * (size_t)h->R;
    int32_t rc = DZO_OK;
    if ((rc = tp_alloc((void **)&h->rec_index, 4 * n)) || (rc = tp_alloc(&h->rec_normals, es * 3 * n)) || (rc = tp_alloc(&h->rec_uniform, es * n)) ||
        (rc = tp_alloc((void **)&h->rec_code, n))) {
        tp_free_record(h);
        return rc;
    }
    h->rec_cap = capacity_steps;
    DZO_HIP(hipMemset(h->rec_index, 0, 4 * n));
    DZO_HIP(hipMemset(h->rec_normals, 0, es * 3 * n));
    DZO_HIP(hipMemset(h->rec_uniform, 0, es * n));
    DZO_HIP(hipMemset(h->rec_code, 0, n));
    DZO_HIP(hipDeviceSynchronize());
    return DZO_OK;
}

int32_t dzo_tempering_get_ptr(dzo_tempering_t h, int32_t what, void **ptr_dev) {
    DZO_REQUIRE(h && ptr_dev, DZO_ERR_INVALID, "null argument");
    size_t bytes = 0;
    return tp_array(h, what, ptr_dev, &bytes);
}

int32_t dzo_tempering_read(dzo_tempering_t h, int32_t what, void *out_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && out_host, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(tp_array(h, what, &p, &bytes));
    return copy_blocking(out_host, p, bytes, hipMemcpyDeviceToHost);
}

int32_t dzo_tempering_set(dzo_tempering_t h, int32_t what, const void *in_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && in_host, DZO_ERR_INVALID, "null argument");
    DZO_REQUIRE(what == DZO_TEMPERING_RADII || what == DZO_TEMPERING_RNG_STATES, DZO_ERR_INVALID,
                "only the perturbation radii and the random states can be set (got %d)", what);
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(tp_array(h, what, &p, &bytes));
    return copy_blocking(p, in_host, bytes, hipMemcpyHostToDevice);
}

}  // extern "C"
