// dzo_basin_hopping.hip -- basin hopping (Monte Carlo over the quenched landscape, Wales & Doye 1997) of MANY walkers over
// Lennard-Jones clusters on gfx950: the tempering move of scripts/MonteCarlo.jl applied to every particle, the quench of
// dzo_lbfgs_batch_* and the Metropolis test on the quenched energies, composed on the device.
//
// As a host loop a hop is an upload, a constructor, a chain of step launches until every instance is stuck, a read and a
// decision, and every walker waits for the slowest quench of every hop.  Here one launch runs num_hops hops of EVERY walker at
// the walker's own pace, and nothing crosses the host or device memory in between:
//
//   * WAVE shape (N <= 64): one wave per walker.  Lane i holds particle i of the current minimum and of the quench's state in
//     registers and derives its own four draws of a hop by a jump of 4 i in the walker's stream (the affine maps are built once
//     per launch); the (s, y) ring is in LDS as in the quench.  No barrier.
//   * BLOCK shape (65 <= N <= 1024): one 256-thread block per walker.  The quench's five vectors and the current minimum are
//     in LDS; the ring is in LDS where (2 m + 6) 3N elements and the scalars fit, else in a handle-owned slab.
//
// A hop is propose -> constructor -> quench_steps steps or stuck -> decide.  The constructor and the steps are the device
// functions of dzo_quench_core.h, which the kernels of dzo_lbfgs_batch.hip are built on: the quenched point, its energy, the
// iteration count and is_stuck have the bits of dzo_lbfgs_batch_create + dzo_lbfgs_batch_step(quench_steps) on the trial.
// The generator, the Box-Muller formulas, the exponential and the radius adaptation are dzo_pcg.h's, shared with
// dzo_tempering.hip.  The rule is stated in include/dzo.h; tests/basin_twin.py replays it.  The best point goes to device memory
// only when it improves; everything else is loaded once and stored once.  No floating-point read-modify-write on shared memory.
#include "dzo_cluster.h"
#include "dzo_pcg.h"
#include "dzo_quench_core.h"

#include <cmath>
#include <new>
#include <vector>

namespace dzo {

constexpr int kBasinMaxN = DZO_BASIN_HOPPING_MAX_PARTICLES;
constexpr int kBasinMaxM = DZO_LBFGS_BATCH_MAX_HISTORY;
static_assert(kBasinMaxN == kClMaxN, "the BLOCK shape of the quench holds an instance");

template <typename T> struct BasinArgs {
    int N, m, quench_steps;
    int create;                // the constructor's quench of the caller's points: no draws, always kept
    int adapt;
    int64_t num_hops, max_halvings;
    T step_length, constraining_radius, fac;
    T *points, *energies, *best_points, *best_energies, *radii;
    const T *inv_temps;
    uint64_t *rng;
    int64_t *counts;           // num_accept | num_reject | hop_counts | quench_iterations | quench_unfinished, batch each
    int64_t batch;
    T *slab;                   // BLOCK shape without room in LDS: 2 m 3N elements per walker
    int64_t rec_cap;           // 0: no record
    T *rec_normals, *rec_uniform, *rec_trial;
    int32_t *rec_iters;
    int8_t *rec_code;
};

template <typename T> __device__ __forceinline__ bool bh_finite(T v) { return v - v == T(0); }

// 0 rejected by the Metropolis test, 1 accepted, 2 the quenched energy is not finite (not inlined: see bh_particle_normals)
template <typename T> __device__ __noinline__ int bh_decide(T Eq, T E, T u, T beta) {
    if (!bh_finite(Eq)) return 2;
    const T delta = Eq - E;
    return (delta <= T(0) || u <= mc_exp<T>(-beta * delta)) ? 1 : 0;
}

// Where lane / thread 0 of walker b stores: per hop the record, after the last hop the walker's scalars.  The addresses are
// pinned to vector registers (pw_pin_ptr).
template <typename T> struct BasinOut {
    T *rec_uniform, *rec_trial;                              // null: no record
    int32_t *rec_iters;
    int8_t *rec_code;
    T *energy, *best_energy, *radius;
    uint64_t *rng;
    int64_t *counts;
    int64_t batch;
    __device__ __forceinline__ BasinOut(const BasinArgs<T> &a, int64_t b) {
        const bool rec = a.rec_cap > 0 && !a.create;
        const int64_t r = a.rec_cap * b;
        rec_uniform = pw_pin_ptr(rec ? a.rec_uniform + r : nullptr);
        rec_trial = pw_pin_ptr(rec ? a.rec_trial + r : nullptr);
        rec_iters = pw_pin_ptr(rec ? a.rec_iters + r : nullptr);
        rec_code = pw_pin_ptr(rec ? a.rec_code + r : nullptr);
        energy = pw_pin_ptr(a.energies + b);
        best_energy = pw_pin_ptr(a.best_energies + b);
        radius = pw_pin_ptr(a.radii + b);
        rng = pw_pin_ptr(a.rng + b);
        counts = pw_pin_ptr(a.counts + b);
        batch = a.batch;
        asm("" : "+v"(batch));
    }
    __device__ __forceinline__ void hop(int64_t i, T u, T trial_energy, int64_t iterations, int code) const {
        if (rec_uniform) {
            rec_uniform[i] = u;
            rec_trial[i] = trial_energy;
            rec_iters[i] = (int32_t)iterations;
            rec_code[i] = (int8_t)code;
        }
    }
    // after the constructor's quench
    __device__ __forceinline__ void created(T E) const { *energy = E; *best_energy = E; }
    // after a hop call: the adaptation of scripts/MonteCarlo.jl:77-81 on this call's counts where asked for
    __device__ __forceinline__ void called(T E, T bestE, T radius_in, T fac, bool adapt, uint64_t s, int64_t acc, int64_t rej, int64_t hops, int64_t iters,
                                           int64_t unfinished) const {
        *energy = E;
        *best_energy = bestE;
        if (adapt) *radius = mc_adapted_radius<T>(radius_in, acc, rej, fac);
        *rng = s;
        counts[0] = acc;
        counts[batch] = rej;
        counts[2 * batch] += hops;
        counts[3 * batch] += iters;
        counts[4 * batch] += unfinished;
    }
};

// The two pieces of a hop that call the fp64 math library are NOT inlined: inlined, their 64-bit constants are hoisted as
// scalar register pairs out of the loop over the hops and are live across the quench, which needs nearly every scalar
// register itself (its pair loop takes particle j through v_readlane), and the allocator then spills scalars.  Arguments and
// results travel by value, in registers: no stack.
template <typename T> struct BasinNormals { T x, y, z; };

// the draws of one particle of a hop: three normals from the four draws that follow state t
template <typename T> __device__ __noinline__ BasinNormals<T> bh_particle_normals(uint64_t t) {
    const uint32_t d1 = pcg_draw(t), d2 = pcg_draw(t), d3 = pcg_draw(t), d4 = pcg_draw(t);
    BasinNormals<T> n;
    pcg_normals<T>(d1, d2, d3, d4, n.x, n.y, n.z);
    return n;
}

// The loop over the hops holds its own values (flags, counters, the generator) in VECTOR registers: the quench inside it needs
// nearly every scalar register (its pair loop takes particle j through v_readlane).  A condition on such values is made
// wave-uniform again where it is branched on, so that the branch is a scalar one and saves no exec mask.
__device__ __forceinline__ int bh_pinned(int v) {
    asm("" : "+v"(v));
    return v;
}
__device__ __forceinline__ bool bh_uniform(bool c) { return __builtin_amdgcn_readfirstlane(c ? 1 : 0) != 0; }
// ... of a pinned flag, read anew (not kept in a scalar register since its last use)
__device__ __forceinline__ bool bh_flag(int v) { return bh_uniform(bh_pinned(v) != 0); }

// the map of a jump by k, held in vector registers: the loop over the hops keeps the scalar registers for the quench
__device__ __forceinline__ PcgMap bh_map(uint64_t k) {
    PcgMap r = pcg_jump_map(k);
    asm("" : "+v"(r.a), "+v"(r.c));
    return r;
}

extern __shared__ __attribute__((aligned(16))) double basin_smem[];

// ------------------------------------------------------------------------------ WAVE shape: grid batch, block 64
// (each kernel of this file is its body as a __device__ function and the entry point that calls it: written into the
// __global__ function itself, the same statements compile to other code -- DESIGN.md, "One table, one entry point per kernel")
template <typename T, typename F> __device__ __forceinline__ void basin_hop_wave_body(BasinArgs<T> a) {
    const int lane = threadIdx.x, N = a.N, m = a.m;
    const int64_t b = blockIdx.x, base = (int64_t)3 * N * b;
    const bool live = lane < N;
    const int create_ = bh_pinned(a.create), adapt_ = bh_pinned(a.adapt);
    T *const pts = pw_pin_ptr(a.points + base), *const best = pw_pin_ptr(a.best_points + base);
    T *const rec_n = pw_pin_ptr(a.rec_cap > 0 && !a.create ? a.rec_normals + (int64_t)3 * N * a.rec_cap * b : nullptr);
    const BasinOut<T> out(a, b);
    // LDS: rho[m] | alpha[m] | S ring | Y ring, as the quench's wave kernel
    double *rho = basin_smem, *alpha = rho + m;
    T *hS = reinterpret_cast<T *>(alpha + m), *hY = hS + m * 3 * 64;
    T cx = live ? pts[lane] : T(0), cy = live ? pts[N + lane] : T(0), cz = live ? pts[2 * N + lane] : T(0);
    T E = a.create ? T(0) : *out.energy, bestE = a.create ? T(0) : *out.best_energy;
    uint64_t s = *out.rng;
    const T beta = pw_pin(a.inv_temps[b]), radius = pw_pin(*out.radius);
    const T R2 = pw_pin(pw_square(a.constraining_radius)), fac = pw_pin(a.fac);
    // a hop takes 4 N + 1 draws: particle i the draws 4 i .. 4 i + 3, the acceptance uniform the draw 4 N
    const PcgMap mine = pcg_jump_map((uint64_t)(4 * lane)), to_uniform = bh_map((uint64_t)(4 * N)), to_next = bh_map((uint64_t)(4 * N + 1));
    int64_t acc = 0, rej = 0, iters = 0, unfinished = 0;
    asm("" : "+v"(acc), "+v"(rej), "+v"(iters), "+v"(unfinished));   // the counters in vector registers, too
    int64_t hops = a.create ? 1 : a.num_hops;
    asm("" : "+v"(hops));
    for (int64_t i = 0; bh_uniform(i < hops); ++i) {
        asm("" : "+v"(s), "+v"(i));
        const bool create = bh_flag(create_);
        QcWave<T> w;
        w.x = cx; w.y = cy; w.z = cz;
        T u = T(0);
        if (!create) {                                       // propose: old + radius * n, kept inside the sphere per particle
            const BasinNormals<T> n = bh_particle_normals<T>(pcg_apply(mine, s));
            const T nx = n.x, ny = n.y, nz = n.z;
            u = pcg_uniform<T>(pcg_extract(pcg_apply(to_uniform, s)));
            s = pcg_apply(to_next, s);
            const T tx = cx + radius * nx, ty = cy + radius * ny, tz = cz + radius * nz;
            const bool inside = live && pw_square(tx) + pw_square(ty) + pw_square(tz) < R2;
            w.x = inside ? tx : cx; w.y = inside ? ty : cy; w.z = inside ? tz : cz;
            if (rec_n && live) {
                T *r = rec_n + 3 * ((int64_t)N * i + lane);
                r[0] = nx; r[1] = ny; r[2] = nz;
            }
        }
        // the constructor on the trial (:381-397), then the quench
        cl_wave_eval<T, F>(N, lane, w.x, w.y, w.z, w.E, w.gx, w.gy, w.gz);
        bool stuck = qc_wave_first_direction<T>(a.step_length, w.gx, w.gy, w.gz, w.px, w.py, w.pz);
        w.sx = w.sy = w.sz = w.yx = w.yy = w.yz = w.dE = T(0);
        w.it = 0;
        w.hc = w.halv = w.head = 0;
        if (!bh_uniform(stuck)) stuck = qc_wave_run<T, F>(N, m, lane, a.quench_steps, a.max_halvings, w, rho, alpha, hS, hY);
        const bool created = bh_flag(create_);
        const int code = created ? 1 : bh_decide<T>(w.E, E, u, beta);
        if (code == 1) { cx = w.x; cy = w.y; cz = w.z; E = w.E; }
        if (created || (bh_finite(w.E) && w.E < bestE)) {
            bestE = w.E;
            if (live) { best[lane] = w.x; best[N + lane] = w.y; best[2 * N + lane] = w.z; }
        }
        acc += code == 1;
        rej += code != 1;
        iters += w.it;
        unfinished += stuck ? 0 : 1;
        if (bh_pinned(lane) == 0) out.hop(i, u, w.E, w.it, code);
    }
    if (live) { pts[lane] = cx; pts[N + lane] = cy; pts[2 * N + lane] = cz; }
    if (bh_pinned(lane) == 0) {
        if (create_ != 0) out.created(E);
        else out.called(E, bestE, radius, fac, adapt_ != 0, s, acc, rej, hops, iters, unfinished);
    }
}
template <typename T, typename F> __global__ __launch_bounds__(64) void basin_hop_wave_kernel(BasinArgs<T> a) { basin_hop_wave_body<T, F>(a); }

// ------------------------------------------------------------------------------ BLOCK shape: grid batch, block 256
// HL: the history ring is in LDS (else in a.slab)
template <typename T, typename F, bool HL> __device__ __forceinline__ void basin_hop_block_body(BasinArgs<T> a) {
    const int tid = threadIdx.x, N = a.N, m = a.m, n3 = 3 * N;
    const int64_t b = blockIdx.x, base = (int64_t)n3 * b;
    const int create_ = bh_pinned(a.create), adapt_ = bh_pinned(a.adapt);
    // LDS: rho[m] | alpha[m] | red[2 kWaves] | X | G | D | DX | DG | M (the current minimum) | (S ring | Y ring)
    double *rho = basin_smem, *alpha = rho + m, *red = alpha + m;
    T *X = reinterpret_cast<T *>(red + 2 * kWaves), *G = X + n3, *D = G + n3, *DX = D + n3, *DG = DX + n3, *M = DG + n3;
    T *hS, *hY;
    if constexpr (HL) { hS = M + n3; hY = hS + (size_t)m * n3; }
    else { hS = a.slab + 2 * (int64_t)n3 * m * b; hY = hS + (size_t)m * n3; }
    T *const pts = pw_pin_ptr(a.points + base), *const best = pw_pin_ptr(a.best_points + base);
    T *const rec_n = pw_pin_ptr(a.rec_cap > 0 && !a.create ? a.rec_normals + (int64_t)n3 * a.rec_cap * b : nullptr);
    const BasinOut<T> out(a, b);
    QcBlock<T> w{X, G, D, DX, DG, hS, hY, rho, alpha, red, T(0), T(0), 0, 0, 0, 0, 0};
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) M[c * N + i] = pts[c * N + i];)
    T E = a.create ? T(0) : *out.energy, bestE = a.create ? T(0) : *out.best_energy;
    uint64_t s = *out.rng;
    const T beta = pw_pin(a.inv_temps[b]), radius = pw_pin(*out.radius);
    const T R2 = pw_pin(pw_square(a.constraining_radius)), fac = pw_pin(a.fac);
    PcgMap mine[kClPer];
#pragma unroll
    for (int q = 0; q < kClPer; ++q) mine[q] = pcg_jump_map((uint64_t)(4 * (tid + kBlock * q)));
    const PcgMap to_uniform = bh_map((uint64_t)(4 * N)), to_next = bh_map((uint64_t)(4 * N + 1));
    int64_t acc = 0, rej = 0, iters = 0, unfinished = 0;
    asm("" : "+v"(acc), "+v"(rej), "+v"(iters), "+v"(unfinished));   // the counters in vector registers, too
    int64_t hops = a.create ? 1 : a.num_hops;
    asm("" : "+v"(hops));
    for (int64_t hop = 0; bh_uniform(hop < hops); ++hop) {
        asm("" : "+v"(s), "+v"(hop));
        const bool create = bh_flag(create_);
        T u = T(0);
        if (!create) {
            u = pcg_uniform<T>(pcg_extract(pcg_apply(to_uniform, s)));
            CL_FOR_OWN(i, {
                const BasinNormals<T> n = bh_particle_normals<T>(pcg_apply(mine[q], s));
                const T nx = n.x, ny = n.y, nz = n.z;
                const T ox = M[i], oy = M[N + i], oz = M[2 * N + i];
                const T tx = ox + radius * nx, ty = oy + radius * ny, tz = oz + radius * nz;
                const bool inside = pw_square(tx) + pw_square(ty) + pw_square(tz) < R2;
                X[i] = inside ? tx : ox; X[N + i] = inside ? ty : oy; X[2 * N + i] = inside ? tz : oz;
                if (rec_n) {
                    T *r = rec_n + 3 * ((int64_t)N * hop + i);
                    r[0] = nx; r[1] = ny; r[2] = nz;
                }
            })
            s = pcg_apply(to_next, s);
        } else {
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) X[c * N + i] = M[c * N + i];)
        }
        __syncthreads();                                     // the trial is complete
        // the constructor on the trial (:381-397), then the quench
        T gx[kClPer], gy[kClPer], gz[kClPer];
        cl_block_eval<T, F>(N, tid, X, red, w.par, w.E, gx, gy, gz);
        bool stuck;
        const T sc = qc_block_first_scale<T>(N, tid, a.step_length, gx, gy, gz, red, w.par, stuck);
        CL_FOR_OWN(i, {
            G[i] = gx[q]; G[N + i] = gy[q]; G[2 * N + i] = gz[q];
            D[i] = stuck ? T(0) : sc * gx[q]; D[N + i] = stuck ? T(0) : sc * gy[q]; D[2 * N + i] = stuck ? T(0) : sc * gz[q];
            for (int c = 0; c < 3; ++c) DX[c * N + i] = DG[c * N + i] = T(0);
        })
        w.dE = T(0);
        w.it = 0;
        w.hc = w.halv = w.head = 0;
        if (!bh_uniform(stuck)) stuck = qc_block_run<T, F>(N, m, tid, a.quench_steps, a.max_halvings, w);
        // every thread has read X for the last time behind a barrier; from here a thread touches its own elements only
        const bool created = bh_flag(create_);
        const int code = created ? 1 : bh_decide<T>(w.E, E, u, beta);
        if (code == 1) {
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) M[c * N + i] = X[c * N + i];)
            E = w.E;
        }
        if (created || (bh_finite(w.E) && w.E < bestE)) {
            bestE = w.E;
            CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) best[c * N + i] = X[c * N + i];)
        }
        acc += code == 1;
        rej += code != 1;
        iters += w.it;
        unfinished += stuck ? 0 : 1;
        if (bh_pinned(tid) == 0) out.hop(hop, u, w.E, w.it, code);
    }
    CL_FOR_OWN(i, for (int c = 0; c < 3; ++c) pts[c * N + i] = M[c * N + i];)
    if (bh_pinned(tid) == 0) {
        if (create_ != 0) out.created(E);
        else out.called(E, bestE, radius, fac, adapt_ != 0, s, acc, rej, hops, iters, unfinished);
    }
}
template <typename T, typename F, bool HL> __global__ __launch_bounds__(kBlock) void basin_hop_block_kernel(BasinArgs<T> a) { basin_hop_block_body<T, F, HL>(a); }

}  // namespace dzo

using namespace dzo;

struct dzo_basin_hopping_s {
    int device = -1;
    int32_t dtype = DZO_F64, radial = DZO_RADIAL_LENNARD_JONES;
    int N = 0, m = 0, quench_steps = 0;
    int64_t B = 0, max_halvings = 4096;
    double step_length = 0, constraining_radius = 0, fac = 0;
    void *points = nullptr;          // the caller's
    void *energies = nullptr, *best_points = nullptr, *best_energies = nullptr, *radii = nullptr, *inv_temps = nullptr, *slab = nullptr;
    uint64_t *rng = nullptr;
    int64_t *counts = nullptr;       // num_accept | num_reject | hop_counts | quench_iterations | quench_unfinished
    bool hist_lds = true;
    size_t lds_bytes = 0;
    int64_t rec_cap = 0;
    void *rec_normals = nullptr, *rec_uniform = nullptr, *rec_trial = nullptr;
    int32_t *rec_iters = nullptr;
    int8_t *rec_code = nullptr;
};

namespace dzo {

static void bh_free_record(dzo_basin_hopping_s *h) {
    for (void *q : {h->rec_normals, h->rec_uniform, h->rec_trial, (void *)h->rec_iters, (void *)h->rec_code})
        if (q) (void)hipFree(q);
    h->rec_normals = h->rec_uniform = h->rec_trial = nullptr;
    h->rec_iters = nullptr; h->rec_code = nullptr;
    h->rec_cap = 0;
}

static void bh_free(dzo_basin_hopping_s *h) {
    bh_free_record(h);
    for (void *q : {h->energies, h->best_points, h->best_energies, h->radii, h->inv_temps, h->slab, (void *)h->rng, (void *)h->counts})
        if (q) (void)hipFree(q);
    delete h;
}

template <typename T, typename F> static const void *bh_kernel(const dzo_basin_hopping_s *h) {
    if (h->N <= 64) return (const void *)basin_hop_wave_kernel<T, F>;
    return h->hist_lds ? (const void *)basin_hop_block_kernel<T, F, true> : (const void *)basin_hop_block_kernel<T, F, false>;
}

template <typename T, typename F> static void bh_launch(hipStream_t s, const dzo_basin_hopping_s *h, int64_t num_hops, int create, int adapt) {
    BasinArgs<T> a;
    a.N = h->N; a.m = h->m; a.quench_steps = h->quench_steps;
    a.create = create; a.adapt = adapt;
    a.num_hops = num_hops; a.max_halvings = h->max_halvings;
    a.step_length = (T)h->step_length; a.constraining_radius = (T)h->constraining_radius; a.fac = (T)h->fac;
    a.points = (T *)h->points; a.energies = (T *)h->energies; a.best_points = (T *)h->best_points; a.best_energies = (T *)h->best_energies;
    a.radii = (T *)h->radii; a.inv_temps = (const T *)h->inv_temps;
    a.rng = h->rng; a.counts = h->counts; a.batch = h->B;
    a.slab = (T *)h->slab;
    a.rec_cap = h->rec_cap;
    a.rec_normals = (T *)h->rec_normals; a.rec_uniform = (T *)h->rec_uniform; a.rec_trial = (T *)h->rec_trial;
    a.rec_iters = h->rec_iters; a.rec_code = h->rec_code;
    const dim3 grid((unsigned)h->B);
    if (h->N <= 64) hipLaunchKernelGGL((basin_hop_wave_kernel<T, F>), grid, dim3(64), h->lds_bytes, s, a);
    else if (h->hist_lds) hipLaunchKernelGGL((basin_hop_block_kernel<T, F, true>), grid, dim3(kBlock), h->lds_bytes, s, a);
    else hipLaunchKernelGGL((basin_hop_block_kernel<T, F, false>), grid, dim3(kBlock), h->lds_bytes, s, a);
}

// `what` -> device address, bytes
static int32_t bh_array(dzo_basin_hopping_s *h, int32_t what, void **p, size_t *bytes) {
    const size_t es = dtype_size(h->dtype), B = (size_t)h->B, n3 = 3 * (size_t)h->N, cap = (size_t)h->rec_cap;
    const bool rec = what >= DZO_BASIN_HOPPING_REC_NORMALS && what <= DZO_BASIN_HOPPING_REC_CODE;
    DZO_REQUIRE(!rec || h->rec_cap > 0, DZO_ERR_STATE, "nothing is being recorded (dzo_basin_hopping_set_record)");
    switch (what) {
    case DZO_BASIN_HOPPING_POINTS: *p = h->points; *bytes = es * n3 * B; break;
    case DZO_BASIN_HOPPING_ENERGIES: *p = h->energies; *bytes = es * B; break;
    case DZO_BASIN_HOPPING_BEST_POINTS: *p = h->best_points; *bytes = es * n3 * B; break;
    case DZO_BASIN_HOPPING_BEST_ENERGIES: *p = h->best_energies; *bytes = es * B; break;
    case DZO_BASIN_HOPPING_RADII: *p = h->radii; *bytes = es * B; break;
    case DZO_BASIN_HOPPING_INV_TEMPS: *p = h->inv_temps; *bytes = es * B; break;
    case DZO_BASIN_HOPPING_NUM_ACCEPT: *p = h->counts; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_NUM_REJECT: *p = h->counts + h->B; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_RNG_STATES: *p = h->rng; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_HOP_COUNTS: *p = h->counts + 2 * h->B; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_QUENCH_ITERATIONS: *p = h->counts + 3 * h->B; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_QUENCH_UNFINISHED: *p = h->counts + 4 * h->B; *bytes = 8 * B; break;
    case DZO_BASIN_HOPPING_REC_NORMALS: *p = h->rec_normals; *bytes = es * n3 * cap * B; break;
    case DZO_BASIN_HOPPING_REC_UNIFORM: *p = h->rec_uniform; *bytes = es * cap * B; break;
    case DZO_BASIN_HOPPING_REC_TRIAL_ENERGY: *p = h->rec_trial; *bytes = es * cap * B; break;
    case DZO_BASIN_HOPPING_REC_QUENCH_ITERATIONS: *p = h->rec_iters; *bytes = 4 * cap * B; break;
    case DZO_BASIN_HOPPING_REC_CODE: *p = h->rec_code; *bytes = cap * B; break;
    default: set_error("unknown basin-hopping array %d", what); return DZO_ERR_INVALID;
    }
    return DZO_OK;
}

}  // namespace dzo

extern "C" {

int32_t dzo_basin_hopping_create(int32_t radial, int64_t n_particles, int64_t batch, int32_t dtype, void *points_dev,
                                 const double *inverse_temperatures, const double *perturbation_radii, double constraining_radius,
                                 double initial_step_length, int32_t history_length, int32_t quench_steps, uint64_t base_seed,
                                 dzo_basin_hopping_t *out) {
    DZO_TRY(require_init());
    DZO_REQUIRE(out, DZO_ERR_INVALID, "null argument");
    *out = nullptr;
    DZO_REQUIRE(points_dev && inverse_temperatures && perturbation_radii, DZO_ERR_INVALID, "null argument");
    DZO_TRY(pw_check_args(radial, dtype, n_particles, batch, "batch", kBasinMaxN, DZO_ERR_UNSUPPORTED, "the basin-hopping kernels hold a walker in one block"));
    DZO_REQUIRE(history_length >= 1, DZO_ERR_INVALID, "history_length must be at least 1 (got %d)", history_length);
    DZO_REQUIRE(history_length <= kBasinMaxM, DZO_ERR_UNSUPPORTED, "history_length = %d: the batched kernels keep up to %d pairs", history_length, kBasinMaxM);
    DZO_REQUIRE(quench_steps >= 1, DZO_ERR_INVALID, "quench_steps must be at least 1 (got %d)", quench_steps);
    DZO_REQUIRE(constraining_radius > 0, DZO_ERR_INVALID, "constraining_radius must be positive (it may be infinite)");
    DZO_REQUIRE(initial_step_length > 0, DZO_ERR_ASSERT, "AssertionError: initial_step_length > _zero (src/DZOptimization.jl:380)");
    DZO_TRY(require_same_backend("LBFGSOptimizer", "src/DZOptimization.jl:363-364", points_dev, "initial_point", nullptr, ""));
    dzo_basin_hopping_s *h = new (std::nothrow) dzo_basin_hopping_s();
    DZO_REQUIRE(h, DZO_ERR_NOMEM, "out of host memory");
    h->device = ctx().device; h->dtype = dtype; h->radial = radial; h->N = (int)n_particles; h->B = batch; h->points = points_dev;
    h->m = history_length; h->quench_steps = quench_steps;
    h->step_length = initial_step_length; h->constraining_radius = constraining_radius;
    h->fac = dtype == DZO_F64 ? mc_fac<double>() : mc_fac<float>();
    const size_t es = dtype_size(dtype), B = (size_t)batch, n3 = 3 * (size_t)n_particles, m = (size_t)history_length;
    const size_t small = 16 * m;                              // rho | alpha
    if (n_particles <= 64) {
        h->lds_bytes = small + 2 * m * 3 * 64 * es;
    } else {
        const size_t vectors = small + 16 * kWaves + 6 * n3 * es;
        h->hist_lds = vectors + 2 * m * n3 * es <= kClLdsMax;
        h->lds_bytes = h->hist_lds ? vectors + 2 * m * n3 * es : vectors;
    }
    int32_t rc = cl_alloc({{&h->energies, es * B}, {&h->best_points, es * n3 * B}, {&h->best_energies, es * B}, {&h->radii, es * B},
                           {&h->inv_temps, es * B}, {h->hist_lds ? nullptr : &h->slab, 2 * es * n3 * m * B}, {(void **)&h->rng, 8 * B},
                           {(void **)&h->counts, 5 * 8 * B}},
                          "the basin-hopping state");
    if (rc != DZO_OK) { bh_free(h); return rc; }
    std::vector<uint64_t> states(B);
    for (size_t k = 0; k < B; ++k) states[k] = pcg_advance(kPcgInc + (base_seed + (uint64_t)k));
    std::vector<double> hd(2 * B);
    std::vector<float> hf(2 * B);
    for (size_t k = 0; k < B; ++k) {
        hd[k] = inverse_temperatures[k]; hd[B + k] = perturbation_radii[k];
        hf[k] = (float)inverse_temperatures[k]; hf[B + k] = (float)perturbation_radii[k];
    }
    const void *src = dtype == DZO_F64 ? (const void *)hd.data() : (const void *)hf.data();
    hipError_t e = hipMemcpy(h->inv_temps, src, es * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->radii, (const char *)src + es * B, es * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->rng, states.data(), 8 * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();          // the memsets of cl_alloc ran on the null stream
    // dynamic LDS above the default needs the attribute; it belongs to the kernel and is raised to the limit (dzo_cluster.h)
    if (e == hipSuccess && h->lds_bytes > 48 * 1024) {
        const void *k = nullptr;
        DZO_DISPATCH_RADIAL(radial, dtype, k = (bh_kernel<T, F>(h)));   // (radial and dtype have been checked)
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kClLdsMax);
    }
    if (e != hipSuccess) { bh_free(h); return hip_fail(e, "basin-hopping state upload", __FILE__, __LINE__); }
    {
        hipStream_t s = ctx().stream;
        DZO_TIMED("basin_hopping_init", s);
        DZO_DISPATCH_RADIAL(radial, dtype, (bh_launch<T, F>(s, h, 0, 1, 0)));     // the quench of the caller's points; not waited for
        e = hipGetLastError();
    }
    if (e != hipSuccess) { bh_free(h); return hip_fail(e, "basin-hopping constructor", __FILE__, __LINE__); }
    *out = h;
    return DZO_OK;
}

int32_t dzo_basin_hopping_destroy(dzo_basin_hopping_t h) {
    if (!h) return DZO_OK;
    DeviceScope scope(h->device);
    (void)hipStreamSynchronize(ctx().stream);
    bh_free(h);
    return DZO_OK;
}

int32_t dzo_basin_hopping_set_max_halvings(dzo_basin_hopping_t h, int64_t max_halvings) {
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(max_halvings >= 1, DZO_ERR_INVALID, "max_halvings must be at least 1 (got %lld): a launch cannot search without bound", (long long)max_halvings);
    h->max_halvings = max_halvings;
    return DZO_OK;
}

int32_t dzo_basin_hopping_hop(dzo_basin_hopping_t h, int64_t num_hops, int32_t adapt) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(num_hops >= 0, DZO_ERR_INVALID, "num_hops must not be negative (got %lld)", (long long)num_hops);
    DZO_REQUIRE(h->rec_cap == 0 || num_hops <= h->rec_cap, DZO_ERR_INVALID, "%lld hops do not fit the record of %lld (dzo_basin_hopping_set_record)",
                (long long)num_hops, (long long)h->rec_cap);
    DeviceScope scope(h->device);
    hipStream_t s = ctx().stream;
    DZO_TIMED("basin_hopping_hop", s);
    DZO_DISPATCH_RADIAL(h->radial, h->dtype, (bh_launch<T, F>(s, h, num_hops, 0, adapt ? 1 : 0)));
    DZO_HIP(hipGetLastError());
    return DZO_OK;
}

int32_t dzo_basin_hopping_set_record(dzo_basin_hopping_t h, int64_t capacity_hops) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h, DZO_ERR_INVALID, "null handle");
    DZO_REQUIRE(capacity_hops >= 0 && capacity_hops <= ((int64_t)1 << 24), DZO_ERR_INVALID, "capacity_hops must be in 0 .. 2^24 (got %lld)",
                (long long)capacity_hops);
    DeviceScope scope(h->device);
    DZO_HIP(hipStreamSynchronize(ctx().stream));
    bh_free_record(h);
    if (capacity_hops == 0) return DZO_OK;
    const size_t es = dtype_size(h->dtype), n = (size_t)capacity_hops * (size_t)h->B;
    int32_t rc = cl_alloc({{&h->rec_normals, es * 3 * (size_t)h->N * n}, {&h->rec_uniform, es * n}, {&h->rec_trial, es * n},
                           {(void **)&h->rec_iters, 4 * n}, {(void **)&h->rec_code, n}},
                          "the basin-hopping record");
    if (rc != DZO_OK) { bh_free_record(h); return rc; }
    h->rec_cap = capacity_hops;
    DZO_HIP(hipDeviceSynchronize());
    return DZO_OK;
}

int32_t dzo_basin_hopping_get_ptr(dzo_basin_hopping_t h, int32_t what, void **ptr_dev) {
    DZO_REQUIRE(h && ptr_dev, DZO_ERR_INVALID, "null argument");
    size_t bytes = 0;
    return bh_array(h, what, ptr_dev, &bytes);
}

int32_t dzo_basin_hopping_read(dzo_basin_hopping_t h, int32_t what, void *out_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && out_host, DZO_ERR_INVALID, "null argument");
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(bh_array(h, what, &p, &bytes));
    return copy_blocking(out_host, p, bytes, hipMemcpyDeviceToHost);
}

int32_t dzo_basin_hopping_set(dzo_basin_hopping_t h, int32_t what, const void *in_host) {
    DZO_TRY(require_init());
    DZO_REQUIRE(h && in_host, DZO_ERR_INVALID, "null argument");
    DZO_REQUIRE(what == DZO_BASIN_HOPPING_RADII || what == DZO_BASIN_HOPPING_RNG_STATES, DZO_ERR_INVALID,
                "only the perturbation radii and the random states can be set (got %d)", what);
    DeviceScope scope(h->device);
    void *p = nullptr;
    size_t bytes = 0;
    DZO_TRY(bh_array(h, what, &p, &bytes));
    return copy_blocking(p, in_host, bytes, hipMemcpyHostToDevice);
}

}  // extern "C"
