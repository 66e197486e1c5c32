// dzo_pairwise.h -- internal interface of the pairwise radial (Lennard-Jones) N-body objective (see dzo_pairwise.hip).
#pragma once
#include "dzo_common.h"

namespace dzo {
// doubles of device workspace the launchers below need for N particles on the current device (row partials of a
// split j range, per-block / per-row energy partials)
int64_t pairwise_workspace_doubles(int64_t n_particles);
// E = sum_i 1/2 sum_{j != i} e(r2_ij) into result_dev[0] (fp64; device or pinned host), enqueued on s, no host wait
int32_t pairwise_energy_async(hipStream_t s, int32_t radial, int64_t n_particles, int32_t dtype, const void *x, const void *y,
                              const void *z, double *ws, double *result_dev);
// g_i = 2 sum_{j != i} e'(r2_ij) (r_i - r_j), enqueued on s
int32_t pairwise_gradient_async(hipStream_t s, int32_t radial, int64_t n_particles, int32_t dtype, void *gx, void *gy, void *gz,
                                const void *x, const void *y, const void *z, double *ws);

// ------------------------------------------------------------------------------ host helpers of the units built on this header
// hipMalloc (at least 16 bytes) of a piece of `what_for`, cleared when `zero_fill`; DZO_ERR_NOMEM with `what_for` in the message
int32_t device_alloc(void **p, size_t bytes, const char *what_for, bool zero_fill);
// The argument checks of every entry point that takes `count` sets of n_particles particles, in this order: radial, dtype,
// n_particles >= 1, count in 1 .. 2^30 (DZO_ERR_INVALID, `count_name` in the message), n_particles <= max_particles (`over_max`;
// `holder` says what holds that many).
int32_t pw_check_args(int32_t radial, int32_t dtype, int64_t n_particles, int64_t count, const char *count_name, int64_t max_particles,
                      int32_t over_max, const char *holder);
// `bytes` of a handle's array to or from the host on the current context's stream; returns when they have arrived
int32_t copy_blocking(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);

// The device pieces below are shared by dzo_pairwise.hip, dzo_tempering.hip, dzo_hessian_batch.hip and, through dzo_cluster.h,
// dzo_lbfgs_batch.hip and dzo_adgd_batch.hip (one definition, the same bits in all of them).
// ------------------------------------------------------------------------------ radial functions (:16-72)
template <typename T> __device__ __forceinline__ T pw_twice(T a) { return a + a; }
template <typename T> __device__ __forceinline__ T pw_square(T a) { return a * a; }

template <typename T> struct LJRadial {
    // lj_energy :16-27
    static __device__ __forceinline__ T energy(T r2) {
        const T inv_r2 = T(1) / r2;                          // inv, :22 (IEEE division)
        const T inv_r4 = pw_square(inv_r2);
        const T inv_r6 = inv_r4 * inv_r2;
        return T(4) * dfma<T>(inv_r6, inv_r6, -inv_r6);
    }
    // lj_first_derivative :30-47
    static __device__ __forceinline__ T first(T r2) {
        const T inv_r2 = T(1) / r2;
        const T inv_r4 = pw_square(inv_r2);
        const T inv_r6 = inv_r4 * inv_r2;
        const T inv_r8 = pw_square(inv_r4);
        return T(-12) * dfma<T>(inv_r8, pw_twice(inv_r6), -inv_r8);
    }
    // lj_second_derivative :50-72
    static __device__ __forceinline__ T second(T r2) {
        const T inv_r2 = T(1) / r2;
        const T inv_r4 = pw_square(inv_r2);
        const T inv_r8 = pw_square(inv_r4);
        const T inv_r10 = inv_r8 * inv_r2;
        return T(48) * dfma<T>(T(3.5), pw_square(inv_r8), -inv_r10);
    }
};

// The Morse pair term in reduced units (pair minimum at r = 1, depth 1): E(r) = t^2 - 2 t, t = exp(RHO (1 - r)), as functions of
// r2 like the above (derivatives with respect to r2, not r).  RHO is a template integer: one more range is one more line in
// DZO_RADIAL_CASES_ and one more constant in include/dzo.h.  One fixed operation order, every fma written out:
//   r = sqrt(r2) (IEEE), a = RHO * (1 - r), t = exp(a) (the device library's exp / expf), tm1 = t - 1
//   energy = fma(t, t, -(t + t))
//   first  = ((-RHO * t) * tm1) / r                                      dE/d(r2) = -RHO t (t - 1) / r
//   second = ((RHO * t) * fma(RHO * r, (t + t) - 1, tm1)) / ((r2 + r2) * r)   d2E/d(r2)2 = RHO t (RHO r (2t - 1) + (t - 1)) / (2 r2 r)
// r, t and tm1 are the same expressions in all three members, so a kernel that calls two of them on one r2 computes one square
// root and one exp per pair (checked in the gfx950 code of the quench, hvp and tempering kernels).
// At r2 = 0 (self term, padding) first and second are infinite or NaN and the energy is finite; all three are dropped by the
// caller's select like the Lennard-Jones values.
template <typename T> __device__ __forceinline__ T pw_sqrt(T v);
template <> __device__ __forceinline__ double pw_sqrt<double>(double v) { return __builtin_sqrt(v); }
template <> __device__ __forceinline__ float pw_sqrt<float>(float v) { return __builtin_sqrtf(v); }
template <typename T> __device__ __forceinline__ T pw_exp(T v);
template <> __device__ __forceinline__ double pw_exp<double>(double v) { return ::exp(v); }
template <> __device__ __forceinline__ float pw_exp<float>(float v) { return ::expf(v); }

template <typename T, int RHO> struct MorseRadial {
    static __device__ __forceinline__ T decay(T r) { return pw_exp<T>(T(RHO) * (T(1) - r)); }   // t
    static __device__ __forceinline__ T energy(T r2) {
        const T t = decay(pw_sqrt<T>(r2));
        return dfma<T>(t, t, -pw_twice(t));
    }
    static __device__ __forceinline__ T first(T r2) {
        const T r = pw_sqrt<T>(r2);
        const T t = decay(r);
        const T tm1 = t - T(1);
        return ((T(-RHO) * t) * tm1) / r;                    // IEEE division
    }
    static __device__ __forceinline__ T second(T r2) {
        const T r = pw_sqrt<T>(r2);
        const T t = decay(r);
        const T tm1 = t - T(1);
        const T inner = dfma<T>(T(RHO) * r, pw_twice(t) - T(1), tm1);
        return ((T(RHO) * t) * inner) / (pw_twice(r2) * r);
    }
};

// The Riesz (Coulomb, s = 1) pair term 1 / r of legacy/ExampleFunctions.jl:30-83, as functions of r2 like the above:
//   r = sqrt(r2) (IEEE), inv_r = 1 / r
//   energy = inv_r
//   first  = -0.5 * (inv_r / r2)                  inv_r / r2 is the reference's inv_dist_cubed (:62)
//   second = 0.75 * ((inv_r / r2) / r2)
// The scaling by 1/2 and the caller's doubling are exact, so a gradient term 2 first (r_i - r_j) has the bits of the reference's
// dist * inv_dist_cubed.  At r2 = 0 all three are infinite or NaN and are dropped by the caller's select.  Not a DZO_RADIAL_*:
// only the kernels of dzo_sphere.hip use it, and it does not pass through DZO_DISPATCH_RADIAL.
template <typename T> struct RieszRadial {
    static __device__ __forceinline__ T energy(T r2) { return T(1) / pw_sqrt<T>(r2); }
    static __device__ __forceinline__ T first(T r2) {
        const T inv_r = T(1) / pw_sqrt<T>(r2);
        return T(-0.5) * (inv_r / r2);
    }
    static __device__ __forceinline__ T second(T r2) {
        const T inv_r = T(1) / pw_sqrt<T>(r2);
        return T(0.75) * ((inv_r / r2) / r2);
    }
};

// (radial, dtype) -> (T, F): the statement runs with `using T` and `using F` of the selected pair; an unknown selector or type
// leaves the calling function with DZO_ERR_INVALID (pw_check_args has the message for callers that check first).  Every
// launch and every kernel-pointer lookup that depends on the radial goes through this one table.
#define DZO_RADIAL_CASES_(radial, ...)                                                                    \
    if ((radial) == DZO_RADIAL_LENNARD_JONES) { using F = ::dzo::LJRadial<T>; __VA_ARGS__; }              \
    else if ((radial) == DZO_RADIAL_MORSE_RHO6) { using F = ::dzo::MorseRadial<T, 6>; __VA_ARGS__; }      \
    else if ((radial) == DZO_RADIAL_MORSE_RHO14) { using F = ::dzo::MorseRadial<T, 14>; __VA_ARGS__; }    \
    else { ::dzo::set_error("unknown radial function %d", (int)(radial)); return DZO_ERR_INVALID; }
#define DZO_DISPATCH_RADIAL(radial, dtype, ...)                                                           \
    do {                                                                                                  \
        if ((dtype) == DZO_F64) { using T = double; DZO_RADIAL_CASES_(radial, __VA_ARGS__) }              \
        else if ((dtype) == DZO_F32) { using T = float; DZO_RADIAL_CASES_(radial, __VA_ARGS__) }          \
        else { ::dzo::set_error("bad dtype %d", (int)(dtype)); return DZO_ERR_INVALID; }                  \
    } while (0)

// `self ? 0 : e(r2)` as a select of two computed values: the term is evaluated in every lane and then dropped (ifelse, :145),
// never branched around -- a conditional EXPRESSION is a branch in the source, and the compiler keeps a branch around a
// division sequence ("skip the expensive operand"): an exec-mask save / restore per pair that is never taken and that keeps
// the independent chains of the four unrolled pairs from being interleaved.  pw_pin makes the value opaque so that the select
// is not turned back into that branch late in code generation.
template <typename T> __device__ __forceinline__ T pw_pin(T v) {
    asm("" : "+v"(v));
    return v;
}
// The same for an address.  Pointers that a kernel uses again when its loop ends are kept in VECTOR registers: as kernel
// arguments they would sit in scalar registers through the whole loop next to the scalarised integer arithmetic, and the
// allocator then spills scalars.
template <typename P> __device__ __forceinline__ P *pw_pin_ptr(P *p) {
    asm("" : "+v"(p));
    return p;
}

// ------------------------------------------------------------------------------ the pair term
// what pw_pair adds up: e (into ax), e' (r_i - r_j), the hvp's row, or e (into *row) and e' (r_i - r_j) from one r2
enum { kPwEnergy = 0, kPwGradient = 1, kPwHvp = 2, kPwEnergyGradient = 3 };

template <typename T> struct PwPoint { T x, y, z, u, v, w; };   // u, v, w: the hvp's direction (zero elsewhere)

// the squared distance, summed in this order everywhere
template <typename T> __device__ __forceinline__ T pw_r2(T dx, T dy, T dz) {
    const T r2 = pw_square(dx) + pw_square(dy) + pw_square(dz);
    return r2;
}

// e(r2) of the pair (px, py, pz) - (xj, yj, zj), pinned and RETURNED; the caller drops the self term with a select.  Kept apart
// from pw_pair<T, F, kPwEnergy> on a zero accumulator: that form compiles to other code in the delta and tempering kernels.
template <typename T, typename F> __device__ __forceinline__ T pw_pair_energy(T px, T py, T pz, T xj, T yj, T zj) {
    return pw_pin(F::energy(pw_r2(px - xj, py - yj, pz - zj)));
}

// one (i, j) term of :137-146 / :245-257 / :395-419 added to the accumulators (`row`: kPwEnergyGradient only); `self` = (i == j) or padding
template <typename T, typename F, int MODE>
__device__ __forceinline__ void pw_pair(bool self, const PwPoint<T> &pi, const PwPoint<T> &pj, T &ax, T &ay, T &az, T *row = nullptr) {
    const T dx = pi.x - pj.x;
    const T dy = pi.y - pj.y;
    const T dz = pi.z - pj.z;
    const T r2 = pw_r2(dx, dy, dz);
    if constexpr (MODE == kPwEnergy) {
        const T e = pw_pin(F::energy(r2));
        ax += self ? T(0) : e;
    } else if constexpr (MODE == kPwGradient) {
        const T f1 = pw_pin(F::first(r2));
        const T f = self ? T(0) : f1;
        ax += f * dx;
        ay += f * dy;
        az += f * dz;
    } else if constexpr (MODE == kPwEnergyGradient) {
        const T e = pw_pin(F::energy(r2));
        const T f1 = pw_pin(F::first(r2));
        *row += self ? T(0) : e;
        const T f = self ? T(0) : f1;
        ax += f * dx;
        ay += f * dy;
        az += f * dz;
    } else {
        const T du = pi.u - pj.u;
        const T dv = pi.v - pj.v;
        const T dw = pi.w - pj.w;
        const T f1 = pw_pin(F::first(r2));
        const T f = self ? T(0) : f1;
        const T s2 = pw_pin(F::second(r2));
        const T s = self ? T(0) : s2;
        const T overlap = dx * du + dy * dv + dz * dw;
        const T g = pw_twice(overlap * s);
        ax += f * du + g * dx;
        ay += f * dv + g * dy;
        az += f * dw + g * dz;
    }
}
}  // namespace dzo
