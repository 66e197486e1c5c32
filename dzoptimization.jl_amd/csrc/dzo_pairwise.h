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

// The device pieces below are shared by dzo_pairwise.hip and dzo_tempering.hip (one definition, the same bits in both).
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

// `self ? 0 : e(r2)` as a select of two computed values: the term is evaluated in every lane and then dropped (ifelse, :145),
// never branched around -- a conditional EXPRESSION is a branch in the source, and the compiler keeps a branch around a
// division sequence ("skip the expensive operand"): an exec-mask save / restore per pair that is never taken and that keeps
// the independent chains of the four unrolled pairs from being interleaved.  pw_pin makes the value opaque so that the select
// is not turned back into that branch late in code generation.
template <typename T> __device__ __forceinline__ T pw_pin(T v) {
    asm("" : "+v"(v));
    return v;
}
}  // namespace dzo
