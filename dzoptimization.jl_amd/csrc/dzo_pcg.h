// dzo_pcg.h -- the PCG32 XSH-RR generator (legacy/PCG.jl:7-22) and the draws built on it, shared by dzo_tempering.hip and
// dzo_basin_hopping.hip.  The stream rule is stated in include/dzo.h; tests/tempering_twin.py and tests/basin_twin.py replay it.
// The integer part compiles under hipcc (__host__ __device__) and under a plain C++17 compiler (tools/pcg_jump_table.cpp);
// the floating-point part (Box-Muller on the device's fp64 log / sqrt / cospi / sinpi) is for kernels only.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define DZO_PCG_FN __host__ __device__ __forceinline__
#else
#define DZO_PCG_FN inline
#endif

namespace dzo {

constexpr uint64_t kPcgMul = 0x5851F42D4C957F2DULL, kPcgInc = 0x14057B7EF767814FULL;

DZO_PCG_FN uint64_t pcg_advance(uint64_t s) { return kPcgMul * s + kPcgInc; }

DZO_PCG_FN uint32_t pcg_extract(uint64_t s) {
    const uint32_t v = (uint32_t)(((s >> 18) ^ s) >> 27);
    const uint32_t r = (uint32_t)(s >> 59);
    return (v >> r) | (v << ((32u - r) & 31u));             // bitrotate(v, -r)
}

DZO_PCG_FN uint32_t pcg_draw(uint64_t &s) {
    const uint32_t v = pcg_extract(s);
    s = pcg_advance(s);
    return v;
}

// k advances at once are one affine map s' = A_k s + C_k with A_k = A^k and C_k = (A^(k-1) + ... + A + 1) C (mod 2^64): the
// LCG skip, built by squaring from the bits of k in O(log k) multiplications.  A caller that jumps by the same k again and again
// keeps the map (the lanes of a basin-hopping kernel do).
struct PcgMap { uint64_t a, c; };

DZO_PCG_FN PcgMap pcg_jump_map(uint64_t k) {
    PcgMap r{1, 0};                                          // the map of the bits of k taken so far
    uint64_t a = kPcgMul, c = kPcgInc;                       // the map of 2^bit advances
    for (; k != 0; k >>= 1) {
        if (k & 1) { r.a *= a; r.c = r.c * a + c; }
        c *= a + 1;
        a *= a;
    }
    return r;
}

DZO_PCG_FN uint64_t pcg_apply(const PcgMap &m, uint64_t s) { return m.a * s + m.c; }

DZO_PCG_FN uint64_t pcg_jump(uint64_t s, uint64_t k) { return pcg_apply(pcg_jump_map(k), s); }

constexpr double kTwoM32 = 2.3283064365386962890625e-10;    // 2^-32

// _fac of scripts/MonteCarlo.jl:21-24 = ten successive square roots of two in T, on the host (its sqrt is correctly rounded)
template <typename T> inline double mc_fac() {
    T f = T(2);
    for (int i = 0; i < 10; ++i) f = std::sqrt(f);
    return (double)f;
}

#ifdef __HIPCC__
// the radius adaptation of scripts/MonteCarlo.jl:77-81 on the counts of one call, capped at 1
template <typename T> __device__ __forceinline__ T mc_adapted_radius(T radius, int64_t acc, int64_t rej, T fac) {
    T r = radius;
    if (3 * acc < rej) r = radius / fac;
    else if (3 * acc > rej) { const T v = radius * fac; r = v < T(1) ? v : T(1); }
    return r;
}

// the acceptance uniform of a draw: d 2^-32 in fp64 (exact), rounded to T; in [0, 1]
template <typename T> __device__ __forceinline__ T pcg_uniform(uint32_t d) { return (T)((double)d * kTwoM32); }

// the exponential of the Metropolis test, in T
template <typename T> __device__ __forceinline__ T mc_exp(T v);
template <> __device__ __forceinline__ double mc_exp<double>(double v) { return ::exp(v); }
template <> __device__ __forceinline__ float mc_exp<float>(float v) { return ::expf(v); }

// three normals of four draws (Box-Muller in fp64, each rounded to T; the fourth normal is not used)
template <typename T> __device__ __forceinline__ void pcg_normals(uint32_t d1, uint32_t d2, uint32_t d3, uint32_t d4, T &nx, T &ny, T &nz) {
    const double u1 = ((double)d1 + 0.5) * kTwoM32, u2 = ((double)d2 + 0.5) * kTwoM32;   // exact
    const double u3 = ((double)d3 + 0.5) * kTwoM32, u4 = ((double)d4 + 0.5) * kTwoM32;
    const double r1 = ::sqrt(-2.0 * ::log(u1)), r2 = ::sqrt(-2.0 * ::log(u3));
    const double c1 = ::cospi(2.0 * u2), s1 = ::sinpi(2.0 * u2), c2 = ::cospi(2.0 * u4);
    nx = (T)(r1 * c1);
    ny = (T)(r1 * s1);
    nz = (T)(r2 * c2);
}
#endif

}  // namespace dzo
