// dzo_align.hip -- rigid and permutational alignment of MANY pairs of clusters of identical particles on gfx950: the optimal
// assignment of the particles of B to those of A in the frames given (dzo_align_batch_assign), and the multi-start alternation
// of that assignment with the best proper rotation (dzo_align_batch_pairs).  include/dzo.h has the contract; tests/align_twin.py
// restates it in numpy.
//
// Launch shape.  ONE WAVE per (pair, start): a block of 64 threads, grid batch * n_starts, every wave independent of every
// other.  Lane l owns the columns (particles of B) l + 64 q, q < Q; align_wave_kernel is instantiated for Q = 1, 4 and 16
// (N <= 64, <= 256, <= 1024).  A lane keeps the rotated coordinates, the column potential, the slack and the visited flag (one
// bit of a mask) of its columns in registers.  The centred coordinates of A and the row potentials (fp64) and the column ->
// row, predecessor and previous-cycle arrays (16-bit indices) live in dynamic LDS, 38 N + 8 bytes, and are read wave-uniformly.
// At N = 1024 that is 38 920 bytes: four waves fit the 160 KiB of a compute unit, one per SIMD, which is also what the 512
// VGPRs the Q = 16 form may use allow.  At N <= 64 the LDS is 2.4 KiB and the register file sets the occupancy.
// The argmin of a column scan is a wave reduction of (value, index) through DPP moves and the gfx950 permlane swaps (the
// helpers of dzo_common.h), so a scan needs no workgroup barrier that waits for another wave: the block IS one wave, and the
// __syncthreads() below order its LDS traffic only.
// align_finish_kernel (one wave per pair) picks the best start and writes the outputs; every output element has one writer.
// Every loop is bounded by a count known at entry (a path by N + 1 columns, an augmentation by N + 1 links, the cycles by
// max_cycles, a Jacobi by kAlignSweeps); the choice of the next column is an index taken from a reduction whose candidates are
// unvisited columns only, so a NaN can neither keep a loop alive nor send an index out of range.
#include "dzo_common.h"
#include "dzo_pairwise.h"
#include "dzo_pcg.h"

#include <cmath>

namespace dzo {

constexpr int kAlignMaxN = DZO_ALIGN_MAX_PARTICLES;
constexpr int kAlignSweeps = 12;                             // cyclic Jacobi sweeps of the 3 x 3 and 4 x 4 problems at most
constexpr unsigned short kAlignNone = 0xFFFF;                // "no row" / "no column" in the 16-bit index arrays
constexpr int kAlignRecord = 24;                             // fp64 cells of a start's record (see AlignRecord)
static_assert(kAlignMaxN + 1 < kAlignNone, "indices are kept in 16 bits");
static_assert(kAlignMaxN == 16 * 64, "Q = 16 columns per lane hold the largest cluster");

// what a start leaves for the finish kernel: cells of the fp64 record
enum AlignRecord { kArDistance = 0, kArCycles = 1, kArStatus = 2, kArRotation = 3, kArCentroidA = 12, kArCentroidB = 15 };

struct AlignArgs {
    int N, n_starts, n_orient, n_principal_first, n_random_first;   // orientation o: identity < principal < random
    int max_cycles, assign_only;
    unsigned long long seed;
    const void *a, *b;                                       // T (3N, batch)
    double *records;                                         // (kAlignRecord, batch * n_starts)
    int32_t *perms;                                          // (N, batch * n_starts): row -> column
};

// ------------------------------------------------------------------------------ wave argmin of (value, column)
// the better of two candidates: a candidate without a column loses, then the smaller value, then the lower column.  Symmetric
// in its two arguments, so both partners of an exchange keep the same one.
__device__ __forceinline__ void al_better(double &v, double &c, double ov, double oc) {
    const bool take = oc < 65535.0 && (c >= 65535.0 || ov < v || (!(v < ov) && oc < c));
    v = take ? ov : v;
    c = take ? oc : c;
}
__device__ __forceinline__ void al_swap16(double v, double &x, double &y) {
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u2 rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = __hiloint2double((int)rh.x, (int)rl.x);
    y = __hiloint2double((int)rh.y, (int)rl.y);
}
__device__ __forceinline__ void al_swap32(double v, double &x, double &y) {
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const u2 rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    x = __hiloint2double((int)rh.x, (int)rl.x);
    y = __hiloint2double((int)rh.y, (int)rl.y);
}
// the smallest value of the wave and its column (the lowest column among equal values), the same in every lane: the result
// is read from lane 0, so the lanes agree whatever the values are
__device__ __forceinline__ void al_argmin(double &v, int &col) {
    double c = (double)col;                                  // columns are < 2^16: exact
    al_better(v, c, lane_xor1(v), lane_xor1(c));
    al_better(v, c, lane_xor2(v), lane_xor2(c));
    al_better(v, c, lane_xor4(v), lane_xor4(c));
    al_better(v, c, lane_xor8(v), lane_xor8(c));
    double vx, vy, cx, cy;
    al_swap16(v, vx, vy); al_swap16(c, cx, cy);              // {own, partner} in an order that does not matter
    v = vx; c = cx; al_better(v, c, vy, cy);
    al_swap32(v, vx, vy); al_swap32(c, cx, cy);
    v = vx; c = cx; al_better(v, c, vy, cy);
    v = readlane_f64(v, 0);
    col = (int)readlane_f64(c, 0);
}

// ------------------------------------------------------------------------------ cyclic Jacobi of a small symmetric matrix
// A (D x D, both triangles) becomes diagonal, V its eigenvectors in columns.  Every lane runs it on the same values.  Pairs
// (p, q), p < q, in row order; a pair whose element is exactly zero is skipped; a sweep that finds every element zero ends it.
template <int D> __device__ __forceinline__ void al_jacobi(double (&A)[D][D], double (&V)[D][D]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kAlignSweeps; ++sweep) {
        bool any = false;
#pragma unroll
        for (int p = 0; p < D - 1; ++p) {
#pragma unroll
            for (int q = p + 1; q < D; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0 && apq == apq) {
                    any = true;
                    const double theta = (A[q][q] - A[p][p]) / (apq + apq);
                    const double root = ::sqrt(theta * theta + 1.0);
                    const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
                    const double c = 1.0 / ::sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < D; ++k) {            // columns p and q
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = c * akp - s * akq;
                        A[k][q] = s * akp + c * akq;
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = c * vkp - s * vkq;
                        V[k][q] = s * vkp + c * vkq;
                    }
#pragma unroll
                    for (int k = 0; k < D; ++k) {            // rows p and q
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = c * apk - s * aqk;
                        A[q][k] = s * apk + c * aqk;
                    }
                    A[p][q] = 0.0;
                    A[q][p] = 0.0;
                }
            }
        }
        if (!any) break;
    }
}

// the rotation matrix (row-major) of a quaternion (w, x, y, z) of any length but zero, normalised here
__device__ __forceinline__ void al_quat_rotation(double w, double x, double y, double z, double (&R)[9]) {
    const double n = ::sqrt((w * w + x * x) + (y * y + z * z));
    w /= n; x /= n; y /= n; z /= n;
    R[0] = (w * w + x * x) - (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = (w * w - x * x) + (y * y - z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = (w * w - x * x) - (y * y - z * z);
}

// the right-handed principal frame (columns of F, eigenvalues ascending, ties to the lower index) of the second moments
// m = (xx, xy, xz, yy, yz, zz)
__device__ __forceinline__ void al_principal_frame(const double (&m)[6], double (&F)[3][3]) {
    double A[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}}, V[3][3];
    al_jacobi<3>(A, V);
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    // rank of the first two eigenvalues in the stable ascending order (the third takes the place that is left)
    const int r0 = (e1 < e0) + (e2 < e0), r1 = (e0 <= e1) + (e2 < e1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v0 = V[k][0], v1 = V[k][1], v2 = V[k][2];
        F[k][0] = r0 == 0 ? v0 : r1 == 0 ? v1 : v2;
        F[k][1] = r0 == 1 ? v0 : r1 == 1 ? v1 : v2;
        F[k][2] = r0 == 2 ? v0 : r1 == 2 ? v1 : v2;
    }
    const double det = F[0][0] * (F[1][1] * F[2][2] - F[2][1] * F[1][2]) - F[1][0] * (F[0][1] * F[2][2] - F[2][1] * F[0][2]) +
                       F[2][0] * (F[0][1] * F[1][2] - F[1][1] * F[0][2]);
    if (det < 0.0) { F[0][2] = -F[0][2]; F[1][2] = -F[1][2]; F[2][2] = -F[2][2]; }
}

// ------------------------------------------------------------------------------ one wave per (pair, start): grid batch * n_starts, block 64
template <typename T, int Q> __global__ __launch_bounds__(64) void align_wave_kernel(AlignArgs g) {
    extern __shared__ double al_lds[];
    const int N = g.N, lane = threadIdx.x;
    double *AX = al_lds, *AY = AX + N, *AZ = AY + N, *U = AZ + N;
    unsigned short *rowof = reinterpret_cast<unsigned short *>(U + N);   // N + 1: the row of a column; column N is the virtual one
    unsigned short *way = rowof + (N + 1);                   // N + 1: the column before a column on the path
    unsigned short *prev = way + (N + 1);                    // N: rowof of the previous cycle
    const int64_t wave = blockIdx.x, pair = wave / g.n_starts;
    const int start = (int)(wave - pair * g.n_starts);
    const int inverted = start >= g.n_orient, orient = inverted ? start - g.n_orient : start;
    const T *a = (const T *)g.a + (int64_t)3 * N * pair, *b = (const T *)g.b + (int64_t)3 * N * pair;
    double *rec = g.records + (int64_t)kAlignRecord * wave;
    int32_t *perm_out = g.perms + (int64_t)N * wave;

    // ---- the inputs: non-finite coordinates end the start here; centroids (a lane's particles in order, then the wave tree)
    bool finite = true;
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lane + 64 * q;
        if (j < N) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double va = (double)a[d * N + j], vb = (double)b[d * N + j];
                finite = finite && __builtin_fabs(va) < __builtin_inf() && __builtin_fabs(vb) < __builtin_inf();
                sa[d] += va;
                sb[d] += vb;
            }
        }
    }
    if (__ballot(!finite) != 0) {                            // the whole wave leaves: nothing below has run
        if (lane == 0) {
            rec[kArDistance] = __builtin_nan("");
            rec[kArCycles] = 0.0;
            rec[kArStatus] = (double)DZO_ALIGN_FAILED;
        }
        return;
    }
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
    if (!g.assign_only) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            ca[d] = wave_sum_all(sa[d]) / (double)N;
            cb[d] = wave_sum_all(sb[d]) / (double)N;
        }
    }
    const double sgn = inverted ? -1.0 : 1.0;
    // centred A into LDS, centred (and, for the second half of the starts, inverted) B into registers
    double b0x[Q], b0y[Q], b0z[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lane + 64 * q;
        b0x[q] = b0y[q] = b0z[q] = 0.0;
        if (j < N) {
            AX[j] = (double)a[j] - ca[0];
            AY[j] = (double)a[N + j] - ca[1];
            AZ[j] = (double)a[2 * N + j] - ca[2];
            prev[j] = kAlignNone;
            b0x[q] = sgn * ((double)b[j] - cb[0]);
            b0y[q] = sgn * ((double)b[N + j] - cb[1]);
            b0z[q] = sgn * ((double)b[2 * N + j] - cb[2]);
        }
    }
    __syncthreads();

    // ---- the first rotation of this start
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!g.assign_only && orient >= g.n_principal_first && orient < g.n_random_first) {
        double ma[6] = {0, 0, 0, 0, 0, 0}, mb[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            if (j < N) {
                const double x = AX[j], y = AY[j], z = AZ[j];
                ma[0] += x * x; ma[1] += x * y; ma[2] += x * z; ma[3] += y * y; ma[4] += y * z; ma[5] += z * z;
                const double bx = b0x[q], by = b0y[q], bz = b0z[q];
                mb[0] += bx * bx; mb[1] += bx * by; mb[2] += bx * bz; mb[3] += by * by; mb[4] += by * bz; mb[5] += bz * bz;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) { ma[k] = wave_sum_all(ma[k]); mb[k] = wave_sum_all(mb[k]); }
        double FA[3][3], FB[3][3];
        al_principal_frame(ma, FA);
        al_principal_frame(mb, FB);
        const int k = orient - g.n_principal_first;          // (+,+,+), (+,-,-), (-,+,-), (-,-,+)
        const double s0 = (k == 2 || k == 3) ? -1.0 : 1.0, s1 = (k == 1 || k == 3) ? -1.0 : 1.0, s2 = (k == 1 || k == 2) ? -1.0 : 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[3 * r + c] = (s0 * FA[r][0] * FB[c][0] + s1 * FA[r][1] * FB[c][1]) + s2 * FA[r][2] * FB[c][2];
    } else if (!g.assign_only && orient >= g.n_random_first) {
        const uint64_t r = (uint64_t)(orient - g.n_random_first);
        uint64_t s = pcg_advance(kPcgInc + g.seed);          // the seeded state of the stream
        s = pcg_jump(s, 4ull * r);                           // trial r: draws 4 r .. 4 r + 3, whatever the pair
        const uint32_t d1 = pcg_draw(s), d2 = pcg_draw(s), d3 = pcg_draw(s), d4 = pcg_draw(s);
        const double u1 = ((double)d1 + 0.5) * kTwoM32, u2 = ((double)d2 + 0.5) * kTwoM32;
        const double u3 = ((double)d3 + 0.5) * kTwoM32, u4 = ((double)d4 + 0.5) * kTwoM32;
        const double r1 = ::sqrt(-2.0 * ::log(u1)), r2 = ::sqrt(-2.0 * ::log(u3));
        al_quat_rotation(r1 * ::cospi(2.0 * u2), r1 * ::sinpi(2.0 * u2), r2 * ::cospi(2.0 * u4), r2 * ::sinpi(2.0 * u4), R);
    }

    // ---- the alternation
    unsigned dead = 0;                                       // the columns >= N of this lane
#pragma unroll
    for (int q = 0; q < Q; ++q) dead |= lane + 64 * q < N ? 0u : 1u << q;
    double bx[Q], by[Q], bz[Q], V[Q], slack[Q];
    int cycles = 0, status = DZO_ALIGN_CYCLE_LIMIT;
    const int max_cycles = g.assign_only ? 1 : g.max_cycles;
    for (int cycle = 0; cycle < max_cycles; ++cycle) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            bx[q] = (R[0] * b0x[q] + R[1] * b0y[q]) + R[2] * b0z[q];
            by[q] = (R[3] * b0x[q] + R[4] * b0y[q]) + R[5] * b0z[q];
            bz[q] = (R[6] * b0x[q] + R[7] * b0y[q]) + R[8] * b0z[q];
            V[q] = 0.0;
            const int j = lane + 64 * q;
            if (j < N) { U[j] = 0.0; rowof[j] = kAlignNone; }
        }
        __syncthreads();
        // -- the assignment: rows in index order, each by one shortest augmenting path
        for (int i = 0; i < N; ++i) {
            unsigned used = 0, blocked = dead;               // visited columns; those and the columns >= N
#pragma unroll
            for (int q = 0; q < Q; ++q) slack[q] = __builtin_inf();
            if (lane == 0) rowof[N] = (unsigned short)i;
            __syncthreads();
            int j0 = N;
            for (int step = 0; step <= N; ++step) {          // a path visits at most i + 1 <= N columns
                const int i0 = rowof[j0] < N ? rowof[j0] : 0;   // a row: j0 is the virtual column or a matched one
                const double ax = AX[i0], ay = AY[i0], az = AZ[i0], ui = U[i0];
                if (j0 < N && (j0 & 63) == lane) { used |= 1u << (j0 >> 6); blocked |= 1u << (j0 >> 6); }
                double best = __builtin_inf();
                int col = kAlignNone;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int j = lane + 64 * q;
                    if (!((blocked >> q) & 1u)) {
                        const double dx = ax - bx[q], dy = ay - by[q], dz = az - bz[q];
                        const double cost = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
                        const double cur = (cost - ui) - V[q];
                        if (cur < slack[q]) { slack[q] = cur; way[j] = (unsigned short)j0; }
                        if (slack[q] < best || col == kAlignNone) { best = slack[q]; col = j; }
                    }
                }
                al_argmin(best, col);                        // an unvisited column < N: there are N - (visited <= i) >= 1 of them
                const double delta = best;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if ((used >> q) & 1u) { U[rowof[lane + 64 * q] < N ? rowof[lane + 64 * q] : 0] += delta; V[q] -= delta; }   // matched columns have distinct rows
                    else slack[q] -= delta;                  // (+inf stays +inf on the columns >= N)
                }
                if (lane == 0) U[i] += delta;                // the row of the virtual column
                __syncthreads();
                j0 = col < N ? col : 0;                      // (col is always < N; the clamp keeps the index in range regardless)
                if (rowof[j0] == kAlignNone) break;
            }
            for (int k = 0; k <= N && j0 != N; ++k) {        // augment along the path back to the virtual column
                const int j1 = way[j0] <= N ? way[j0] : N;   // (always <= N; the clamp keeps the index in range regardless)
                if (lane == 0) rowof[j0] = rowof[j1];        // lane 0 alone reads and writes rowof here
                j0 = j1;
            }
            __syncthreads();
        }
        // -- the same permutation as in the previous cycle?
        bool same = true;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            if (j < N) { same = same && prev[j] == rowof[j]; prev[j] = rowof[j]; }
        }
        const bool converged = __ballot(!same) == 0;
        cycles = cycle + 1;
        if (g.assign_only) break;
        // -- the best proper rotation of this assignment (Horn 1987): S_uv = sum b0_u a_v over the matched pairs
        double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int j = lane + 64 * q;
            if (j < N) {
                const int i = rowof[j] < N ? rowof[j] : j;   // (every column has a row; the clamp keeps the index in range regardless)
                const double ax = AX[i], ay = AY[i], az = AZ[i];
                S[0] += b0x[q] * ax; S[1] += b0x[q] * ay; S[2] += b0x[q] * az;
                S[3] += b0y[q] * ax; S[4] += b0y[q] * ay; S[5] += b0y[q] * az;
                S[6] += b0z[q] * ax; S[7] += b0z[q] * ay; S[8] += b0z[q] * az;
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = wave_sum_all(S[k]);
        double H[4][4], E[4][4];
        H[0][0] = (S[0] + S[4]) + S[8];
        H[1][1] = (S[0] - S[4]) - S[8];
        H[2][2] = (S[4] - S[0]) - S[8];
        H[3][3] = (S[8] - S[0]) - S[4];
        H[0][1] = H[1][0] = S[5] - S[7];
        H[0][2] = H[2][0] = S[6] - S[2];
        H[0][3] = H[3][0] = S[1] - S[3];
        H[1][2] = H[2][1] = S[1] + S[3];
        H[1][3] = H[3][1] = S[6] + S[2];
        H[2][3] = H[3][2] = S[5] + S[7];
        al_jacobi<4>(H, E);
        int top = 0;                                         // the largest eigenvalue, the first one among equals
        double ev = H[0][0];
        if (H[1][1] > ev) { ev = H[1][1]; top = 1; }
        if (H[2][2] > ev) { ev = H[2][2]; top = 2; }
        if (H[3][3] > ev) { ev = H[3][3]; top = 3; }
        const double qw = top == 0 ? E[0][0] : top == 1 ? E[0][1] : top == 2 ? E[0][2] : E[0][3];
        const double qx = top == 0 ? E[1][0] : top == 1 ? E[1][1] : top == 2 ? E[1][2] : E[1][3];
        const double qy = top == 0 ? E[2][0] : top == 1 ? E[2][1] : top == 2 ? E[2][2] : E[2][3];
        const double qz = top == 0 ? E[3][0] : top == 1 ? E[3][1] : top == 2 ? E[3][2] : E[3][3];
        al_quat_rotation(qw, qx, qy, qz, R);
        if (converged) { status = DZO_ALIGN_CONVERGED; break; }
    }

    // ---- what the start found: sum |a_i - R b0_p(i)|^2 (or the matched costs), the permutation, the rotation
    double d2 = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = lane + 64 * q;
        if (j < N) {
            const int i = rowof[j] < N ? rowof[j] : j;
            const double rx = (R[0] * b0x[q] + R[1] * b0y[q]) + R[2] * b0z[q];
            const double ry = (R[3] * b0x[q] + R[4] * b0y[q]) + R[5] * b0z[q];
            const double rz = (R[6] * b0x[q] + R[7] * b0y[q]) + R[8] * b0z[q];
            const double dx = AX[i] - rx, dy = AY[i] - ry, dz = AZ[i] - rz;
            d2 += __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
            perm_out[i] = j;                                 // a permutation: one writer per row
        }
    }
    d2 = wave_sum_all(d2);
    if (lane == 0) {
        rec[kArDistance] = g.assign_only ? d2 : ::sqrt(d2);
        rec[kArCycles] = (double)cycles;
        rec[kArStatus] = (double)status;
#pragma unroll
        for (int k = 0; k < 9; ++k) rec[kArRotation + k] = sgn * R[k];
#pragma unroll
        for (int d = 0; d < 3; ++d) { rec[kArCentroidA + d] = ca[d]; rec[kArCentroidB + d] = cb[d]; }
    }
}

// ------------------------------------------------------------------------------ the best start of every pair: grid batch, block 64
template <typename T> struct AlignOut {
    T *aligned;
    int32_t *perm;
    double *rotation, *distance;
    int32_t *best_trial, *cycles, *status;
    double *trial_distances;                                 // or null
};

template <typename T> __global__ __launch_bounds__(64) void align_finish_kernel(AlignArgs g, AlignOut<T> o) {
    const int N = g.N, lane = threadIdx.x, n_starts = g.n_starts;
    const int64_t pair = blockIdx.x;
    const double *recs = g.records + (int64_t)kAlignRecord * n_starts * pair;
    const T *b = (const T *)g.b + (int64_t)3 * N * pair;
    T *x = o.aligned + (int64_t)3 * N * pair;
    const bool failed = recs[kArStatus] == (double)DZO_ALIGN_FAILED;   // every start of a pair sees the same inputs
    int best = 0;
    double dbest = recs[kArDistance];
    for (int t = 1; t < n_starts; ++t) {                     // the first start among equals
        const double d = recs[(int64_t)kAlignRecord * t + kArDistance];
        if (d < dbest) { dbest = d; best = t; }
    }
    if (o.trial_distances)
        for (int t = lane; t < n_starts; t += 64) o.trial_distances[(int64_t)n_starts * pair + t] = recs[(int64_t)kAlignRecord * t + kArDistance];
    if (failed) {
        for (int e = lane; e < 3 * N; e += 64) x[e] = b[e];
        for (int i = lane; i < N; i += 64) o.perm[(int64_t)N * pair + i] = i;
        if (lane < 9) o.rotation[9 * pair + lane] = (lane & 3) == 0 ? 1.0 : 0.0;
        if (lane == 0) {
            o.distance[pair] = __builtin_nan("");
            o.best_trial[pair] = 0;
            o.cycles[pair] = 0;
            o.status[pair] = DZO_ALIGN_FAILED;
        }
        return;
    }
    const double *rec = recs + (int64_t)kAlignRecord * best;
    const int32_t *perm = g.perms + (int64_t)N * ((int64_t)n_starts * pair + best);
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rec[kArRotation + k];
    const double cax = rec[kArCentroidA], cay = rec[kArCentroidA + 1], caz = rec[kArCentroidA + 2];
    const double cbx = rec[kArCentroidB], cby = rec[kArCentroidB + 1], cbz = rec[kArCentroidB + 2];
    for (int i = lane; i < N; i += 64) {
        int j = perm[i];
        j = j >= 0 && j < N ? j : i;                         // a permutation by construction; the clamp keeps the read in range
        const double px = (double)b[j] - cbx, py = (double)b[N + j] - cby, pz = (double)b[2 * N + j] - cbz;
        x[i] = (T)(((R[0] * px + R[1] * py) + R[2] * pz) + cax);
        x[N + i] = (T)(((R[3] * px + R[4] * py) + R[5] * pz) + cay);
        x[2 * N + i] = (T)(((R[6] * px + R[7] * py) + R[8] * pz) + caz);
        o.perm[(int64_t)N * pair + i] = j;
    }
    if (lane < 9) o.rotation[9 * pair + lane] = R[lane];
    if (lane == 0) {
        o.distance[pair] = dbest;
        o.best_trial[pair] = best;
        o.cycles[pair] = (int32_t)rec[kArCycles];
        o.status[pair] = (int32_t)rec[kArStatus];
    }
}

// the assignment alone: the permutation and the cost of the single start of every pair
__global__ __launch_bounds__(64) void align_assign_finish_kernel(AlignArgs g, int32_t *perm, double *cost) {
    const int N = g.N, lane = threadIdx.x;
    const int64_t pair = blockIdx.x;
    const double *rec = g.records + (int64_t)kAlignRecord * pair;
    const bool failed = rec[kArStatus] == (double)DZO_ALIGN_FAILED;
    for (int i = lane; i < N; i += 64) perm[(int64_t)N * pair + i] = failed ? i : g.perms[(int64_t)N * pair + i];
    if (lane == 0) cost[pair] = rec[kArDistance];
}

// ------------------------------------------------------------------------------ host side
static size_t align_lds_bytes(int N) { return (size_t)38 * N + 8; }

template <typename T, int Q> static void align_launch_q(hipStream_t s, int64_t waves, const AlignArgs &g) {
    hipLaunchKernelGGL((align_wave_kernel<T, Q>), dim3((unsigned)waves), dim3(64), align_lds_bytes(g.N), s, g);
}

template <typename T> static void align_launch(hipStream_t s, int64_t waves, const AlignArgs &g) {
    if (g.N <= 64) align_launch_q<T, 1>(s, waves, g);
    else if (g.N <= 256) align_launch_q<T, 4>(s, waves, g);
    else align_launch_q<T, 16>(s, waves, g);
}

template <typename T> static void align_launch_finish(hipStream_t s, int64_t batch, const AlignArgs &g, void *aligned, int32_t *perm, double *rotation,
                                                      double *distance, int32_t *best_trial, int32_t *cycles, int32_t *status, double *trial_distances) {
    hipLaunchKernelGGL(align_finish_kernel<T>, dim3((unsigned)batch), dim3(64), 0, s, g,
                       AlignOut<T>{(T *)aligned, perm, rotation, distance, best_trial, cycles, status, trial_distances});
}

static int32_t align_check_sizes(int64_t n_particles, int64_t batch, int32_t dtype) {
    DZO_REQUIRE(dtype == DZO_F32 || dtype == DZO_F64, DZO_ERR_INVALID, "bad dtype %d", dtype);
    DZO_REQUIRE(n_particles >= 1, DZO_ERR_INVALID, "n_particles must be at least 1 (got %lld)", (long long)n_particles);
    DZO_REQUIRE(batch >= 1 && batch <= ((int64_t)1 << 30), DZO_ERR_INVALID, "batch must be in 1 .. 2^30 (got %lld)", (long long)batch);
    DZO_REQUIRE(n_particles <= kAlignMaxN, DZO_ERR_UNSUPPORTED, "n_particles = %lld: the alignment kernels hold a pair in one wave, up to %d particles",
                (long long)n_particles, kAlignMaxN);
    return DZO_OK;
}

// the workspace of `waves` starts: their records, then their permutations
static int32_t align_workspace(int64_t waves, int N, void **ws, AlignArgs &g) {
    const size_t rec_bytes = (size_t)waves * kAlignRecord * sizeof(double);
    DZO_TRY(device_alloc(ws, rec_bytes + (size_t)waves * N * sizeof(int32_t), "the per-start records of the alignment", false));
    g.records = (double *)*ws;
    g.perms = (int32_t *)((char *)*ws + rec_bytes);
    return DZO_OK;
}

}  // namespace dzo

using namespace dzo;

extern "C" {

int32_t dzo_align_batch_assign(int64_t n_particles, int64_t batch, int32_t dtype, const void *a_dev, const void *b_dev, int32_t *perm_dev,
                               double *cost_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(a_dev && b_dev && perm_dev && cost_dev, DZO_ERR_INVALID, "null argument");
    DZO_TRY(align_check_sizes(n_particles, batch, dtype));
    const char *where = "dzo_align_batch_assign", *cite = "include/dzo.h";
    DZO_TRY(require_same_backend(where, cite, a_dev, "a", b_dev, "b"));
    DZO_TRY(require_same_backend(where, cite, a_dev, "a", perm_dev, "perm"));
    DZO_TRY(require_same_backend(where, cite, a_dev, "a", cost_dev, "cost"));
    Context &c = ctx();
    AlignArgs g{};
    g.N = (int)n_particles; g.n_starts = 1; g.n_orient = 1; g.n_principal_first = 1; g.n_random_first = 1; g.max_cycles = 1; g.assign_only = 1;
    g.a = a_dev; g.b = b_dev;
    void *ws = nullptr;
    DZO_TRY(align_workspace(batch, g.N, &ws, g));
    int32_t rc = [&]() -> int32_t {
        {
            DZO_TIMED("align_assign", c.stream);
            DZO_DISPATCH(dtype, align_launch<T>(c.stream, batch, g));
            DZO_HIP(hipGetLastError());
            hipLaunchKernelGGL(align_assign_finish_kernel, dim3((unsigned)batch), dim3(64), 0, c.stream, g, perm_dev, cost_dev);
            DZO_HIP(hipGetLastError());
        }
        DZO_HIP(hipStreamSynchronize(c.stream));
        return DZO_OK;
    }();
    (void)hipFree(ws);
    return rc;
}

int32_t dzo_align_batch_pairs(int64_t n_particles, int64_t batch, int32_t dtype, const void *a_dev, const void *b_dev, int32_t trials,
                              int32_t random_trials, int32_t max_cycles, int32_t allow_inversion, uint64_t seed, void *aligned_dev,
                              int32_t *perm_dev, double *rotation_dev, double *distance_dev, int32_t *best_trial_dev, int32_t *cycles_dev,
                              int32_t *status_dev, double *trial_distances_dev) {
    DZO_TRY(require_init());
    DZO_REQUIRE(a_dev && b_dev && aligned_dev && perm_dev && rotation_dev && distance_dev && best_trial_dev && cycles_dev && status_dev,
                DZO_ERR_INVALID, "null argument");
    DZO_TRY(align_check_sizes(n_particles, batch, dtype));
    DZO_REQUIRE(trials >= 0 && (trials & ~(DZO_ALIGN_TRIAL_IDENTITY | DZO_ALIGN_TRIAL_PRINCIPAL)) == 0, DZO_ERR_INVALID, "unknown bits in trials = %d", trials);
    DZO_REQUIRE(random_trials >= 0, DZO_ERR_INVALID, "random_trials must not be negative (got %d)", random_trials);
    DZO_REQUIRE(trials != 0 || random_trials != 0, DZO_ERR_INVALID, "no start: trials == 0 and random_trials == 0");
    DZO_REQUIRE(max_cycles >= 1, DZO_ERR_INVALID, "max_cycles must be at least 1 (got %d)", max_cycles);
    DZO_REQUIRE(random_trials <= DZO_ALIGN_MAX_RANDOM_TRIALS, DZO_ERR_UNSUPPORTED, "random_trials = %d: up to %d (the stream rule reserves that many per pair)",
                random_trials, DZO_ALIGN_MAX_RANDOM_TRIALS);
    DZO_REQUIRE(max_cycles <= DZO_ALIGN_MAX_CYCLES, DZO_ERR_UNSUPPORTED, "max_cycles = %d: up to %d", max_cycles, DZO_ALIGN_MAX_CYCLES);
    const char *where = "dzo_align_batch_pairs", *cite = "include/dzo.h";
    for (const void *p : {b_dev, (const void *)aligned_dev, (const void *)perm_dev, (const void *)rotation_dev, (const void *)distance_dev,
                          (const void *)best_trial_dev, (const void *)cycles_dev, (const void *)status_dev, (const void *)trial_distances_dev})
        DZO_TRY(require_same_backend(where, cite, a_dev, "a", p, "every other array"));
    Context &c = ctx();
    AlignArgs g{};
    g.N = (int)n_particles;
    g.n_principal_first = (trials & DZO_ALIGN_TRIAL_IDENTITY) ? 1 : 0;
    g.n_random_first = g.n_principal_first + ((trials & DZO_ALIGN_TRIAL_PRINCIPAL) ? 4 : 0);
    g.n_orient = g.n_random_first + random_trials;
    g.n_starts = (allow_inversion ? 2 : 1) * g.n_orient;
    g.max_cycles = max_cycles; g.assign_only = 0; g.seed = seed;
    g.a = a_dev; g.b = b_dev;
    const int64_t waves = batch * g.n_starts;
    DZO_REQUIRE(waves <= ((int64_t)1 << 31) - 1, DZO_ERR_UNSUPPORTED, "batch * n_starts = %lld: one launch holds up to 2^31 - 1 waves", (long long)waves);
    void *ws = nullptr;
    DZO_TRY(align_workspace(waves, g.N, &ws, g));
    int32_t rc = [&]() -> int32_t {
        {
            DZO_TIMED("align_starts", c.stream);
            DZO_DISPATCH(dtype, align_launch<T>(c.stream, waves, g));
            DZO_HIP(hipGetLastError());
        }
        {
            DZO_TIMED("align_finish", c.stream);
            DZO_DISPATCH(dtype, align_launch_finish<T>(c.stream, batch, g, aligned_dev, perm_dev, rotation_dev, distance_dev, best_trial_dev, cycles_dev,
                                                       status_dev, trial_distances_dev));
            DZO_HIP(hipGetLastError());
        }
        DZO_HIP(hipStreamSynchronize(c.stream));
        return DZO_OK;
    }();
    (void)hipFree(ws);
    return rc;
}

}  // extern "C"
