// dzo_symeig_plan.h -- the one DECISION of the batched symmetric eigensolver (dzo_symeig.hip) as a plain function of plain
// inputs, in the manner of dzo_lbfgs_plan.h: where the matrix of an instance lives while it is iterated on, with which leading
// dimension, and how much dynamic LDS the launch asks for.  No HIP here: the header compiles with a plain C++17 compiler and
// the whole range n = 1 .. DZO_SYMEIG_MAX_N is tested on the CPU through dzo_symeig_plan (tests/test_symeig_build.py).
#pragma once

#include <cstdint>

#include "../../include/dzo.h"

namespace dzo {

constexpr int64_t kSymeigLdsLimit = 160 * 1024;             // the LDS of a gfx950 CU: one block, one instance
constexpr int64_t kSymeigRedBytes = 64;                     // the block's reduction cells (four wave sums in fp64, the verdict)

struct SymeigPlan {
    int32_t storage;                                        // DZO_SYMEIG_STORAGE_LDS / DZO_SYMEIG_STORAGE_MEMORY
    int64_t ld;                                             // elements between the columns of the iterated matrix
    int64_t lds_bytes;                                      // dynamic LDS of the launch
};

// Dynamic LDS, in this order: the reduction cells, the angles of a round (c, s per pair: m = n + (n & 1) elements), the
// diagonal for the final rank count (m elements), and on LDS storage the matrix (n columns of ld elements).
//
// ld on LDS storage is the smallest ODD number >= n.  The column phase walks a column (stride 1); the row phase walks a row,
// stride ld elements.  By the bank rule (64 banks of 4 bytes; ds_read_b64 serves 32 lanes per cycle on bank (a / 4) % 64,
// ds_read_b32 and the writes on (a / 4) % 32) a stride of ld doubles is 2 ld dwords: odd ld sends 32 consecutive lanes to the
// 32 distinct even banks, ld = 32 k would send them all to one.  The same holds for ld floats and 32 banks.  On memory storage
// nothing is banked and ld = n.
static inline SymeigPlan symeig_plan(int64_t n, int32_t dtype) {
    const int64_t es = dtype == DZO_F64 ? 8 : 4, m = n + (n & 1);
    const int64_t small = kSymeigRedBytes + 2 * m * es;
    const int64_t ld = n | 1;
    if (small + n * ld * es <= kSymeigLdsLimit) return {DZO_SYMEIG_STORAGE_LDS, ld, small + n * ld * es};
    return {DZO_SYMEIG_STORAGE_MEMORY, n, small};
}

}  // namespace dzo
