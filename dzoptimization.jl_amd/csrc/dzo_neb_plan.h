// dzo_neb_plan.h -- the one DECISION of the batched nudged elastic band (dzo_neb.hip) as a plain function of plain inputs, in
// the manner of dzo_symeig_plan.h: which launch shape serves a band, where its points, velocities and forces live while a
// launch iterates on it, and how much dynamic LDS the launch asks for.  No HIP here: the header compiles with a plain C++17
// compiler and its edges are tested on the CPU through dzo_neb_plan (tests/test_neb_build.py).
#pragma once

#include <cstdint>

#include "../../include/dzo.h"

namespace dzo {

constexpr int64_t kNebLdsLimit = 160 * 1024 - 1024;        // kClLdsMax: the dynamic LDS the cluster units allow a launch
// the block's reduction cells (2 x 4 wave sums), F.F of every image, E of every image and the kernel's copy of its arguments
// (24 cells), 8 bytes each
constexpr int64_t kNebSmallBytes = 8 * (2 * 4 + 2 * DZO_NEB_MAX_IMAGES + 24);

struct NebPlan {
    int32_t shape;                                          // DZO_NEB_SHAPE_WAVE / DZO_NEB_SHAPE_BLOCK
    int32_t storage;                                        // DZO_NEB_STORAGE_LDS / DZO_NEB_STORAGE_MEMORY
    int64_t lds_bytes;                                      // dynamic LDS of the launch
};

// Dynamic LDS, in this order: the small cells, in the BLOCK shape the stage of the image under evaluation (3N elements: the
// pair loop of cl_block_eval reads it N times per particle), and on LDS storage the band, its velocities and its forces
// (3 arrays of 3N M elements).  One block serves one band, and a band's state is touched about ten times per iteration
// between barriers, so it is kept in LDS whenever everything fits what a launch may ask for; a band that does not fit is
// iterated on in device memory (the caller's band, the handle's velocities and forces), where it stays in L2.  There is no
// in-between: with part of the state in LDS the kernel body would need two address spaces per array for no measured gain.
// The WAVE shape (N <= 64) always fits: 3 * 32 images * 192 elements * 8 bytes = 144 KiB.  LDS is allotted per block, so a
// small band leaves room for several blocks per CU and a large one takes the CU alone, which is what a band per block wants
// up to 256 bands; nothing here is rounded up beyond the request.
static inline NebPlan neb_plan(int64_t n_particles, int64_t n_images, int32_t dtype) {
    const int64_t es = dtype == DZO_F64 ? 8 : 4, n = 3 * n_particles;
    const int32_t shape = n_particles <= 64 ? DZO_NEB_SHAPE_WAVE : DZO_NEB_SHAPE_BLOCK;
    const int64_t fixed = kNebSmallBytes + (shape == DZO_NEB_SHAPE_BLOCK ? n * es : 0);
    const int64_t state = 3 * n * n_images * es;
    if (fixed + state <= kNebLdsLimit) return {shape, DZO_NEB_STORAGE_LDS, fixed + state};
    return {shape, DZO_NEB_STORAGE_MEMORY, fixed};
}

}  // namespace dzo
