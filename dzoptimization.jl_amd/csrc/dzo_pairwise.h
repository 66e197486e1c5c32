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
}  // namespace dzo
