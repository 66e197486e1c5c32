// dzo_chain.h -- the asynchronous launch paths behind three blocking entry points, for a unit that chains them on one stream
// without a host wait in between (dzo_modefollow.hip: Hessian, eigensolver, step; dzo_hybridef.hip: lowest mode, step).  The
// arguments are the entry points' and have been checked by the caller; the kernels and what the entry points themselves do are
// untouched.
#pragma once
#include "dzo_common.h"

namespace dzo {

// dzo_pairwise_batch_hessian (dzo_hessian_batch.hip): hessians[b] of points[b], (3N, 3N, batch), enqueued on s
int32_t hb_enqueue_hessian(hipStream_t s, int32_t radial, int32_t dtype, int N, int64_t batch, const void *points, void *hessians);

// dzo_symmetric_batch_eigen (dzo_symeig.hip).  se_prepare once per (n, dtype) and device before the first launch: the LDS
// attribute of the kernel.  se_enqueue: the launch on s; `work` is the (n, n, batch) workspace of MEMORY storage (null on LDS
// storage; dzo_symeig_plan tells), owned by the caller for as long as the launch runs.
int32_t se_prepare(int64_t n, int32_t dtype);
int32_t se_enqueue(hipStream_t s, int64_t n, int64_t batch, int32_t dtype, const void *matrices, void *work, void *eigenvalues, void *eigenvectors,
                   int32_t *sweeps, int32_t max_sweeps);

// dzo_pairwise_batch_lowest_mode (dzo_lowmode.hip).  lm_prepare once per (radial, N, krylov, dtype) and device before the first launch:
// the LDS attribute of the kernel.  lm_enqueue: the launch on s, no host wait; `basis` is the Lanczos workspace of 3N * krylov *
// batch elements for N > 64 (null up to 64, where the basis lives in LDS), owned by the caller for as long as the launch runs.
int32_t lm_prepare(int32_t radial, int32_t dtype, int N, int krylov, int project_rigid);
int32_t lm_enqueue(hipStream_t s, int32_t radial, int32_t dtype, int N, int64_t batch, const void *points, int32_t project_rigid, int32_t krylov, int32_t max_cycles,
                   double res_tol, uint64_t base_seed, const void *start, void *basis, void *eigenvalues, void *vectors, double *residuals,
                   int32_t *info);

}  // namespace dzo
