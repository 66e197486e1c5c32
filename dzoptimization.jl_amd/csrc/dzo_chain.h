// dzo_chain.h -- the asynchronous launch paths behind two blocking entry points, for a unit that chains them on one stream
// without a host wait in between (dzo_modefollow.hip: Hessian, eigensolver, step).  The arguments are the entry points' and
// have been checked by the caller; the kernels and what the entry points themselves do are untouched.
#pragma once
#include "dzo_common.h"

namespace dzo {

// dzo_pairwise_batch_hessian (dzo_hessian_batch.hip): hessians[b] of points[b], (3N, 3N, batch), enqueued on s
int32_t hb_enqueue_hessian(hipStream_t s, int32_t dtype, int N, int64_t batch, const void *points, void *hessians);

// dzo_symmetric_batch_eigen (dzo_symeig.hip).  se_prepare once per (n, dtype) and device before the first launch: the LDS
// attribute of the kernel.  se_enqueue: the launch on s; `work` is the (n, n, batch) workspace of MEMORY storage (null on LDS
// storage; dzo_symeig_plan tells), owned by the caller for as long as the launch runs.
int32_t se_prepare(int64_t n, int32_t dtype);
int32_t se_enqueue(hipStream_t s, int64_t n, int64_t batch, int32_t dtype, const void *matrices, void *work, void *eigenvalues, void *eigenvectors,
                   int32_t *sweeps, int32_t max_sweeps);

}  // namespace dzo
